// gossip_protocol_amd/csrc/audit_kernels.hpp -- the view audit of both scale engines, the
// row-wise twin of the census (census_kernels.hpp): for every alive observer r, over the entries
// its view stores at the engine's current tick T, how many there are (size), how many name a
// member that is not alive (dead), how many alive members' entries are age_limit ticks old or
// older (suspect), the sum and the maximum of the age over the alive members' entries (age_sum,
// age_max) and the 64-bit fingerprint of the view (print: the sum mod 2^64 of audit_fp(x) over
// the stored ids; the host adds audit_fp(r) at readback).  One streaming pass per call; no tick
// kernel is involved.  A row r is read iff start[r] <= T <= crash[r] (policy.hpp): a crashed
// row's buffer is stale and a row that has not started is empty.
//
// The full view accumulates into n-length arrays the host zeroed, with integer atomics only, so
// the result is exact and does not depend on the order the shards, tiles or workgroups run in;
// the partial view holds a row in one shard and stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsp {

constexpr int kAuditStrip = 512;     // full view: columns of one wave instruction (16 B per lane)
#ifndef GSP_AUDIT_STRIPS             // A/B only (make lib-variant VFLAGS=-DGSP_AUDIT_STRIPS=1|2|4)
#define GSP_AUDIT_STRIPS 4
#endif
constexpr int kAuditStrips = GSP_AUDIT_STRIPS;   // full view: strips a wave owns, 2,048 columns of a row
constexpr int kAuditRows = 256;      // full view: rows of a work item, interleaved over 4 waves

// the per-row arrays on the device: kAuditFields x n uint32, then print
enum { kAudSize = 0, kAudDead, kAudSuspect, kAudAgeSum, kAudAgeMax, kAuditFields };

// The fingerprint of one id: the splitmix64 finaliser (event_mix's, scale_row.hpp).
__host__ __device__ inline uint64_t audit_fp(uint32_t x) {
    uint64_t z = uint64_t(x) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The per-column truth of tick T, written once per call by launch_audit_truth: bit x of `alive`
// (byte x / 8) is set iff x is alive at T, the bits from n up to the last byte are 0; fp[x] =
// audit_fp(x) (NULL: not written, the partial view computes it per entry).
struct AuditTruthArgs {
    int32_t n, tick;
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    uint8_t *alive;                  // [(n + 7) / 8]
    uint64_t *fp;                    // [n] or NULL
};

// Full view: one shard's table of tick T, rows [row0, row0 + rows) x columns [col0, col0 + stride)
struct AuditScaleArgs {
    const uint16_t *table;           // [rows][stride], hb << 5 | ts mod 32, 0 = absent
    int64_t stride;                  // a multiple of kAuditStrip
    int32_t n, col0, row0, rows, tick, age_limit;
    const int32_t *fail_tick, *start_tick;   // as above
    const uint8_t *alive;            // the truth of this call
    const uint64_t *fp;
    uint32_t *arr;                   // [kAuditFields][n]
    unsigned long long *print;       // [n]
};

// Partial view: one shard's views of tick T, rows [row0, row0 + rows)
struct AuditPviewArgs {
    const uint64_t *table;           // [rows][view], id << 32 | hb << 5 | ts mod 32, sorted by id
    const int32_t *len;              // [rows]: valid slots of each row (the rest are ~0)
    int32_t n, view, row0, rows, tick, age_limit;
    const int32_t *fail_tick, *start_tick;
    const uint8_t *alive;
    uint32_t *arr;
    unsigned long long *print;
};

hipError_t launch_audit_truth(const AuditTruthArgs &a, hipStream_t st);
hipError_t launch_audit_scale(const AuditScaleArgs &a, hipStream_t st);
hipError_t launch_audit_pview(const AuditPviewArgs &a, hipStream_t st);

}  // namespace gsp
