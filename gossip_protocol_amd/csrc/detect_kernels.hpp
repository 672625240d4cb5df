// gossip_protocol_amd/csrc/detect_kernels.hpp -- the detection ledger of both scale engines: the
// event ring's records of a tick folded into per-member arrays on the device (gossip.h "Detection
// ledger").
//
// State, shared by every local shard: arr[kDetFields][n] (32-bit words), by_tick[span][4] and
// tot[kDetTotals] (64-bit).  first_* hold ~0 for none and take an unsigned MIN; last_remove holds
// t + 1 (0: none) and takes an unsigned MAX; the rest are sums -- so shards, workgroups and ranks
// combine with one operator per field and the host converts at readback.
//
// One fold is one launch per local shard over a fixed grid of (stripe, slice) workgroups, placed
// after every writer of the tick on the engine's stream.  A workgroup reads its stripe's counter
// on the device and takes min(counter, cap) records, the slices interleaved in runs of 256: 8-byte
// loads, coalesced along the stripe.  It writes nothing the tick kernels or another fold workgroup
// reads; the counters are zeroed by a memset behind the launch, so no workgroup zeroes a counter
// another one may still read.
//
// Two forms of the per-member update (the A/B is in DESIGN.md 4h):
//   kDetectPlain       one global atomic per record and field
//   kDetectAggregated  a per-workgroup open-addressed table in LDS keyed by x accumulates min /
//                      max / counts with LDS atomics and is flushed with one global atomic per
//                      distinct x and field; a record whose probe finds no slot takes the plain
//                      path
// The per-tick totals are summed per thread, then per workgroup in LDS, then one global atomic
// per workgroup and class for the tick of the stripe's first record (after the first fold every
// record of a fold carries one t); records of another tick add directly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "event_ring.hpp"

namespace gsp {

constexpr int kDetSlices = 4;            // workgroups per stripe
constexpr int kDetTable = 1024;          // LDS table slots per workgroup (aggregated form)
constexpr int kDetProbes = 8;            // linear probes before a record takes the plain path

enum DetField { kDetFirst = 0, kDetLast, kDetRemovers, kDetFalse, kDetFirstFalse, kDetRevivals,
                kDetEvicts, kDetFields };
enum DetTotal { kDetRecords = 0, kDetLost, kDetTrue, kDetFalseTot, kDetJoins, kDetRevived,
                kDetEvicted, kDetTotals };
enum DetForm { kDetectPlain = 0, kDetectAggregated = 1 };

struct DetectFoldArgs {
    EvRingArgs ev;                       // the shard's ring
    int32_t n;
    int32_t span;                        // by_tick rows: max_ticks + 1
    const int32_t *crash;                // [n] the failure schedule of every member
    uint32_t *arr;                       // [kDetFields][n]
    unsigned long long *by_tick;         // [span][4]
    unsigned long long *tot;             // [kDetTotals]
};

hipError_t launch_detect_fold(const DetectFoldArgs &a, int form, hipStream_t st);

}  // namespace gsp
