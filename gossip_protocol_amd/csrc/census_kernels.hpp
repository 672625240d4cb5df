// gossip_protocol_amd/csrc/census_kernels.hpp -- the membership census of both scale engines:
// for every member x, how many alive rows list x (listed), how many of those entries are
// younger than age_limit ticks (fresh) and the largest heartbeat they store (max_hb), from
// the tables of the engine's current tick T.  One streaming pass per call; no tick kernel is
// involved.  A row r counts iff start[r] <= T <= crash[r] (policy.hpp): a crashed row's buffer
// is stale and a row that has not started is empty.
//
// Every kernel accumulates into n-length arrays the host zeroed, with integer atomics only, so
// the result is exact and does not depend on the order the shards, tiles or workgroups run in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsp {

constexpr int kCensusStrip = 512;    // full view: columns of a work item (one wave at 16 B per lane)
constexpr int kCensusRows = 256;     // full view: rows of a work item, interleaved over 4 waves;
                                     // a wave's packed 16-bit counters see at most 64 rows
constexpr int kCensusCut = 4096;     // partial view, privatised form: ids below it count in LDS
constexpr bool kCensusPviewLds = false;   // partial view: the form gsp_pview_census runs

// Full view: one shard's table of tick T, rows [row0, row0 + rows) x columns [col0, col0 + stride)
struct CensusScaleArgs {
    const uint16_t *table;           // [rows][stride], hb << 5 | ts mod 32, 0 = absent
    int64_t stride;                  // a multiple of kCensusStrip
    int32_t n, col0, row0, rows, tick, age_limit;
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    uint32_t *listed, *fresh, *max_hb;   // [n]
};

// Partial view: one shard's views of tick T, rows [row0, row0 + rows)
struct CensusPviewArgs {
    const uint64_t *table;           // [rows][view], id << 32 | hb << 5 | ts mod 32, sorted by id
    const int32_t *len;              // [rows]: valid slots of each row (the rest are ~0)
    int32_t n, view, row0, rows, tick, age_limit;
    const int32_t *fail_tick, *start_tick;   // as above
    unsigned long long *counts;      // [n]: fresh << 32 | listed, one 64-bit add per entry
    uint32_t *max_hb;                // [n]
};

hipError_t launch_census_scale(const CensusScaleArgs &a, hipStream_t st);
// lds = false: global atomics per entry; true: a persistent grid of `cus` x 2 workgroups counts
// the ids below kCensusCut in LDS and flushes them once per workgroup (slower at 1,048,576 x 256
// in both the early and the hub-heavy ticks, DESIGN.md 4e: kept for A/B and tested)
hipError_t launch_census_pview(const CensusPviewArgs &a, bool lds, int32_t cus, hipStream_t st);

}  // namespace gsp
