// gossip_protocol_amd/csrc/reach_kernels.hpp -- overlay reach of both scale engines: a
// level-synchronous BFS over the "r lists x" graph of the engine's current tick T, in HBM.
// Vertices are the nodes alive at T (start[r] <= T <= crash[r], policy.hpp); r -> x is an edge
// iff both are alive, r's list in table[T & 1] holds x and (T - ts) mod 32 < age_limit.  Rows
// that are not alive are never read (their buffers are stale), and no tick kernel is involved.
//
// One level is one launch per shard and the kernel boundary is the only synchronisation: no
// workgroup waits for, or needs a value from, another one of the same launch.  The shared state
// is hops[n] (kReachUnset where not reached), so shards, tiles and ranks combine with MIN.
// Every write of the launch of level `cur` is atomicMin(hops[x], cur + 1), i.e. the same value
// from every writer, and every read that decides anything is "was x in the frontier / unreached
// as of the last launch" -- taken from hops words nobody rewrites to a value that matters (a
// frontier word is final; an unreached word can only turn into cur + 1) or from the two bitmaps
// reach_level wrote before the launch.  A stale read therefore costs a redundant atomic, never a
// different result.
//
// A level costs about the frontier, not the table: a row outside the frontier (FROM) or already
// reached (TO) is rejected from its 4-byte hops word before any entry is loaded, and a full-view
// 512-column strip with no unreached alive column loads no row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsp {

constexpr uint32_t kReachUnset = 0xFFFFFFFFu;
constexpr int kReachStrip = 512;     // full view: columns of a work item (one wave at 16 B per lane)
constexpr int kReachRows = 256;      // full view FROM: rows of a work item, interleaved over 4 waves
constexpr int kReachChunk = 2048;    // nodes per workgroup of reach_level; the bitmaps cover n
                                     // rounded up to it, so every strip byte read exists

inline size_t reach_bitmap_words(int32_t n) {      // 64-bit words of one bitmap
    return (size_t(n) + kReachChunk - 1) / kReachChunk * (kReachChunk / 64);
}

// What every form shares.  front / todo are as reach_level left them for level `cur`.
struct ReachCommon {
    int32_t n, tick, age_limit;
    uint32_t cur;                    // the frontier's level; the launch writes cur + 1
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    uint32_t *hops;                  // [n]
    const uint64_t *front;           // bit x: hops[x] == cur
    const uint64_t *todo;            // bit x: x alive and hops[x] unset
};

// Full view: one shard's table of tick T, rows [row0, row0 + rows) x columns [col0, col0 + stride)
struct ReachScaleArgs {
    ReachCommon c;
    const uint16_t *table;           // [rows][stride], hb << 5 | ts mod 32, 0 = absent
    int64_t stride;                  // a multiple of kReachStrip, and so is col0
    int32_t col0, row0, rows;
};

// Partial view: one shard's views of tick T, rows [row0, row0 + rows)
struct ReachPviewArgs {
    ReachCommon c;
    const uint64_t *table;           // [rows][view], id << 32 | hb << 5 | ts mod 32, sorted by id
    const int32_t *len;              // [rows]: valid slots of each row (the rest are ~0)
    int32_t view, row0, rows;
};

// hops[id] = 0 for every alive source (ids already range-checked); hops was set to kReachUnset
hipError_t launch_reach_seed(const int32_t *sources, int32_t n_sources, const ReachCommon &c,
                             hipStream_t st);
// *count += nodes with hops == level; front <- hops == level, todo <- alive and unset
// (both bitmaps are written whole, reach_bitmap_words(n) words each)
hipError_t launch_reach_level(const ReachCommon &c, uint32_t level, uint64_t *front, uint64_t *todo,
                              uint32_t *count, hipStream_t st);
// one BFS level; to = false: GSP_REACH_FROM (push from the frontier rows), true: GSP_REACH_TO
// (every unreached alive row pulls from the frontier bits)
hipError_t launch_reach_scale(const ReachScaleArgs &a, bool to, hipStream_t st);
hipError_t launch_reach_pview(const ReachPviewArgs &a, bool to, hipStream_t st);

}  // namespace gsp
