// gossip_protocol_amd/csrc/reach_multi_kernels.hpp -- multi-source overlay reach of both scale
// engines: up to 64 independent single-source BFS trees over the graph of reach_kernels.hpp (same
// vertices, same edge rule, same tables) in one sweep per level.  A node's state is one 64-bit
// word, bit b belonging to sources[b] alone: one visit of an entry advances every tree whose
// frontier holds the row with one AND and one OR.
//
// Synchronisation is reach's: one level is one launch per local shard, and the kernel boundary
// is the only synchronisation.  There is no cooperative or persistent grid, no flag, no spin, and
// no value one workgroup needs from another within a launch.
//
// Three words per node, seen / front / next, and one writer per phase:
//   - a row-form launch (level `cur`) only READS seen, front and the two bitmaps, all of them as
//     the level kernel left them, and only WRITES next, and only by OR (an atomicOr, or the store
//     of the one wave that owns the word into the zero the level kernel left);
//   - the level kernel, alone between two row-form launches, is the only writer of seen, front,
//     the bitmaps, the counters and hops: new = next & ~seen; seen |= new; front = new; next = 0.
// OR is commutative, associative and idempotent, and nothing a row form reads changes while it
// runs, so next -- and with it every output -- is the same bit for bit whatever the dispatch
// order, the shard count or the layout.  A lost race cannot exist; only a redundant atomicOr can.
// The seed goes the same way: it ORs the alive sources' bits into next and the level kernel of
// level 0 admits them, so hops 0, the level-0 counts and the first bitmaps come from the one
// place every later level's do.
//
// The two bitmaps the level kernel rewrites whole are the row forms' rejection tests:
//   hot   bit x: front[x] != 0
//   open  bit x: x is alive and seen[x] still lacks the bit of an alive source
// A row outside the frontier (FROM) or with nothing left to gain (TO) is rejected before any
// entry is loaded; a target that is not alive has no open bit and never receives one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "reach_kernels.hpp"

namespace gsp {

constexpr int kReachMultiMax = 64;   // GSP_REACH_MAX_SOURCES: the bits of a node's word

// the nodes the per-node words and the bitmaps cover: n rounded up to kReachChunk
inline size_t reach_multi_nodes(int32_t n) { return reach_bitmap_words(n) * 64; }

// What every row form shares, as the level kernel left it for level `cur`.
struct ReachMultiCommon {
    int32_t n, tick, age_limit;
    uint64_t want;                   // the bits whose source is alive at T
    const uint64_t *seen;            // [reach_multi_nodes(n)] bit b: reached by tree b
    const uint64_t *front;           // bit b: at hop `cur` of tree b
    uint64_t *next;                  // what this launch ORs into; zero on entry
    const uint64_t *hot;             // bitmap: front[x] != 0
    const uint64_t *open;            // bitmap: x alive and (want & ~seen[x]) != 0
};

// the same shapes as ReachScaleArgs / ReachPviewArgs
struct ReachMultiScaleArgs {
    ReachMultiCommon c;
    const uint16_t *table;           // [rows][stride], hb << 5 | ts mod 32, 0 = absent
    int64_t stride;                  // a multiple of kReachStrip, and so is col0
    int32_t col0, row0, rows;
};

struct ReachMultiPviewArgs {
    ReachMultiCommon c;
    const uint64_t *table;           // [rows][view], id << 32 | hb << 5 | ts mod 32, sorted by id
    const int32_t *len;              // [rows]
    int32_t view, row0, rows;
};

struct ReachMultiLevelArgs {
    int32_t n, tick, n_sources;
    uint32_t level;
    uint64_t want;
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL
    uint64_t *seen, *front, *next;   // [reach_multi_nodes(n)]
    uint64_t *hot, *open;            // [reach_bitmap_words(n)], written whole
    uint32_t *count;                 // [kReachMultiMax] cumulative: nodes reached by tree b
    uint32_t *hops;                  // [n_sources][n], or NULL: hops[b][x] = level where new
};

// next[sources[b]] |= 1 << b for every source alive at T (ids already range-checked)
hipError_t launch_reach_multi_seed(const int32_t *sources, const ReachMultiLevelArgs &a, hipStream_t st);
// new = next & ~seen; seen |= new; front = new; next = 0; count[b] += nodes with bit b new
hipError_t launch_reach_multi_level(const ReachMultiLevelArgs &a, hipStream_t st);
// one BFS level; to = false: GSP_REACH_FROM (push), true: GSP_REACH_TO (pull)
hipError_t launch_reach_multi_scale(const ReachMultiScaleArgs &a, bool to, hipStream_t st);
hipError_t launch_reach_multi_pview(const ReachMultiPviewArgs &a, bool to, hipStream_t st);
// ranks: next[x] = OR over w < world of stage[w][x], x < nodes (stage: every rank's next, gathered)
hipError_t launch_reach_multi_fold(const uint64_t *stage, int32_t world, size_t nodes, uint64_t *next,
                                   hipStream_t st);

}  // namespace gsp
