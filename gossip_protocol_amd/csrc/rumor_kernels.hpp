// gossip_protocol_amd/csrc/rumor_kernels.hpp -- the rumor trace of both scale engines: which of
// up to 32 rumors every node has heard, moved one hop per tick over the messages the tick
// kernels really merge (gossip.h "Rumor trace").
//
// State, shared by every local shard: know[2][n] (one 32-bit mask per node, ping-pong by tick
// parity: tick t reads know[(t + 1) & 1] and writes know[t & 1]), heard[rumors][n] (the tick a
// bit was first set, -1 before) and known[rumors][max_ticks + 1] (nodes whose heard equals t).
//
// One tick is one launch per local shard over the shard's receiver CSR of that tick, placed
// after the CSR (and, partial view, the receipt records) is complete and before the tick kernels,
// which may sort csr_src in place (the same set).  The launch only reads know_prev and only
// writes know_cur, every row of the shard exactly once and by one lane, so the kernel boundary
// is the only synchronisation: no LDS, no spin, nothing a workgroup needs from another one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsp {

constexpr int kRumorMax = 32;        // rumors of a trace: the bits of a know word
constexpr int kRumorLaneSeg = 64;    // a longer segment is walked by the whole wave

struct RumorTickArgs {
    int32_t n, tick;
    int32_t row0, rows;              // the shard's receivers; off / rc_* are indexed from row0
    const int32_t *off;              // [rows + 1] receiver CSR of this tick
    const int32_t *csr_src;          // sender ids, kJoinRepSrc (-1) for a JOINREP: node 0's word
    const int32_t *rc_info;          // bounded partial view: [rows] k | k_all << 3, else NULL
    const int32_t *rc_src;           // ... [rows][8] the k smallest senders (a JOINREP first)
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    const uint32_t *know_prev;       // [n] know of tick - 1
    uint32_t *know_cur;              // [n] rows [row0, row0 + rows) are written
    int32_t *heard;                  // [rumors][n]
    uint32_t *known;                 // [rumors][known_stride]; [b][tick] is added to
    int32_t known_stride;
};

struct RumorSeedArgs {
    int32_t n, tick, rumor;
    int32_t lo, hi;                  // heard / known are recorded for ids in [lo, hi) (the rows a
                                     // rank holds); the bit is set in know for every alive source
    const int32_t *sources;          // ids in [0, n): checked by the host
    int32_t n_sources;
    const int32_t *fail_tick, *start_tick;
    uint32_t *know;                  // [n] know of `tick`
    int32_t *heard;                  // [n] of this rumor
    uint32_t *known;                 // this rumor's word of `tick`
};

hipError_t launch_rumor_seed(const RumorSeedArgs &a, hipStream_t st);
hipError_t launch_rumor_tick(const RumorTickArgs &a, hipStream_t st);

}  // namespace gsp
