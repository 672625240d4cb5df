// gossip_protocol_amd/csrc/components_kernels.hpp -- overlay components of both scale engines: the
// exact weakly and strongly connected components of the graph of reach_kernels.hpp (same
// vertices, same edge rule, same tables) at the engine's current tick T.  The result is
// label[x] = the smallest id of x's component, kCompNone for a node that is not alive.
//
// Both kinds are rounds of one table sweep per local shard and one n-length kernel, with the
// kernel boundary as the only synchronisation, and both only ever move a 32-bit word one way
// (atomicMin or atomicMax of node ids), so a stale read costs a later round, never a different
// fixed point, and shards, tiles and ranks combine with MIN / MAX.
//
// Weak: lab[] is a forest of parent pointers, lab[x] <= x, a root has lab[x] == x and is the
// smallest id of its tree, and a tree never leaves one component.
//   sweep  for an alive row r and the alive members x it lists: the smallest lab[x] of the row is
//          hooked below lab[r] (atomicMin(lab[lab[r]], that)), and per column the smallest lab[r]
//          of the wave's rows below lab[x].  An edge whose ends differ always moves one of them.
//   jump   every node follows its pointers to the root, stores it, and adds it to a checksum.
// The checksum only falls; the round that leaves it as it was hooked nothing, so every edge joins
// two nodes of one tree and the roots are the components' smallest ids.
//
// Strong: forward-backward colouring with trimming, on the nodes not yet assigned.  fcol[x] is
// the largest unassigned id that reaches x, bcol[x] the largest that x reaches, both inside x's
// part: an edge counts only between two unassigned nodes that ended the previous turn with the
// same (fcol, bcol) pair -- a strong component never straddles two parts, and the parts of a turn
// refine those of the turn before.
//   turn   (n-length) closes the previous turn and opens the next: a node with no counted
//          in-edge or no counted out-edge is a component of its own (trim), a node with
//          fcol == bcol == c is in the component of c (c reaches it and it reaches c); everyone
//          else keeps the pair as its part and starts over from fcol = bcol = own id.
//   sweep  fcol[x] = max(fcol[x], fcol[r]) and bcol[r] = max(bcol[r], bcol[x]) over the counted
//          edges r -> x; the first sweep of a turn also marks has_in[x] and has_out[r].
//   jump   fcol[x] = fcol[fcol[x]] up to the fixed point (c reaches x and c' reaches c), the same
//          for bcol, and both into the checksum, which only rises.
// A turn ends with the round that leaves the checksum as it was, and assigns at least the
// component of the largest unassigned id.  comp[] holds the largest id of each component; two
// last n-length kernels turn it into the smallest.
//
// Full view: a work item is reach's (512-column strip, 256 rows): a wave keeps its eight columns'
// words in registers, reads the strip of each of its active rows as one 1-KiB instruction, folds
// the row's word into the column registers and the columns' words into one word per row, and
// issues an atomic only where a word would move.  Partial view: a wave takes 64 rows and walks
// the active ones 64 slots at a time.  Rows and columns outside `active` (not alive, or already
// assigned) are never read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "reach_kernels.hpp"

namespace gsp {

constexpr uint32_t kCompNone = 0xFFFFFFFFu;      // lab / comp: not alive (weak), not assigned (strong)
enum { kCompWeak = 0, kCompStrong = 1 };         // GSP_COMPONENTS_WEAK / GSP_COMPONENTS_STRONG
// the cumulative 64-bit counters: the checksum after each round's jump, the nodes each turn left
// unassigned, and the checksum as the weak init or a turn set it (what an idle round repeats)
enum { kCompSum = 0, kCompLeft, kCompBase, kCompCounters };

// the nodes every array and the bitmap cover: n rounded up to kReachChunk, so every strip byte
// and word a full-view work item reads exists
inline size_t components_nodes(int32_t n) { return reach_bitmap_words(n) * 64; }

// What the kernels share.  Every array has components_nodes(n) words; weak uses lab alone.
struct CompCommon {
    int32_t n, tick, age_limit, kind;
    int32_t first;                   // strong: the first sweep of a turn (marks has_in / has_out)
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    uint64_t *active;                // bit x: x alive (weak); alive and not assigned (strong)
    uint32_t *lab;                   // weak: parent pointers
    uint32_t *fcol, *bcol;           // strong: this turn's colours
    uint32_t *pf, *pb;               // strong: the previous turn's pair, the part
    uint32_t *has_in, *has_out;      // strong: 1 where the first sweep saw a counted edge
    uint32_t *comp;                  // strong: the component's largest id, kCompNone until assigned
    unsigned long long *ctr;         // [kCompCounters], cumulative over the call
};

// the shapes of ReachScaleArgs / ReachPviewArgs
struct CompScaleArgs {
    CompCommon c;
    const uint16_t *table;           // [rows][stride], hb << 5 | ts mod 32, 0 = absent
    int64_t stride;                  // a multiple of kReachStrip, and so is col0
    int32_t col0, row0, rows;
};

struct CompPviewArgs {
    CompCommon c;
    const uint64_t *table;           // [rows][view], id << 32 | hb << 5 | ts mod 32, sorted by id
    const int32_t *len;              // [rows]
    int32_t view, row0, rows;
};

// weak: lab[x] = x for the alive, kCompNone for everyone else; active = alive; ctr[kCompBase] +=
// the checksum
hipError_t launch_components_weak_init(const CompCommon &c, hipStream_t st);
// strong: closes the previous turn (not when `opening`) and opens the next; ctr[kCompLeft] += the
// nodes still unassigned, ctr[kCompBase] += their checksum.  Before the opening turn comp is
// kCompNone everywhere.
hipError_t launch_components_turn(const CompCommon &c, bool opening, hipStream_t st);
// one shard's sweep of c.kind
hipError_t launch_components_scale(const CompScaleArgs &a, hipStream_t st);
hipError_t launch_components_pview(const CompPviewArgs &a, hipStream_t st);
// the n-length kernel of a round of c.kind; ctr[kCompSum] += the checksum
hipError_t launch_components_jump(const CompCommon &c, hipStream_t st);
// strong, after the last turn: comp (largest id) into lab (smallest id), through pf as scratch
hipError_t launch_components_canon(const CompCommon &c, hipStream_t st);

}  // namespace gsp
