// gossip_protocol_amd/csrc/traffic_kernels.hpp -- the traffic ledger of both scale engines: per
// node, the messages it put on the network, the messages addressed to it while alive (before and
// after the inbox cut) and while not alive, the member entries it had to merge and its largest
// fan-in of one tick (gossip.h "Traffic ledger").
//
// State, shared by every local shard:
//   arr[kTrFields][n]  u32  sent, recv, merged, lost
//   wide               u64  entries[n] | sums[span][kTrSums] | fanin[span][kTrBuckets]   (added to)
//                           | peak[n] | tmax[span]                                       (max'ed)
//   watch[w][span][2]  u32  (sent, recv) of the watched nodes per tick; watch_slot[n] maps a node to
//                           its w (-1: not watched)
// peak[r] = largest recv of one tick << 32 | ~tick: a later tick with the same count is the smaller
// word, so a plain compare keeps the first tick, and MAX across ranks reduces the pair as one.
//
// One tick is two launches per CSR.  The receiver pass runs where the receiver CSR of t is
// complete and before the tick kernels (which may sort csr_src in place): one lane per receiver,
// a segment past kTrLaneSeg walked by the whole wave.  The sender pass runs once the tick's send
// slots are final: one lane per sender.  Every row of arr / entries / peak / watch is written by
// exactly one lane, so the kernel boundary is the only synchronisation; a workgroup strides over
// its rows, reduces the per-tick sums and the maximum over its waves and adds each with one atomic
// per workgroup and field, and the fan-in histogram is privatised in LDS and flushed with at most
// kTrBuckets atomics per workgroup (at most 1,024 workgroups).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsp {

enum : int { kTrSent = 0, kTrRecv, kTrMerged, kTrLost, kTrFields };
enum : int { kTrSumSent = 0, kTrSumRecv, kTrSumMerged, kTrSumLost, kTrSumEntries, kTrSums };
constexpr int kTrBuckets = 18;       // fan-in classes: 0, then 2^(b-1) <= k < 2^b, the last open
constexpr int kTrLaneSeg = 64;       // a longer segment is walked by the whole wave
constexpr int kTrMaxWatch = 1024;

// Offsets into `wide` (u64 words) for n nodes and span = max_ticks + 1 ticks.
struct TrafficLayout {
    size_t n, span;
    __host__ __device__ size_t entries() const { return 0; }
    __host__ __device__ size_t sums() const { return n; }
    __host__ __device__ size_t fanin() const { return n + span * kTrSums; }
    __host__ __device__ size_t added() const { return n + span * (kTrSums + kTrBuckets); }   // words that are summed
    __host__ __device__ size_t peak() const { return added(); }
    __host__ __device__ size_t tmax() const { return added() + n; }
    __host__ __device__ size_t total() const { return added() + n + span; }
};

struct TrafficRecvArgs {
    int32_t n, tick, span;
    int32_t row0, rows;              // the shard's receivers; off / rc_* are indexed from row0
    const int32_t *off;              // [rows + 1] receiver CSR of this tick
    const int32_t *csr_src;          // sender ids, kJoinRepSrc (-1) for a JOINREP
    const int32_t *rc_info;          // bounded partial view: [rows] k | k_all << 3, else NULL
    const int32_t *rc_src;           // ... [rows][8] the k smallest senders (a JOINREP first)
    const int32_t *fail_tick;        // [n]
    const int32_t *start_tick;       // [n], or NULL: every node starts at 0
    const int32_t *psize;            // [n] payload entries of a GOSSIP each node sent at tick - 1
    int32_t intro_list;              // a JOINREP carries min(intro_list, psize[0]) entries
    int32_t form;                    // kTrafficFromCsr: one atomic per message adds sent[sender]
    uint32_t *arr;                   // [kTrFields][n]
    unsigned long long *wide;        // TrafficLayout
    const int32_t *watch_slot;       // [n]
    uint32_t *watch;                 // [n_watch][span][2]
};

struct TrafficSendArgs {
    int32_t n, tick, span;
    int32_t row0, rows, fanout;
    const int32_t *out_dst;          // [rows][fanout] this tick's send slots, -1: none or dropped
    uint32_t *arr;
    unsigned long long *wide;
    const int32_t *watch_slot;
    uint32_t *watch;
};

// the delivered JOINREPs node 0 sent at `tick`: ok[count] of the join plan's joiners
struct TrafficJoinArgs {
    int32_t n, tick, span;
    const int32_t *ok;
    int32_t count;
    uint32_t *arr;
    unsigned long long *wide;
    const int32_t *watch_slot;
    uint32_t *watch;
};

// partial view with TFAIL: psize[row0 + lr] = the entries of view row lr not suspected at `tick`
struct TrafficSizeArgs {
    int32_t tick, tfail, view;
    int32_t row0, rows;
    const uint64_t *table;           // [rows][view] packed entries, ts mod 32 in the low 5 bits
    const int32_t *len;              // [rows]
    int32_t *psize;                  // [n]
};

enum : int { kTrafficFromSlots = 0, kTrafficFromCsr = 1 };

hipError_t launch_traffic_recv(const TrafficRecvArgs &a, hipStream_t st);
hipError_t launch_traffic_send(const TrafficSendArgs &a, hipStream_t st);
hipError_t launch_traffic_join(const TrafficJoinArgs &a, hipStream_t st);
hipError_t launch_traffic_sizes(const TrafficSizeArgs &a, hipStream_t st);

}  // namespace gsp
