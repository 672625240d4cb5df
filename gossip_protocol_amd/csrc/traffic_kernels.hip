// gossip_protocol_amd/csrc/traffic_kernels.hip -- the traffic ledger's passes (traffic_kernels.hpp).
#include "traffic_kernels.hpp"
#include "wave_ops.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ bool traffic_alive(const int32_t *start_tick, const int32_t *fail_tick,
                                              int32_t r, int32_t t) {
    return (start_tick ? start_tick[r] : 0) <= t && t <= fail_tick[r];
}

// the node a message from `s` is charged to: a JOINREP (kJoinRepSrc = -1) is node 0's; any id
// outside [0, n) reads node 0 too, so no sender id becomes an address unchecked
__device__ __forceinline__ int32_t traffic_node(int32_t n, int32_t s) {
    return uint32_t(s) < uint32_t(n) ? s : 0;
}

// 1 + the payload entries of one merged message
__device__ __forceinline__ uint64_t traffic_entries(const TrafficRecvArgs &a, int32_t s, int32_t jsize) {
    return 1ull + uint64_t(s < 0 ? jsize : a.psize[traffic_node(a.n, s)]);
}

// the alternative form's sender side: one message of tick - 1 charged to its sender
__device__ __forceinline__ void traffic_charge(const TrafficRecvArgs &a, int32_t s) {
    const int32_t x = traffic_node(a.n, s);
    atomicAdd(&a.arr[int64_t(kTrSent) * a.n + x], 1u);
    const int32_t w = a.watch_slot[x];
    if (w >= 0) atomicAdd(&a.watch[(int64_t(w) * a.span + (a.tick - 1)) * 2], 1u);
}

__device__ __forceinline__ int traffic_bucket(uint32_t k) {
    const int b = k ? 32 - __builtin_clz(k) : 0;
    return b < kTrBuckets ? b : kTrBuckets - 1;
}

// A wave takes 64 consecutive local rows at a time, one lane per receiver; a workgroup strides
// over the rows (every lane makes the same number of trips: the ballots and the DPP reductions
// need the whole wave) and keeps the tick's totals in registers, so that it adds each field to
// global memory once: with one atomic per wave the 16,384 waves of 2^20 rows queued on the same
// few addresses for longer than the rows took to count.
__global__ void __launch_bounds__(256) traffic_recv_kernel(TrafficRecvArgs a) {
    __shared__ uint32_t s_hist[kTrBuckets];
    __shared__ unsigned long long s_red[4][kTrSums + 1];
    const int tid = int(threadIdx.x), lane = tid & 63;
    if (tid < kTrBuckets) s_hist[tid] = 0u;
    __syncthreads();
    const TrafficLayout L{size_t(a.n), size_t(a.span)};
    const int32_t jsize = a.intro_list < a.psize[0] ? a.intro_list : a.psize[0];
    const bool charge = a.form == kTrafficFromCsr;
    uint64_t t_recv = 0ull, t_merged = 0ull, t_lost = 0ull, t_entries = 0ull;
    uint32_t t_max = 0u;
    for (int64_t base = int64_t(blockIdx.x) * 256; base < a.rows; base += int64_t(gridDim.x) * 256) {
        const int32_t lr = int32_t(base) + tid;
        const bool valid = lr < a.rows;
        const int32_t r = a.row0 + lr;
        int32_t o0 = 0, k = 0;
        bool alive = false;
        if (valid) {
            o0 = a.off[lr];
            k = a.off[lr + 1] - o0;
            alive = traffic_alive(a.start_tick, a.fail_tick, r, a.tick);
        }
        uint32_t merged = 0u;
        uint64_t entries = 0ull;
        bool wide = false;
        if (alive && a.rc_info) {                      // the K smallest senders, as the tick kernel
            merged = uint32_t(a.rc_info[lr] & 7);
            const int32_t *src = a.rc_src + int64_t(lr) * 8;
            for (uint32_t j = 0; j < merged; ++j) entries += traffic_entries(a, src[j], jsize);
        }
        if (valid && k > 0 && ((alive && !a.rc_info) || charge)) {
            if (k <= kTrLaneSeg) {
                for (int32_t j = 0; j < k; ++j) {
                    const int32_t s = a.csr_src[o0 + j];
                    if (alive && !a.rc_info) entries += traffic_entries(a, s, jsize);
                    if (charge) traffic_charge(a, s);
                }
            } else {
                wide = true;
            }
            if (alive && !a.rc_info) merged = uint32_t(k);
        }
        // the wave's long segments (a join burst on node 0, a drain-all hub), one after the
        // other: the whole wave strides over the segment and sums across its lanes
        for (uint64_t m = __ballot(wide); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const int32_t wo = int32_t(lane_of(uint32_t(o0), l)), wk = int32_t(lane_of(uint32_t(k), l));
            const bool sum = lane_of(uint32_t(alive && !a.rc_info), l) != 0u;
            uint64_t acc = 0ull;
            for (int32_t j = lane; j < wk; j += 64) {
                const int32_t s = a.csr_src[wo + j];
                if (sum) acc += traffic_entries(a, s, jsize);
                if (charge) traffic_charge(a, s);
            }
            acc = wave_sum64(acc);
            if (lane == l && sum) entries = acc;
        }
        const uint32_t recv = alive ? uint32_t(k) : 0u, lost = (valid && !alive) ? uint32_t(k) : 0u;
        if (valid) {
            if (recv) {
                a.arr[int64_t(kTrRecv) * a.n + r] += recv;
                unsigned long long *peak = a.wide + L.peak() + r;
                const unsigned long long now = (uint64_t(recv) << 32) | uint32_t(~uint32_t(a.tick));
                if (now > *peak) *peak = now;
            }
            if (merged) {
                a.arr[int64_t(kTrMerged) * a.n + r] += merged;
                a.wide[L.entries() + r] += entries;
            }
            if (lost) a.arr[int64_t(kTrLost) * a.n + r] += lost;
            const int32_t w = a.watch_slot[r];
            if (w >= 0) a.watch[(int64_t(w) * a.span + a.tick) * 2 + 1] = recv;
            if (alive) atomicAdd(&s_hist[traffic_bucket(recv)], 1u);
        }
        t_recv += recv;
        t_merged += merged;
        t_lost += lost;
        t_entries += entries;
        t_max = recv > t_max ? recv : t_max;
    }
    // the tick's totals: wave reductions, then one atomic per workgroup and field that is not zero
    t_recv = wave_sum64(t_recv);
    t_merged = wave_sum64(t_merged);
    t_lost = wave_sum64(t_lost);
    t_entries = wave_sum64(t_entries);
    t_max = wave_max32(t_max);
    if (lane == 0) {
        unsigned long long *w = s_red[tid >> 6];
        w[kTrSumSent] = t_recv + t_lost;               // the from-CSR form: the sends of tick - 1
        w[kTrSumRecv] = t_recv;
        w[kTrSumMerged] = t_merged;
        w[kTrSumLost] = t_lost;
        w[kTrSumEntries] = t_entries;
        w[kTrSums] = t_max;
    }
    __syncthreads();
    if (tid <= kTrSums) {
        unsigned long long v = 0ull;
        for (int wv = 0; wv < 4; ++wv) v = tid == kTrSums ? (s_red[wv][tid] > v ? s_red[wv][tid] : v) : v + s_red[wv][tid];
        unsigned long long *sums = a.wide + L.sums() + size_t(a.tick) * kTrSums;
        if (tid == kTrSums) {
            if (v) atomicMax(a.wide + L.tmax() + a.tick, v);
        } else if (tid == kTrSumSent) {
            if (charge && v) atomicAdd(sums - kTrSums + kTrSumSent, v);
        } else if (v) {
            atomicAdd(sums + tid, v);
        }
    }
    if (tid < kTrBuckets && s_hist[tid])
        atomicAdd(a.wide + L.fanin() + size_t(a.tick) * kTrBuckets + tid, (unsigned long long)s_hist[tid]);
}

// One lane per sender over the tick's send slots, a workgroup striding over the rows; the tick's
// total is added once per workgroup.
__global__ void __launch_bounds__(256) traffic_send_kernel(TrafficSendArgs a) {
    __shared__ unsigned long long s_red[4];
    const int tid = int(threadIdx.x);
    const TrafficLayout L{size_t(a.n), size_t(a.span)};
    uint64_t t_sent = 0ull;
    for (int64_t base = int64_t(blockIdx.x) * 256; base < a.rows; base += int64_t(gridDim.x) * 256) {
        const int32_t lr = int32_t(base) + tid;
        if (lr >= a.rows) continue;
        uint32_t c = 0u;
        const int32_t *od = a.out_dst + int64_t(lr) * a.fanout;
        for (int32_t q = 0; q < a.fanout; ++q) c += od[q] >= 0 ? 1u : 0u;
        const int32_t x = a.row0 + lr;
        if (c) a.arr[int64_t(kTrSent) * a.n + x] += c;
        const int32_t w = a.watch_slot[x];
        if (w >= 0) a.watch[(int64_t(w) * a.span + a.tick) * 2] = c;
        t_sent += c;
    }
    t_sent = wave_sum64(t_sent);                       // every lane is back here
    if ((tid & 63) == 0) s_red[tid >> 6] = t_sent;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long v = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        if (v) atomicAdd(a.wide + L.sums() + size_t(a.tick) * kTrSums + kTrSumSent, v);
    }
}

// One workgroup: the delivered JOINREPs of the tick, added to node 0 behind the sender pass.
__global__ void __launch_bounds__(256) traffic_join_kernel(TrafficJoinArgs a) {
    __shared__ uint32_t s_part[4];
    const int tid = int(threadIdx.x);
    uint32_t c = 0u;
    for (int32_t i = tid; i < a.count; i += 256) c += a.ok[i] ? 1u : 0u;
    c = wave_sum32(c);
    if ((tid & 63) == 0) s_part[tid >> 6] = c;
    __syncthreads();
    if (tid != 0) return;
    const uint32_t total = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    if (!total) return;
    const TrafficLayout L{size_t(a.n), size_t(a.span)};
    atomicAdd(&a.arr[int64_t(kTrSent) * a.n], total);
    atomicAdd(a.wide + L.sums() + size_t(a.tick) * kTrSums + kTrSumSent, (unsigned long long)total);
    const int32_t w = a.watch_slot[0];
    if (w >= 0) atomicAdd(&a.watch[(int64_t(w) * a.span + a.tick) * 2], total);
}

// A wave per view row: lane l takes slots l, l + 64, ...; the ballots count the row.
__global__ void __launch_bounds__(256) traffic_size_kernel(TrafficSizeArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int32_t lr = int32_t(blockIdx.x) * 4 + (int32_t(threadIdx.x) >> 6);
    if (lr >= a.rows) return;                          // wave-uniform
    const int32_t len = a.len[lr] < a.view ? a.len[lr] : a.view;
    const uint32_t t5 = uint32_t(a.tick) & 31u, tf = uint32_t(a.tfail);
    const uint64_t *row = a.table + int64_t(lr) * a.view;
    int32_t cnt = 0;
    for (int32_t i0 = 0; i0 < len; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint64_t v = i < len ? row[i] : ~0ull;
        cnt += __builtin_popcountll(__ballot(v != ~0ull && ((t5 - uint32_t(v)) & 31u) < tf));
    }
    if (lane == 0) a.psize[a.row0 + lr] = cnt;
}

// workgroups of the two row passes: one per 256 rows up to four per compute unit of a 256-CU part,
// each then striding over its share
unsigned traffic_grid(int32_t rows) {
    const int64_t blocks = (int64_t(rows) + 255) / 256;
    return unsigned(blocks < 1024 ? blocks : 1024);
}

bool traffic_common_ok(int32_t n, int32_t tick, int32_t span, const uint32_t *arr,
                       const unsigned long long *wide, const int32_t *watch_slot, const uint32_t *watch) {
    return n > 0 && n <= (1 << 21) && tick >= 1 && tick < span && arr && wide && watch_slot && watch;
}

}  // namespace

hipError_t launch_traffic_recv(const TrafficRecvArgs &a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    if (!traffic_common_ok(a.n, a.tick, a.span, a.arr, a.wide, a.watch_slot, a.watch) || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.n || !a.off || !a.csr_src || !a.fail_tick || !a.psize ||
        (a.rc_info && !a.rc_src))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(traffic_recv_kernel, dim3(traffic_grid(a.rows)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_traffic_send(const TrafficSendArgs &a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    if (!traffic_common_ok(a.n, a.tick, a.span, a.arr, a.wide, a.watch_slot, a.watch) || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.n || a.fanout < 1 || !a.out_dst)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(traffic_send_kernel, dim3(traffic_grid(a.rows)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_traffic_join(const TrafficJoinArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    if (!traffic_common_ok(a.n, a.tick, a.span, a.arr, a.wide, a.watch_slot, a.watch) || !a.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(traffic_join_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_traffic_sizes(const TrafficSizeArgs &a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    if (a.row0 < 0 || a.view < 1 || a.tfail < 1 || !a.table || !a.len || !a.psize) return hipErrorInvalidValue;
    hipLaunchKernelGGL(traffic_size_kernel, dim3(unsigned((a.rows + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
