// gossip_protocol_amd/csrc/rumor_kernels.hip -- the rumor-trace kernels (rumor_kernels.hpp).
#include "rumor_kernels.hpp"
#include "wave_ops.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ bool rumor_alive(const int32_t *start_tick, const int32_t *fail_tick,
                                            int32_t r, int32_t t) {
    return (start_tick ? start_tick[r] : 0) <= t && t <= fail_tick[r];
}

// the word a message from `s` carries: a JOINREP (kJoinRepSrc = -1) is node 0's; any id outside
// [0, n) reads node 0's word too, so no sender id becomes an address unchecked
__device__ __forceinline__ uint32_t rumor_word(const RumorTickArgs &a, int32_t s) {
    return a.know_prev[uint32_t(s) < uint32_t(a.n) ? s : 0];
}

// One lane per source.  The atomicOr picks one winner among duplicates: it alone records the
// tick and counts the node.
__global__ void __launch_bounds__(256) rumor_seed_kernel(RumorSeedArgs a) {
    const int32_t i = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    if (i >= a.n_sources) return;
    const int32_t id = a.sources[i];
    if (!rumor_alive(a.start_tick, a.fail_tick, id, a.tick)) return;
    const uint32_t bit = 1u << a.rumor;
    const uint32_t old = atomicOr(&a.know[id], bit);
    if (!(old & bit) && id >= a.lo && id < a.hi) {
        a.heard[id] = a.tick;
        atomicAdd(a.known, 1u);
    }
}

// A wave takes 64 consecutive local rows, one lane per receiver.  Every lane stays in the kernel
// to its end (the ballots and the DPP reductions need the whole wave).
__global__ void __launch_bounds__(256) rumor_tick_kernel(RumorTickArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int32_t lr = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    const bool valid = lr < a.rows;
    const int32_t r = a.row0 + lr;
    int32_t o0 = 0, k = 0;
    uint32_t mine = 0u;
    bool hears = false;
    if (valid) {
        o0 = a.off[lr];
        k = a.off[lr + 1] - o0;
        mine = a.know_prev[r];
        hears = rumor_alive(a.start_tick, a.fail_tick, r, a.tick);
    }
    uint32_t got = 0u;
    bool wide = false;
    if (hears) {
        if (a.rc_info) {                              // the K smallest senders, as the tick kernel
            const int32_t kk = a.rc_info[lr] & 7;
            const int32_t *src = a.rc_src + int64_t(lr) * 8;
            for (int32_t j = 0; j < kk; ++j) got |= rumor_word(a, src[j]);
        } else if (k <= kRumorLaneSeg) {
            for (int32_t j = 0; j < k; ++j) got |= rumor_word(a, a.csr_src[o0 + j]);
        } else {
            wide = true;
        }
    }
    // the wave's long segments (a join burst on node 0, a drain-all hub), one after the other:
    // the whole wave strides over the segment and ORs across its lanes
    for (uint64_t m = __ballot(wide); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const int32_t wo = int32_t(lane_of(uint32_t(o0), l)), wk = int32_t(lane_of(uint32_t(k), l));
        uint32_t acc = 0u;
        for (int32_t j = lane; j < wk; j += 64) acc |= rumor_word(a, a.csr_src[wo + j]);
        acc = wave_or32(acc);
        if (lane == l) got = acc;
    }
    const uint32_t fresh = got & ~mine;               // 0 for a row that is not alive
    if (valid) {
        a.know_cur[r] = mine | fresh;
        for (uint32_t b = fresh; b; b &= b - 1) a.heard[int64_t(__builtin_ctz(b)) * a.n + r] = a.tick;
    }
    // per bit some row of the wave gained: one add of the rows that gained it
    for (uint32_t any = wave_or32(fresh); any; any &= any - 1) {
        const int b = __builtin_ctz(any);
        const uint64_t rows = __ballot((fresh >> b) & 1u);
        if (lane == 0)
            atomicAdd(&a.known[int64_t(b) * a.known_stride + a.tick], uint32_t(__builtin_popcountll(rows)));
    }
}

}  // namespace

hipError_t launch_rumor_seed(const RumorSeedArgs &a, hipStream_t st) {
    if (a.n_sources <= 0) return hipSuccess;
    if (a.rumor < 0 || a.rumor >= kRumorMax || a.lo < 0 || a.hi > a.n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rumor_seed_kernel, dim3(unsigned((a.n_sources + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_rumor_tick(const RumorTickArgs &a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    if (a.row0 < 0 || int64_t(a.row0) + a.rows > a.n || a.tick < 0 || a.tick >= a.known_stride)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rumor_tick_kernel, dim3(unsigned((a.rows + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
