// gossip_protocol_amd/csrc/detect_kernels.hip -- the detection ledger's fold (detect_kernels.hpp).
#include "detect_kernels.hpp"

namespace gsp {
namespace {

constexpr uint32_t kDetNone = 0xFFFFFFFFu;       // first_*: no record yet; an empty table slot
constexpr int kDetClasses = 4;                   // true remove, false remove, revival, evict
// the workgroup's sums: every record by class, the joins, and by class the records of `tref`
constexpr int kDetSums = 2 * kDetClasses + 1;

__device__ __forceinline__ bool det_is_min(int f) { return f == kDetFirst || f == kDetFirstFalse; }

// one field of member x in the global ledger
__device__ __forceinline__ void det_global(const DetectFoldArgs &a, int f, uint32_t x, uint32_t v) {
    uint32_t *p = a.arr + int64_t(f) * a.n + x;
    if (det_is_min(f)) atomicMin(p, v);
    else if (f == kDetLast) atomicMax(p, v);
    else atomicAdd(p, v);
}

// A workgroup is (stripe, slice): slice s takes the stripe's records [(j * kDetSlices + s) * 256,
// + 256) for j = 0, 1, ... below min(counter, cap).  Everything that decides a barrier is uniform
// over the workgroup (the stripe's counter).
template <bool kAgg>
__global__ void __launch_bounds__(256) detect_fold_kernel(DetectFoldArgs a) {
    __shared__ uint32_t s_sum[kDetSums];
    __shared__ uint32_t s_key[kAgg ? kDetTable : 1];
    __shared__ uint32_t s_val[kAgg ? kDetFields * kDetTable : 1];
    const int tid = int(threadIdx.x);
    const int stripe = int(blockIdx.x) / kDetSlices, slice = int(blockIdx.x) % kDetSlices;
    const unsigned long long made = a.ev.count[stripe * kEvCounterStride];
    const int64_t take = made < (unsigned long long)a.ev.cap ? int64_t(made) : a.ev.cap;
    if (slice == 0 && tid == 0 && made) {
        atomicAdd(&a.tot[kDetRecords], (unsigned long long)take);
        if (made > (unsigned long long)take) atomicAdd(&a.tot[kDetLost], made - (unsigned long long)take);
    }
    if (int64_t(slice) * 256 >= take) return;
    const unsigned long long *buf = a.ev.buf + int64_t(stripe) * a.ev.cap;
    const uint32_t tref = uint32_t(buf[0] >> 42) & 0xFFFFFu;      // take > 0 here

    if (tid < kDetSums) s_sum[tid] = 0u;
    if (kAgg) {
        for (int i = tid; i < kDetTable; i += 256) s_key[i] = kDetNone;
        for (int i = tid; i < kDetFields * kDetTable; i += 256)
            s_val[i] = det_is_min(i / kDetTable) ? kDetNone : 0u;
    }
    __syncthreads();

    uint32_t all[kDetClasses] = {0u, 0u, 0u, 0u}, ref[kDetClasses] = {0u, 0u, 0u, 0u}, joins = 0u;
    for (int64_t i = int64_t(slice) * 256 + tid; i < take; i += int64_t(kDetSlices) * 256) {
        const unsigned long long rec = buf[i];
        const uint32_t kind = uint32_t(rec >> 62), t = uint32_t(rec >> 42) & 0xFFFFFu;
        const uint32_t x = uint32_t(rec) & 0x1FFFFFu;
        if (x >= uint32_t(a.n)) continue;            // no id becomes an address unchecked
        const bool after = int64_t(t) > int64_t(a.crash[x]);
        int cls = -1;
        if (kind == 2u) cls = after ? 0 : 1;
        else if (kind == 1u) { ++joins; cls = after ? 2 : -1; }
        else if (kind == 3u) cls = 3;
        if (cls < 0) continue;
        ++all[cls];
        if (t == tref) ++ref[cls];
        else if (t < uint32_t(a.span)) atomicAdd(&a.by_tick[int64_t(t) * kDetClasses + cls], 1ull);
        int slot = -1;
        if (kAgg) {
            uint32_t h = (x * 2654435761u) >> 22;    // 10 bits: kDetTable slots
            for (int p = 0; p < kDetProbes; ++p) {
                const uint32_t old = atomicCAS(&s_key[h], kDetNone, x);
                if (old == kDetNone || old == x) { slot = int(h); break; }
                h = (h + 1u) & uint32_t(kDetTable - 1);
            }
        }
        if (slot >= 0) {
            uint32_t *v = s_val + slot;
            if (cls == 0) {
                atomicMin(v + kDetFirst * kDetTable, t);
                atomicMax(v + kDetLast * kDetTable, t + 1u);
                atomicAdd(v + kDetRemovers * kDetTable, 1u);
            } else if (cls == 1) {
                atomicAdd(v + kDetFalse * kDetTable, 1u);
                atomicMin(v + kDetFirstFalse * kDetTable, t);
            } else {
                atomicAdd(v + (cls == 2 ? kDetRevivals : kDetEvicts) * kDetTable, 1u);
            }
        } else if (cls == 0) {
            det_global(a, kDetFirst, x, t);
            det_global(a, kDetLast, x, t + 1u);
            det_global(a, kDetRemovers, x, 1u);
        } else if (cls == 1) {
            det_global(a, kDetFalse, x, 1u);
            det_global(a, kDetFirstFalse, x, t);
        } else {
            det_global(a, cls == 2 ? kDetRevivals : kDetEvicts, x, 1u);
        }
    }
    for (int c = 0; c < kDetClasses; ++c) {
        if (all[c]) atomicAdd(&s_sum[c], all[c]);
        if (ref[c]) atomicAdd(&s_sum[kDetClasses + 1 + c], ref[c]);
    }
    if (joins) atomicAdd(&s_sum[kDetClasses], joins);
    __syncthreads();

    if (tid < kDetSums && s_sum[tid]) {
        const unsigned long long v = s_sum[tid];
        if (tid < kDetClasses) atomicAdd(&a.tot[tid == 0 ? kDetTrue : tid == 1 ? kDetFalseTot
                                                : tid == 2 ? kDetRevived : kDetEvicted], v);
        else if (tid == kDetClasses) atomicAdd(&a.tot[kDetJoins], v);
        else if (tref < uint32_t(a.span))
            atomicAdd(&a.by_tick[int64_t(tref) * kDetClasses + (tid - kDetClasses - 1)], v);
    }
    if (kAgg) {
        for (int slot = tid; slot < kDetTable; slot += 256) {
            const uint32_t x = s_key[slot];
            if (x == kDetNone) continue;
            for (int f = 0; f < kDetFields; ++f) {
                const uint32_t v = s_val[f * kDetTable + slot];
                if (v != (det_is_min(f) ? kDetNone : 0u)) det_global(a, f, x, v);
            }
        }
    }
}

}  // namespace

hipError_t launch_detect_fold(const DetectFoldArgs &a, int form, hipStream_t st) {
    if (!a.ev.buf || !a.ev.count || a.ev.cap <= 0 || a.n <= 0 || a.n > (1 << 21) || a.span <= 0 ||
        !a.crash || !a.arr || !a.by_tick || !a.tot)
        return hipErrorInvalidValue;
    const dim3 grid(unsigned(kEvStripes * kDetSlices)), block(256);
    if (form == kDetectAggregated) hipLaunchKernelGGL(detect_fold_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(detect_fold_kernel<false>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
