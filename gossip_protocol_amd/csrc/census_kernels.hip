// gossip_protocol_amd/csrc/census_kernels.hip -- the census kernels (census_kernels.hpp).
#include "census_kernels.hpp"
#include "scale_row.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ bool census_alive(const int32_t *start_tick, const int32_t *fail_tick,
                                             int32_t r, int32_t t) {
    return (start_tick ? start_tick[r] : 0) <= t && t <= fail_tick[r];
}

// ---- full view: a column reduction over rows x stride packed u16 entries -------------------
// Work item = (512-column strip, block of 256 rows).  A wave reads the strip of one row as one
// 1-KiB instruction (16 B per lane, the tick kernels' vector shape) and takes every fourth row
// of the block; the alive test of a row is wave-uniform (one ballot over the wave's 64 rows),
// a dead row is never loaded, and the live rows are loaded four at a time -- the kernel is a
// pure stream with no dependent chain.  Per lane vector the counters are packed 16-bit (two
// columns per dword): a wave adds at most 64 rows, so they cannot overflow.  The four waves
// meet in LDS and the workgroup issues one integer atomic per column and array, as contiguous
// 256-B wave instructions.
//
// Atomic budget at n = 65,536 in 8 column tiles: 256 row blocks x 65,536 columns x 3 arrays x
// 4 B = 0.2 GB of atomics against 8.6 GB streamed.  The guides' chip-wide atomic rate (about
// 1.3 TB/s of added bytes) was measured for float adds of this shape; the integer rate is
// unmeasured.
struct CensusAcc {
    uint32_t listed[4], fresh[4], max_e[4];
};

// t5x2 / lim: T mod 32 / age_limit in both halves.  max_e keeps the largest entry, whose upper
// 11 bits are the largest heartbeat (the timestamp only breaks ties).
__device__ __forceinline__ void census_add(CensusAcc &c, const uint4 &v, uint32_t t5x2, uint32_t lim) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t pe = pk_min(w[i], 0x00010001u);             // present: e != 0
        const uint32_t age = pk_sub(t5x2, w[i]) & 0x001F001Fu;      // (T - ts) mod 32
        c.listed[i] += pe;
        c.fresh[i] += pk_min(pk_subc(lim, age), pe);                // age < age_limit
        c.max_e[i] = pk_max(c.max_e[i], w[i]);
    }
}

__global__ void __launch_bounds__(256) census_scale_kernel(CensusScaleArgs a) {
    // [wave][array][word][lane], the lane dimension padded: the column readers below take the
    // four words of one lane together
    __shared__ uint32_t s_acc[4][3][4][65];
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kCensusRows;
    const int64_t c0 = int64_t(blockIdx.x) * kCensusStrip;
    const uint32_t t5 = uint32_t(a.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.age_limit) | (uint32_t(a.age_limit) << 16);

    // lane j: is the wave's j-th row (rb + wave + 4 j) alive at T?
    const int32_t lr = rb + wave + 4 * lane;
    const bool alive = lr < a.rows && census_alive(a.start_tick, a.fail_tick, a.row0 + lr, a.tick);
    uint64_t live = __ballot(alive);

    CensusAcc c{};
    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    while (__builtin_popcountll(live) >= 4) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = __builtin_ctzll(live);
            live &= live - 1;
            v[q] = ld16<true>(base + j * step);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) census_add(c, v[q], t5x2, lim);
    }
    while (live) {
        const int j = __builtin_ctzll(live);
        live &= live - 1;
        census_add(c, ld16<true>(base + j * step), t5x2, lim);
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s_acc[wave][0][i][lane] = c.listed[i];
        s_acc[wave][1][i][lane] = c.fresh[i];
        s_acc[wave][2][i][lane] = c.max_e[i];
    }
    __syncthreads();
    // thread t: columns t and t + 256 of the strip; a wave's atomics cover 64 contiguous columns
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = int(threadIdx.x) + 256 * h;
        const int ln = col >> 3, word = (col >> 1) & 3, sh = (col & 1) * 16;
        uint32_t l = 0, f = 0, m = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            l += (s_acc[w][0][word][ln] >> sh) & 0xFFFFu;
            f += (s_acc[w][1][word][ln] >> sh) & 0xFFFFu;
            m = max(m, (s_acc[w][2][word][ln] >> sh) & 0xFFFFu);
        }
        const int64_t gc = int64_t(a.col0) + c0 + col;
        if (gc < a.n && l) {           // columns >= n are stride padding
            atomicAdd(&a.listed[gc], l);
            if (f) atomicAdd(&a.fresh[gc], f);
            atomicMax(&a.max_hb[gc], m >> 5);
        }
    }
}

// ---- partial view: a scatter over rows x view 64-bit entries --------------------------------
// One lane per slot (a view of 256 is one 2-KiB coalesced read per 256 lanes).  Only the slots
// below len of an alive row are read; an id >= n (the empty slot's ~0 among them) is dropped
// before it becomes an address.
__device__ __forceinline__ bool census_slot(const CensusPviewArgs &a, uint32_t i, uint32_t &id,
                                            uint32_t &hb, uint32_t &fresh) {
    const uint32_t lr = i / uint32_t(a.view), slot = i - lr * uint32_t(a.view);
    if (!census_alive(a.start_tick, a.fail_tick, a.row0 + int32_t(lr), a.tick)) return false;
    if (int32_t(slot) >= a.len[lr]) return false;
    const uint64_t e = a.table[i];
    id = uint32_t(e >> 32);
    hb = (uint32_t(e) & 0xFFFFu) >> 5;
    fresh = ((uint32_t(a.tick) - uint32_t(e)) & 31u) < uint32_t(a.age_limit) ? 1u : 0u;
    return id < uint32_t(a.n);
}

__device__ __forceinline__ void census_count(const CensusPviewArgs &a, uint32_t id, uint32_t hb,
                                             uint32_t fresh) {
    atomicAdd(&a.counts[id], (uint64_t(fresh) << 32) | 1ull);
    // max_hb only grows during a call, so a value read earlier is a lower bound of the current
    // one: an entry at or below it cannot raise the maximum and skips its atomic (most do: the
    // views' heartbeats for one id lie within a few ticks of each other)
    if (hb > __hip_atomic_load(&a.max_hb[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&a.max_hb[id], hb);
}

// plain form: two global atomics per entry
__global__ void __launch_bounds__(256) census_pview_kernel(CensusPviewArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;     // rows * view < 2^29
    if (i >= uint32_t(a.rows) * uint32_t(a.view)) return;
    uint32_t id, hb, fresh;
    if (census_slot(a, i, id, hb, fresh)) census_count(a, id, hb, fresh);
}

// privatised form: the default eviction order makes low ids hubs (a few ids sit in most views),
// so a persistent grid counts the ids below kCensusCut in LDS and flushes them once per
// workgroup; the other ids take the plain form's atomics
__global__ void __launch_bounds__(1024) census_pview_lds_kernel(CensusPviewArgs a) {
    __shared__ uint32_t s_listed[kCensusCut], s_fresh[kCensusCut], s_hb[kCensusCut];
    for (int i = int(threadIdx.x); i < kCensusCut; i += 1024) s_listed[i] = s_fresh[i] = s_hb[i] = 0u;
    __syncthreads();
    const uint32_t total = uint32_t(a.rows) * uint32_t(a.view);
    for (uint64_t i = uint64_t(blockIdx.x) * 1024u + threadIdx.x; i < total; i += uint64_t(gridDim.x) * 1024u) {
        uint32_t id, hb, fresh;
        if (!census_slot(a, uint32_t(i), id, hb, fresh)) continue;
        if (id < uint32_t(kCensusCut)) {
            atomicAdd(&s_listed[id], 1u);
            if (fresh) atomicAdd(&s_fresh[id], 1u);
            atomicMax(&s_hb[id], hb);
        } else {
            census_count(a, id, hb, fresh);
        }
    }
    __syncthreads();
    const int cut = a.n < kCensusCut ? a.n : kCensusCut;
    for (int i = int(threadIdx.x); i < cut; i += 1024)
        if (s_listed[i]) {
            atomicAdd(&a.counts[i], (uint64_t(s_fresh[i]) << 32) | uint64_t(s_listed[i]));
            atomicMax(&a.max_hb[i], s_hb[i]);
        }
}

}  // namespace

hipError_t launch_census_scale(const CensusScaleArgs &a, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.n) - a.col0 ? a.stride : int64_t(a.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kCensusStrip) return hipErrorInvalidValue;
    const dim3 grid(unsigned((cols + kCensusStrip - 1) / kCensusStrip),
                    unsigned((a.rows + kCensusRows - 1) / kCensusRows));
    hipLaunchKernelGGL(census_scale_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_census_pview(const CensusPviewArgs &a, bool lds, int32_t cus, hipStream_t st) {
    const int64_t total = int64_t(a.rows) * a.view;
    if (total <= 0) return hipSuccess;
    if (total >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (lds) {
        const int64_t want = (total + 1023) / 1024, cap = int64_t(cus > 0 ? cus : 256) * 2;
        hipLaunchKernelGGL(census_pview_lds_kernel, dim3(unsigned(want < cap ? want : cap)), dim3(1024),
                           0, st, a);
    } else {
        hipLaunchKernelGGL(census_pview_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace gsp
