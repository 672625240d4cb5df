// gossip_protocol_amd/csrc/reach_multi_kernels.hip -- the multi-source reach kernels
// (reach_multi_kernels.hpp): the four row forms of reach_kernels.hip with a 64-bit word per node.
#include "reach_multi_kernels.hpp"
#include "reach_row.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ uint64_t wave_or64(uint64_t x) {
    return (uint64_t(wave_or32(uint32_t(x >> 32))) << 32) | wave_or32(uint32_t(x));
}

__device__ __forceinline__ void or_into(uint64_t *p, uint64_t bits) {
    atomicOr(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(bits));
}

__global__ void __launch_bounds__(64) reach_multi_seed_kernel(const int32_t *sources, ReachMultiLevelArgs a) {
    const int32_t b = int32_t(threadIdx.x);
    if (b >= a.n_sources) return;
    const int32_t id = sources[b];                        // in [0, n): checked by the host
    if (reach_alive_at(a.start_tick, a.fail_tick, a.tick, id)) or_into(&a.next[id], 1ull << b);
}

// After a level (and after the seed): admit what the launch ORed into next.  A workgroup takes
// kReachChunk nodes, a wave 64 of them at a time, one node per lane: one ballot is one bitmap
// word.  Lane b of the wave counts tree b: for every bit some lane has gained, the ballot of
// that bit is its count over the wave's 64 nodes, and where hops are wanted the same lanes store
// the level, consecutive x of one row of hops, i.e. one coalesced store.  One atomicAdd per lane
// and wave then goes into the 64 cumulative counters.
__global__ void __launch_bounds__(256) reach_multi_level_kernel(ReachMultiLevelArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint32_t found = 0;
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        uint64_t nw = 0;
        bool open = false;
        if (x < uint32_t(a.n)) {
            const uint64_t s = a.seen[x], nx = a.next[x];
            nw = nx & ~s;
            if (nw) a.seen[x] = s | nw;
            if (nx) a.next[x] = 0;
            a.front[x] = nw;
            open = (a.want & ~(s | nw)) != 0 && reach_alive_at(a.start_tick, a.fail_tick, a.tick, int32_t(x));
        }
        const uint64_t h = __ballot(nw != 0), o = __ballot(open);
        if (lane == 0) {
            a.hot[word] = h;
            a.open[word] = o;
        }
        if (!h) continue;                                 // wave-uniform
        uint64_t any = wave_or64(nw);
        while (any) {
            const int b = __builtin_ctzll(any);
            any &= any - 1;
            const bool mine = (nw >> b) & 1u;
            const uint32_t c = uint32_t(__builtin_popcountll(__ballot(mine)));
            if (lane == b) found += c;
            if (a.hops && mine) a.hops[size_t(b) * size_t(a.n) + x] = a.level;
        }
    }
    if (found) atomicAdd(&a.count[lane], found);
}

__global__ void __launch_bounds__(256) reach_multi_fold_kernel(const uint64_t *stage, int32_t world,
                                                               size_t nodes, uint64_t *next) {
    const size_t x = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (x >= nodes) return;
    uint64_t v = 0;
    for (int32_t w = 0; w < world; ++w) v |= stage[size_t(w) * nodes + x];
    next[x] = v;
}

// ---- full view -------------------------------------------------------------------------------
// acc[q] |= fr where entry q of the lane vector is present and fresh; acc as lo / hi halves, the
// flag (0 / 1) stretched to a mask by a negate
__device__ __forceinline__ void multi_or(uint32_t (&lo)[8], uint32_t (&hi)[8], const uint4 &v, uint64_t fr,
                                         uint32_t t5x2, uint32_t lim) {
    const uint32_t f[4] = {reach_fresh(v.x, t5x2, lim), reach_fresh(v.y, t5x2, lim),
                           reach_fresh(v.z, t5x2, lim), reach_fresh(v.w, t5x2, lim)};
    const uint32_t flo = uint32_t(fr), fhi = uint32_t(fr >> 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t m0 = 0u - (f[i] & 1u), m1 = 0u - (f[i] >> 16);
        lo[2 * i] |= m0 & flo;
        hi[2 * i] |= m0 & fhi;
        lo[2 * i + 1] |= m1 & flo;
        hi[2 * i + 1] |= m1 & fhi;
    }
}

// FROM.  reach_scale_from's work item, a 512-column strip x a block of 256 rows, a wave taking
// every fourth row.  The strip's byte of `open` per lane comes first: a strip whose columns miss
// nothing ends before any row is looked at.  Lane j then loads the front word of the wave's j-th
// row, the ballot of "non-zero" selects the rows to load, and a selected row's word (wave-uniform,
// by readlane) is ORed into the accumulators of the lane's present-and-fresh columns.  At the end
// one atomicOr per open column with anything seen[col] lacks.  Columns >= n are stride padding
// and have no open bit.
__global__ void __launch_bounds__(256) reach_multi_scale_from_kernel(ReachMultiScaleArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kReachRows;
    const int64_t c0 = int64_t(blockIdx.x) * kReachStrip;
    const int64_t gc0 = int64_t(a.col0) + c0;                    // a multiple of 512
    const uint32_t want = reinterpret_cast<const uint8_t *>(a.c.open)[gc0 / 8 + lane];
    if (__ballot(want != 0u) == 0ull) return;

    const int32_t lr = rb + wave + 4 * lane;                     // the wave's lane-th row
    const uint64_t fw = lr < a.rows ? a.c.front[a.row0 + lr] : 0ull;
    uint64_t rows = __ballot(fw != 0ull);
    if (!rows) return;

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    uint32_t lo[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, hi[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    while (__builtin_popcountll(rows) >= 4) {
        uint4 v[4];
        int js[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            js[q] = __builtin_ctzll(rows);
            rows &= rows - 1;
            v[q] = ld16<true>(base + js[q] * step);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) multi_or(lo, hi, v[q], lane_of(fw, js[q]), t5x2, lim);
    }
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        multi_or(lo, hi, ld16<true>(base + j * step), lane_of(fw, j), t5x2, lim);
    }
#pragma unroll
    for (int q = 0; q < kEntriesPerLane; ++q) {
        if (!((want >> q) & 1u) || !(lo[q] | hi[q])) continue;
        const uint32_t col = uint32_t(gc0) + uint32_t(lane * kEntriesPerLane + q);
        const uint64_t nw = ((uint64_t(hi[q]) << 32) | lo[q]) & ~a.c.seen[col];
        if (nw) or_into(&a.c.next[col], nw);
    }
}

// TO.  One wave per row; a row with no open bit ends at once.  The others walk their row in 16-B
// vectors, four in flight, against the `hot` bits of the same columns, load the front word of
// every present-and-fresh hot column and OR it; after each group the wave's OR is tested and the
// row leaves once it covers everything the row still misses.  Column tiles share a row, hence the
// atomicOr.
__global__ void __launch_bounds__(256) reach_multi_scale_to_kernel(ReachMultiScaleArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t lr = int32_t(blockIdx.x) * 4 + wave;
    if (lr >= a.rows) return;
    const uint32_t r = uint32_t(a.row0 + lr);
    if (!reach_bit(a.c.open, r)) return;
    const uint64_t miss = a.c.want & ~a.c.seen[r];               // non-zero: r is open

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    const int32_t strips = int32_t((cols + kReachStrip - 1) / kReachStrip);
    const uint16_t *row = a.table + int64_t(lr) * a.stride + lane * kEntriesPerLane;
    const uint8_t *hot = reinterpret_cast<const uint8_t *>(a.c.hot) + a.col0 / 8 + lane;
    const uint64_t *fr = a.c.front + a.col0 + lane * kEntriesPerLane;
    uint64_t got = 0;
    for (int32_t s0 = 0; s0 < strips; s0 += 4) {
        uint4 v[4];
        uint32_t hb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = s0 + q < strips;                      // wave-uniform
            v[q] = in ? ld16<true>(row + int64_t(s0 + q) * kReachStrip) : make_uint4(0u, 0u, 0u, 0u);
            hb[q] = in ? uint32_t(hot[(s0 + q) * (kReachStrip / 8)]) : 0u;
        }
        uint64_t acc = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t f[4] = {reach_fresh(v[q].x, t5x2, lim), reach_fresh(v[q].y, t5x2, lim),
                                   reach_fresh(v[q].z, t5x2, lim), reach_fresh(v[q].w, t5x2, lim)};
            uint32_t hit = reach_pack(f) & hb[q];
            while (hit) {
                const int e = __builtin_ctz(hit);
                hit &= hit - 1;
                acc |= fr[int64_t(s0 + q) * kReachStrip + e];
            }
        }
        got |= wave_or64(acc);
        if ((got & miss) == miss) break;
    }
    if (lane == 0 && (got & miss)) or_into(&a.c.next[r], got & miss);
}

// ---- partial view ----------------------------------------------------------------------------
// Both forms: a wave takes 64 consecutive rows, tests them with one coalesced read and one
// ballot, and walks only the selected rows, 64 slots at a time.  Only the slots below len are read.
__device__ __forceinline__ bool multi_entry(const ReachMultiPviewArgs &a, uint64_t e, uint32_t &id) {
    return reach_entry_at(e, a.c.n, a.c.tick, a.c.age_limit, id);
}

// FROM (push): the rows whose front word is non-zero; per fresh entry whose target is open, what
// of the row's word the target lacks (a plain load), and an atomicOr only where that is non-zero
__global__ void __launch_bounds__(256) reach_multi_pview_from_kernel(ReachMultiPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    const uint64_t fw = lr < a.rows ? a.c.front[a.row0 + lr] : 0ull;
    uint64_t rows = __ballot(fw != 0ull);
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t row = base + j;
        const uint64_t f = lane_of(fw, j);
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        for (int32_t s = lane; s < len; s += 64) {
            uint32_t id;
            if (!multi_entry(a, view[s], id) || !reach_bit(a.c.open, id)) continue;
            const uint64_t nw = f & ~a.c.seen[id];
            if (nw) or_into(&a.c.next[id], nw);
        }
    }
}

// TO (pull): every open row ORs the front words of its fresh hot entries; no scatter.  The row
// is this wave's alone (row shards hold disjoint rows), so one lane stores into the zero word.
__global__ void __launch_bounds__(256) reach_multi_pview_to_kernel(ReachMultiPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    const uint64_t ms = lr < a.rows && reach_bit(a.c.open, uint32_t(a.row0 + lr))
                            ? a.c.want & ~a.c.seen[a.row0 + lr] : 0ull;
    uint64_t rows = __ballot(ms != 0ull);
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t row = base + j;
        const uint64_t miss = lane_of(ms, j);
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        uint64_t got = 0;
        for (int32_t s0 = 0; s0 < len; s0 += 64) {
            uint32_t id;
            uint64_t acc = 0;
            if (s0 + lane < len && multi_entry(a, view[s0 + lane], id) && reach_bit(a.c.hot, id))
                acc = a.c.front[id];
            got |= wave_or64(acc);
            if ((got & miss) == miss) break;
        }
        if (lane == 0 && (got & miss)) a.c.next[a.row0 + row] = got & miss;
    }
}

}  // namespace

hipError_t launch_reach_multi_seed(const int32_t *sources, const ReachMultiLevelArgs &a, hipStream_t st) {
    if (a.n_sources <= 0 || a.n_sources > kReachMultiMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reach_multi_seed_kernel, dim3(1), dim3(64), 0, st, sources, a);
    return hipGetLastError();
}

hipError_t launch_reach_multi_level(const ReachMultiLevelArgs &a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(reach_multi_level_kernel, dim3(unsigned((a.n + kReachChunk - 1) / kReachChunk)),
                       dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_reach_multi_scale(const ReachMultiScaleArgs &a, bool to, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kReachStrip || a.col0 % kReachStrip || a.col0 < 0 || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.c.n)
        return hipErrorInvalidValue;
    if (to) {
        hipLaunchKernelGGL(reach_multi_scale_to_kernel, dim3(unsigned((a.rows + 3) / 4)), dim3(256), 0, st, a);
    } else {
        const dim3 grid(unsigned((cols + kReachStrip - 1) / kReachStrip),
                        unsigned((a.rows + kReachRows - 1) / kReachRows));
        hipLaunchKernelGGL(reach_multi_scale_from_kernel, grid, dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_reach_multi_pview(const ReachMultiPviewArgs &a, bool to, hipStream_t st) {
    if (a.rows <= 0 || a.view <= 0) return hipSuccess;
    if (a.row0 < 0 || int64_t(a.row0) + a.rows > a.c.n) return hipErrorInvalidValue;
    const dim3 grid(unsigned((a.rows + 255) / 256));
    if (to) hipLaunchKernelGGL(reach_multi_pview_to_kernel, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(reach_multi_pview_from_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_reach_multi_fold(const uint64_t *stage, int32_t world, size_t nodes, uint64_t *next,
                                   hipStream_t st) {
    if (world <= 0 || nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(reach_multi_fold_kernel, dim3(unsigned((nodes + 255) / 256)), dim3(256), 0, st, stage,
                       world, nodes, next);
    return hipGetLastError();
}

}  // namespace gsp
