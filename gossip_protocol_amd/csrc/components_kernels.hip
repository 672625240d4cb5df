// gossip_protocol_amd/csrc/components_kernels.hip -- the overlay-components kernels
// (components_kernels.hpp).
#include "components_kernels.hpp"
#include "reach_row.hpp"
#include "wave_ops.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ uint32_t comp_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// weak: hook the root `top` below `low` (< top).  Once the trees are few, most edges of a sweep
// name the same root: the load spares the atomics that would queue on its one word (a stale read
// costs a redundant atomic, never a different result).
__device__ __forceinline__ void comp_hook(const CompCommon &c, uint32_t top, uint32_t low) {
    if (comp_load(&c.lab[top]) > low) atomicMin(&c.lab[top], low);
}

// The sweeps fold with max alone: strong colours as they are, weak labels complemented, so the
// smallest label is the largest word and kCompNone is 0, the identity of wave_max32.
template <bool kWeak>
__device__ __forceinline__ uint32_t comp_enc(uint32_t v) {
    return kWeak ? ~v : v;
}

// The row side of one row r of a wave: `racc` is each lane's fold of the words of the members the
// row lists, `mine` the row's own word (weak: ~lab[r], strong: bcol[r]), `any` whether the lane
// saw a counted edge.  One atomic per row, and only where the word would move.
template <bool kWeak>
__device__ __forceinline__ void comp_row_side(const CompCommon &c, int lane, uint32_t r, uint32_t racc,
                                              uint32_t mine, bool any) {
    if (__ballot(racc > mine)) {
        const uint32_t red = wave_max32(racc);
        if (lane == 0) {
            if (kWeak) comp_hook(c, ~mine, ~red);             // r's root below the smallest
            else atomicMax(&c.bcol[r], red);
        }
    }
    if (!kWeak && c.first && __ballot(any) && lane == 0) c.has_out[r] = 1u;
}

// ---- the n-length kernels: a workgroup takes kReachChunk nodes, a wave 64 at a time ------------
// (one ballot is one bitmap word; no lane leaves early, the wave sums need all of them)

__global__ void __launch_bounds__(256) comp_weak_init_kernel(CompCommon c) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        const bool alive = x < uint32_t(c.n) && reach_alive_at(c.start_tick, c.fail_tick, c.tick, int32_t(x));
        c.lab[x] = alive ? x : kCompNone;
        if (alive) sum += x;
        const uint64_t w = __ballot(alive);
        if (lane == 0) c.active[word] = w;
    }
    sum = wave_sum64(sum);
    if (lane == 0 && sum) atomicAdd(&c.ctr[kCompBase], (unsigned long long)sum);
}

// every alive node to its root
__global__ void __launch_bounds__(256) comp_weak_jump_kernel(CompCommon c) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        uint32_t l = c.lab[x];
        if (l != kCompNone) {
            // lab[l] <= l and a root holds itself: the walk only goes down and ends
            for (uint32_t p = comp_load(&c.lab[l]); p != l; p = comp_load(&c.lab[l])) l = p;
            c.lab[x] = l;
            sum += l;
        }
    }
    sum = wave_sum64(sum);
    if (lane == 0 && sum) atomicAdd(&c.ctr[kCompSum], (unsigned long long)sum);
}

__global__ void __launch_bounds__(256) comp_turn_kernel(CompCommon c, int opening) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint64_t sum = 0;
    uint32_t left = 0;
#pragma unroll
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        bool open = x < uint32_t(c.n) && reach_alive_at(c.start_tick, c.fail_tick, c.tick, int32_t(x));
        if (open && !opening) {
            open = false;
            if (c.comp[x] == kCompNone) {
                const uint32_t f = c.fcol[x], b = c.bcol[x];
                if (!c.has_in[x] || !c.has_out[x]) c.comp[x] = x;          // trimmed
                else if (f == b) c.comp[x] = f;                            // f reaches x, x reaches f
                else {
                    open = true;
                    c.pf[x] = f;
                    c.pb[x] = b;
                }
            }
        }
        if (open) {
            if (opening) c.pf[x] = c.pb[x] = 0u;                           // one part
            c.fcol[x] = x;
            c.bcol[x] = x;
            c.has_in[x] = 0u;
            c.has_out[x] = 0u;
            sum += 2ull * x;
        }
        const uint64_t w = __ballot(open);
        if (lane == 0) c.active[word] = w;
        left += uint32_t(__builtin_popcountll(w));
    }
    sum = wave_sum64(sum);
    if (lane == 0 && left) {
        atomicAdd(&c.ctr[kCompBase], (unsigned long long)sum);
        atomicAdd(&c.ctr[kCompLeft], (unsigned long long)left);
    }
}

// every open node's colours to the colours of its colours
__global__ void __launch_bounds__(256) comp_strong_jump_kernel(CompCommon c) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        if ((c.active[word] >> lane) & 1ull) {
            // a colour is an open node's id and col[id] >= id: the walk only goes up and ends
            uint32_t f = c.fcol[x], b = c.bcol[x];
            for (uint32_t p = comp_load(&c.fcol[f]); p > f; p = comp_load(&c.fcol[f])) f = p;
            for (uint32_t p = comp_load(&c.bcol[b]); p > b; p = comp_load(&c.bcol[b])) b = p;
            c.fcol[x] = f;
            c.bcol[x] = b;
            sum += uint64_t(f) + b;
        }
    }
    sum = wave_sum64(sum);
    if (lane == 0 && sum) atomicAdd(&c.ctr[kCompSum], (unsigned long long)sum);
}

// pass 0: pf[comp[x]] = min x (pf was set to all ones); pass 1: lab[x] = pf[comp[x]]
__global__ void __launch_bounds__(256) comp_canon_kernel(CompCommon c, int pass) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;         // the grid is components_nodes(n) / 256
    const bool alive = x < uint32_t(c.n) && reach_alive_at(c.start_tick, c.fail_tick, c.tick, int32_t(x));
    const uint32_t top = alive ? c.comp[x] : kCompNone;
    if (pass == 0) {
        // A giant component has whole waves under one top: their smallest x is the first such
        // lane's, one atomic.  Otherwise one per lane; the load spares those that cannot lower it.
        const bool in = top < uint32_t(c.n);
        const uint64_t ins = __ballot(in);
        if (!ins) return;
        const int l0 = __builtin_ctzll(ins);
        const bool same = __ballot(in && top != lane_of(top, l0)) == 0ull;
        if (in && (!same || int(threadIdx.x & 63u) == l0) && comp_load(&c.pf[top]) > x) atomicMin(&c.pf[top], x);
    } else {
        c.lab[x] = top < uint32_t(c.n) ? c.pf[top] : kCompNone;
    }
}

// ---- full view (reach_fresh / reach_pack: reach_row.hpp) --------------------------------------
// Work item = (512-column strip, block of 256 rows), reach's FROM shape: a wave takes every
// fourth row of the block.  Columns >= n are stride padding and have no active bit.
template <bool kWeak>
__global__ void __launch_bounds__(256) comp_scale_kernel(CompScaleArgs a) {
    const CompCommon &c = a.c;
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kReachRows;
    const int64_t c0 = int64_t(blockIdx.x) * kReachStrip;
    const int64_t gc0 = int64_t(a.col0) + c0;                    // a multiple of 512
    const uint32_t colact = reinterpret_cast<const uint8_t *>(c.active)[gc0 / 8 + lane];
    if (__ballot(colact != 0u) == 0ull) return;

    // lane j: the wave's j-th row (rb + wave + 4 j), its words where it is active
    const int32_t lr = rb + wave + 4 * lane;
    const bool rowact = lr < a.rows && reach_bit(c.active, uint32_t(a.row0 + lr));
    uint64_t rows = __ballot(rowact);
    if (!rows) return;
    const uint32_t myr = uint32_t(a.row0 + (rowact ? lr : 0));
    const uint32_t rw = rowact ? comp_enc<kWeak>(kWeak ? c.lab[myr] : c.fcol[myr]) : 0u;
    const uint32_t rbk = !kWeak && rowact ? c.bcol[myr] : 0u;
    const uint32_t rpf = !kWeak && rowact ? c.pf[myr] : 0u;
    const uint32_t rpb = !kWeak && rowact ? c.pb[myr] : 0u;

    // the lane's eight columns: the word the rows fold (weak ~lab, strong bcol), the part, and
    // the fold of the rows' words (weak ~lab[r], strong fcol[r])
    const uint32_t gx0 = uint32_t(gc0) + uint32_t(lane * kEntriesPerLane);
    uint32_t cw[kEntriesPerLane], cpf[kEntriesPerLane], cpb[kEntriesPerLane], cacc[kEntriesPerLane];
    const uint32_t *wsrc = kWeak ? c.lab : c.bcol;
#pragma unroll
    for (int q = 0; q < kEntriesPerLane; ++q) {
        cw[q] = comp_enc<kWeak>(wsrc[gx0 + q]);
        cpf[q] = kWeak ? 0u : c.pf[gx0 + q];
        cpb[q] = kWeak ? 0u : c.pb[gx0 + q];
        cacc[q] = 0u;
    }
    uint32_t cany = 0;

    const uint32_t t5 = uint32_t(c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(c.age_limit) | (uint32_t(c.age_limit) << 16);
    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const uint4 v = ld16<true>(base + j * step);
        const uint32_t r = uint32_t(a.row0 + rb + wave + 4 * j);
        const uint32_t f[4] = {reach_fresh(v.x, t5x2, lim), reach_fresh(v.y, t5x2, lim),
                               reach_fresh(v.z, t5x2, lim), reach_fresh(v.w, t5x2, lim)};
        uint32_t m = reach_pack(f) & colact;
        const uint32_t self = r - gx0;                               // r -> r is no edge
        if (self < uint32_t(kEntriesPerLane)) m &= ~(1u << self);
        const uint32_t ar = lane_of(rw, j);
        if (!kWeak) {
            const uint32_t pfr = lane_of(rpf, j), pbr = lane_of(rpb, j);
#pragma unroll
            for (int q = 0; q < kEntriesPerLane; ++q)
                if (cpf[q] != pfr || cpb[q] != pbr) m &= ~(1u << q);
        }
        uint32_t racc = 0;
#pragma unroll
        for (int q = 0; q < kEntriesPerLane; ++q)
            if ((m >> q) & 1u) {
                cacc[q] = max(cacc[q], ar);
                racc = max(racc, cw[q]);
            }
        cany |= m;
        comp_row_side<kWeak>(c, lane, r, racc, kWeak ? ar : lane_of(rbk, j), m != 0u);
    }
    // the column side: one atomic per column, and only where the word would move
#pragma unroll
    for (int q = 0; q < kEntriesPerLane; ++q) {
        if (!((cany >> q) & 1u)) continue;
        const uint32_t x = gx0 + uint32_t(q);
        if (kWeak) {
            if (cacc[q] > cw[q]) comp_hook(c, ~cw[q], ~cacc[q]);        // x's root
        } else {
            if (cacc[q] > comp_load(&c.fcol[x])) atomicMax(&c.fcol[x], cacc[q]);
            if (c.first) c.has_in[x] = 1u;
        }
    }
}

// ---- partial view -----------------------------------------------------------------------------
// A wave takes 64 consecutive rows and walks the active ones 64 slots at a time.  Only the slots
// below len are read; an id >= n is dropped before it becomes an address.
template <bool kWeak>
__global__ void __launch_bounds__(256) comp_pview_kernel(CompPviewArgs a) {
    const CompCommon &c = a.c;
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    const bool rowact = lr < a.rows && reach_bit(c.active, uint32_t(a.row0 + lr));
    uint64_t rows = __ballot(rowact);
    if (!rows) return;
    const uint32_t myr = uint32_t(a.row0 + (rowact ? lr : 0));
    const uint32_t rw = rowact ? comp_enc<kWeak>(kWeak ? c.lab[myr] : c.fcol[myr]) : 0u;
    const uint32_t rbk = !kWeak && rowact ? c.bcol[myr] : 0u;
    const uint32_t rpf = !kWeak && rowact ? c.pf[myr] : 0u;
    const uint32_t rpb = !kWeak && rowact ? c.pb[myr] : 0u;
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t row = base + j;
        const uint32_t r = uint32_t(a.row0 + row);
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        const uint32_t ar = lane_of(rw, j);
        const uint32_t pfr = lane_of(rpf, j), pbr = lane_of(rpb, j);
        uint32_t racc = 0;
        bool any = false;
        for (int32_t s = lane; s < len; s += 64) {
            uint32_t id;
            if (!reach_entry_at(view[s], c.n, c.tick, c.age_limit, id) || id == r || !reach_bit(c.active, id))
                continue;
            if (kWeak) {
                const uint32_t xw = ~comp_load(&c.lab[id]);
                racc = max(racc, xw);
                if (ar > xw) comp_hook(c, ~xw, ~ar);                    // id's root below r's
            } else {
                if (c.pf[id] != pfr || c.pb[id] != pbr) continue;
                racc = max(racc, comp_load(&c.bcol[id]));
                if (ar > comp_load(&c.fcol[id])) atomicMax(&c.fcol[id], ar);
                if (c.first) c.has_in[id] = 1u;
            }
            any = true;
        }
        comp_row_side<kWeak>(c, lane, r, racc, kWeak ? ar : lane_of(rbk, j), any);
    }
}

inline unsigned comp_chunks(int32_t n) { return unsigned(components_nodes(n) / kReachChunk); }

}  // namespace

hipError_t launch_components_weak_init(const CompCommon &c, hipStream_t st) {
    if (c.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(comp_weak_init_kernel, dim3(comp_chunks(c.n)), dim3(256), 0, st, c);
    return hipGetLastError();
}

hipError_t launch_components_turn(const CompCommon &c, bool opening, hipStream_t st) {
    if (c.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(comp_turn_kernel, dim3(comp_chunks(c.n)), dim3(256), 0, st, c, int(opening));
    return hipGetLastError();
}

hipError_t launch_components_jump(const CompCommon &c, hipStream_t st) {
    if (c.n <= 0) return hipSuccess;
    if (c.kind == kCompWeak) hipLaunchKernelGGL(comp_weak_jump_kernel, dim3(comp_chunks(c.n)), dim3(256), 0, st, c);
    else hipLaunchKernelGGL(comp_strong_jump_kernel, dim3(comp_chunks(c.n)), dim3(256), 0, st, c);
    return hipGetLastError();
}

hipError_t launch_components_canon(const CompCommon &c, hipStream_t st) {
    if (c.n <= 0) return hipSuccess;
    const size_t nodes = components_nodes(c.n);
    if (hipError_t e = hipMemsetAsync(c.pf, 0xFF, nodes * 4, st)) return e;
    for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(comp_canon_kernel, dim3(unsigned(nodes / 256)), dim3(256), 0, st, c, pass);
    return hipGetLastError();
}

hipError_t launch_components_scale(const CompScaleArgs &a, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kReachStrip || a.col0 % kReachStrip || a.col0 < 0 || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.c.n)
        return hipErrorInvalidValue;
    const dim3 grid(unsigned((cols + kReachStrip - 1) / kReachStrip),
                    unsigned((a.rows + kReachRows - 1) / kReachRows));
    if (a.c.kind == kCompWeak) hipLaunchKernelGGL(comp_scale_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(comp_scale_kernel<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_components_pview(const CompPviewArgs &a, hipStream_t st) {
    if (a.rows <= 0 || a.view <= 0) return hipSuccess;
    if (a.row0 < 0 || int64_t(a.row0) + a.rows > a.c.n) return hipErrorInvalidValue;
    const dim3 grid(unsigned((a.rows + 255) / 256));
    if (a.c.kind == kCompWeak) hipLaunchKernelGGL(comp_pview_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(comp_pview_kernel<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
