// gossip_protocol_amd/csrc/reach_kernels.hip -- the overlay-reach kernels (reach_kernels.hpp).
#include "reach_kernels.hpp"
#include "reach_row.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ bool reach_alive(const ReachCommon &c, int32_t r) {
    return reach_alive_at(c.start_tick, c.fail_tick, c.tick, r);
}

// every writer of a launch stores the same cur + 1; the load only spares the atomic (a stale
// unset costs a redundant one)
__device__ __forceinline__ void reach_set(const ReachCommon &c, uint32_t x) {
    if (__hip_atomic_load(&c.hops[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kReachUnset)
        atomicMin(&c.hops[x], c.cur + 1u);
}

__global__ void __launch_bounds__(256) reach_seed_kernel(const int32_t *sources, int32_t n_sources,
                                                         ReachCommon c) {
    const int32_t i = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    if (i >= n_sources) return;
    const int32_t id = sources[i];                        // in [0, n): checked by the host
    if (reach_alive(c, id)) c.hops[id] = 0u;              // duplicates store the same value
}

// After a level: count the nodes at `level` and rewrite both bitmaps whole.  A workgroup takes
// kReachChunk nodes, a wave 64 of them at a time: one ballot is one bitmap word.
__global__ void __launch_bounds__(256) reach_level_kernel(ReachCommon c, uint32_t level, uint64_t *front,
                                                          uint64_t *todo, uint32_t *count) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint32_t found = 0;
#pragma unroll
    for (int k = 0; k < kReachChunk / 256; ++k) {
        const uint32_t word = blockIdx.x * uint32_t(kReachChunk / 64) + uint32_t(k * 4 + wave);
        const uint32_t x = word * 64u + uint32_t(lane);
        bool at = false, open = false;
        if (x < uint32_t(c.n)) {
            const uint32_t h = c.hops[x];
            at = h == level;
            open = h == kReachUnset && reach_alive(c, int32_t(x));
        }
        const uint64_t f = __ballot(at), o = __ballot(open);
        if (lane == 0) {
            front[word] = f;
            todo[word] = o;
        }
        found += uint32_t(__builtin_popcountll(f));
    }
    if (lane == 0 && found) atomicAdd(count, found);
}

// ---- full view (reach_fresh / reach_pack: reach_row.hpp) --------------------------------------
__device__ __forceinline__ void reach_or(uint32_t (&acc)[4], const uint4 &v, uint32_t t5x2, uint32_t lim) {
    acc[0] |= reach_fresh(v.x, t5x2, lim);
    acc[1] |= reach_fresh(v.y, t5x2, lim);
    acc[2] |= reach_fresh(v.z, t5x2, lim);
    acc[3] |= reach_fresh(v.w, t5x2, lim);
}

// FROM.  Work item = (512-column strip, block of 256 rows), the census's shape: a wave reads
// the strip of one row as one 1-KiB instruction and takes every fourth row of the block.  The
// strip's byte of `todo` per lane comes first: a strip with no unreached alive column ends the
// workgroup before any row is looked at.  The wave's ballot then selects its frontier rows,
// only those are loaded, and each lane ORs present & fresh of its 8 columns; what is left after
// the todo mask goes out as one atomicMin per column.  Columns >= n are stride padding and
// have no todo bit.
__global__ void __launch_bounds__(256) reach_scale_from_kernel(ReachScaleArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kReachRows;
    const int64_t c0 = int64_t(blockIdx.x) * kReachStrip;
    const int64_t gc0 = int64_t(a.col0) + c0;                    // a multiple of 512
    const uint32_t want = reinterpret_cast<const uint8_t *>(a.c.todo)[gc0 / 8 + lane];
    if (__ballot(want != 0u) == 0ull) return;

    // lane j: is the wave's j-th row (rb + wave + 4 j) in the frontier?
    const int32_t lr = rb + wave + 4 * lane;
    uint64_t rows = __ballot(lr < a.rows && a.c.hops[a.row0 + lr] == a.c.cur);
    if (!rows) return;

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    while (__builtin_popcountll(rows) >= 4) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = __builtin_ctzll(rows);
            rows &= rows - 1;
            v[q] = ld16<true>(base + j * step);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) reach_or(acc, v[q], t5x2, lim);
    }
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        reach_or(acc, ld16<true>(base + j * step), t5x2, lim);
    }
    uint32_t hit = reach_pack(acc) & want;
    while (hit) {
        const int q = __builtin_ctz(hit);
        hit &= hit - 1;
        reach_set(a.c, uint32_t(gc0) + uint32_t(lane * kEntriesPerLane + q));
    }
}

// TO.  One wave per row.  A row that is not alive or already reached (its todo bit, then its
// hops word: another column tile of this level may have reached it) ends at once; the others
// walk their row in 16-B vectors, four in flight, against the frontier bits of the same columns
// and leave at the first hit.  A frontier bit implies an alive member.
__global__ void __launch_bounds__(256) reach_scale_to_kernel(ReachScaleArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t lr = int32_t(blockIdx.x) * 4 + wave;
    if (lr >= a.rows) return;
    const uint32_t r = uint32_t(a.row0 + lr);
    if (!reach_bit(a.c.todo, r) || a.c.hops[r] != kReachUnset) return;

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    const int32_t strips = int32_t((cols + kReachStrip - 1) / kReachStrip);
    const uint16_t *row = a.table + int64_t(lr) * a.stride + lane * kEntriesPerLane;
    const uint8_t *fr = reinterpret_cast<const uint8_t *>(a.c.front) + a.col0 / 8 + lane;
    for (int32_t s0 = 0; s0 < strips; s0 += 4) {
        uint4 v[4];
        uint32_t fb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = s0 + q < strips;                      // wave-uniform
            v[q] = in ? ld16<true>(row + int64_t(s0 + q) * kReachStrip) : make_uint4(0u, 0u, 0u, 0u);
            fb[q] = in ? uint32_t(fr[(s0 + q) * (kReachStrip / 8)]) : 0u;
        }
        uint32_t hit = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t f[4] = {reach_fresh(v[q].x, t5x2, lim), reach_fresh(v[q].y, t5x2, lim),
                                   reach_fresh(v[q].z, t5x2, lim), reach_fresh(v[q].w, t5x2, lim)};
            hit |= reach_pack(f) & fb[q];
        }
        if (__ballot(hit != 0u)) {
            if (lane == 0) atomicMin(&a.c.hops[r], a.c.cur + 1u);
            return;
        }
    }
}

// ---- partial view ----------------------------------------------------------------------------
// Both forms: a wave takes 64 consecutive rows, tests them with one coalesced read of their
// hops words (TO: and todo bits) and one ballot, and walks only the selected rows, 64 slots at
// a time.  Only the slots below len are read; an id >= n is dropped before it becomes an address.
__device__ __forceinline__ bool reach_entry(const ReachPviewArgs &a, uint64_t e, uint32_t &id) {
    return reach_entry_at(e, a.c.n, a.c.tick, a.c.age_limit, id);
}

// FROM (push): the frontier rows' fresh entries whose target is alive and unset
__global__ void __launch_bounds__(256) reach_pview_from_kernel(ReachPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    uint64_t rows = __ballot(lr < a.rows && a.c.hops[a.row0 + lr] == a.c.cur);
    while (rows) {
        const int32_t row = base + __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        for (int32_t s = lane; s < len; s += 64) {
            uint32_t id;
            if (reach_entry(a, view[s], id) && reach_bit(a.c.todo, id)) reach_set(a.c, id);
        }
    }
}

// TO (pull): every unreached alive row looks for a fresh entry in the frontier; no scatter
__global__ void __launch_bounds__(256) reach_pview_to_kernel(ReachPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    uint64_t rows = __ballot(lr < a.rows && reach_bit(a.c.todo, uint32_t(a.row0 + lr)));
    while (rows) {
        const int32_t row = base + __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        for (int32_t s0 = 0; s0 < len; s0 += 64) {
            uint32_t id;
            const bool hit = s0 + lane < len && reach_entry(a, view[s0 + lane], id) && reach_bit(a.c.front, id);
            if (__ballot(hit)) {
                if (lane == 0) atomicMin(&a.c.hops[a.row0 + row], a.c.cur + 1u);
                break;
            }
        }
    }
}

}  // namespace

hipError_t launch_reach_seed(const int32_t *sources, int32_t n_sources, const ReachCommon &c,
                             hipStream_t st) {
    if (n_sources <= 0) return hipSuccess;
    hipLaunchKernelGGL(reach_seed_kernel, dim3(unsigned((n_sources + 255) / 256)), dim3(256), 0, st,
                       sources, n_sources, c);
    return hipGetLastError();
}

hipError_t launch_reach_level(const ReachCommon &c, uint32_t level, uint64_t *front, uint64_t *todo,
                              uint32_t *count, hipStream_t st) {
    if (c.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(reach_level_kernel, dim3(unsigned((c.n + kReachChunk - 1) / kReachChunk)), dim3(256),
                       0, st, c, level, front, todo, count);
    return hipGetLastError();
}

hipError_t launch_reach_scale(const ReachScaleArgs &a, bool to, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kReachStrip || a.col0 % kReachStrip || a.col0 < 0 || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.c.n)
        return hipErrorInvalidValue;
    if (to) {
        hipLaunchKernelGGL(reach_scale_to_kernel, dim3(unsigned((a.rows + 3) / 4)), dim3(256), 0, st, a);
    } else {
        const dim3 grid(unsigned((cols + kReachStrip - 1) / kReachStrip),
                        unsigned((a.rows + kReachRows - 1) / kReachRows));
        hipLaunchKernelGGL(reach_scale_from_kernel, grid, dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_reach_pview(const ReachPviewArgs &a, bool to, hipStream_t st) {
    if (a.rows <= 0 || a.view <= 0) return hipSuccess;
    if (a.row0 < 0 || int64_t(a.row0) + a.rows > a.c.n) return hipErrorInvalidValue;
    const dim3 grid(unsigned((a.rows + 255) / 256));
    if (to) hipLaunchKernelGGL(reach_pview_to_kernel, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(reach_pview_from_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
