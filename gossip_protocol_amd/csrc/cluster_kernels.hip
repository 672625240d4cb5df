// gossip_protocol_amd/csrc/cluster_kernels.hip -- the overlay clustering kernels
// (cluster_kernels.hpp): the member pass, the link pass and the mutual pass of both tables.
#include "cluster_kernels.hpp"
#include "reach_row.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ void or_into(uint64_t *p, uint64_t bits) {
    atomicOr(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(bits));
}

// counter `field` of observer b, in the copy that `item` (any index of the work item) selects
__device__ __forceinline__ unsigned long long *ctr_at(const ClusterCommon &c, uint32_t item, int field, int b) {
    return c.ctr + (size_t(item % uint32_t(kClusterSlots)) * kClusterCounters + size_t(field)) * kClusterMax + b;
}

__device__ __forceinline__ bool alive_bit(const uint8_t *alive, uint32_t x) {
    return (uint32_t(alive[x >> 3]) >> (x & 7u)) & 1u;
}

// the alive byte of a lane's 8 columns as four packed 0 / 1 words (the audit's form)
__device__ __forceinline__ void alive_words(uint32_t ab, uint32_t (&al)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) al[i] = ((ab >> (2 * i)) & 1u) | (((ab >> (2 * i + 1)) & 1u) << 16);
}

// ---- full view -------------------------------------------------------------------------------
// Member pass: one wave per (observer, 512-column strip) of the observer's own row, where this
// shard holds it.  A lane's 8 present-and-fresh flags are masked by the alive byte of its 8
// columns (0 from n on: stride padding is never an edge), every flag left is one atomicOr of bit
// b, and the wave's count goes into degree[b].
__global__ void __launch_bounds__(256) cluster_scale_member_kernel(ClusterScaleArgs a, int32_t strips) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int b = int(blockIdx.y);
    if (!((a.c.want >> b) & 1ull)) return;
    const int64_t lr = int64_t(a.c.obs[b]) - a.row0;
    if (lr < 0 || lr >= a.rows) return;                          // another shard's row
    const int32_t s = int32_t(blockIdx.x) * 4 + wave;
    if (s >= strips) return;                                     // wave-uniform
    const int64_t c0 = int64_t(s) * kReachStrip;
    const int64_t gc0 = int64_t(a.col0) + c0;                    // a multiple of 512

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    const uint32_t ab = a.c.alive[gc0 / 8 + lane];
    const uint4 v = ld16<false>(a.table + lr * a.stride + c0 + lane * kEntriesPerLane);
    const uint32_t f[4] = {reach_fresh(v.x, t5x2, lim), reach_fresh(v.y, t5x2, lim),
                           reach_fresh(v.z, t5x2, lim), reach_fresh(v.w, t5x2, lim)};
    uint32_t bits = reach_pack(f) & ab;
    const uint32_t total = wave_sum32(uint32_t(__builtin_popcount(bits)));
    uint64_t *m = a.c.member + gc0 + lane * kEntriesPerLane;     // an alive column is below n
    while (bits) {
        const int q = __builtin_ctz(bits);
        bits &= bits - 1;
        or_into(m + q, 1ull << b);
    }
    if (lane == 0 && total) atomicAdd(ctr_at(a.c, uint32_t(s), kCluDegree, b), (unsigned long long)total);
}

// popcount of the two validity words of packed flag word f against the transposed member words
// of the same two entries: bit l of a validity word is lane l's entry
__device__ __forceinline__ uint32_t link_count(uint32_t f, uint64_t m0, uint64_t m1) {
    const uint64_t v0 = __ballot((f & 0xFFFFu) != 0u), v1 = __ballot((f >> 16) != 0u);
    return uint32_t(__builtin_popcountll(v0 & m0)) + uint32_t(__builtin_popcountll(v1 & m1));
}

// one row's lane vector: the entries that are edges (present, fresh, alive column) as eight
// ballots, each against the lane's -- i.e. the observer's -- member word of that entry
__device__ __forceinline__ uint32_t link_row(const uint4 &v, const uint32_t (&al)[4], const uint64_t (&M)[8],
                                             uint32_t t5x2, uint32_t lim) {
    uint32_t c = link_count(reach_fresh(v.x, t5x2, lim) & al[0], M[0], M[1]);
    c += link_count(reach_fresh(v.y, t5x2, lim) & al[1], M[2], M[3]);
    c += link_count(reach_fresh(v.z, t5x2, lim) & al[2], M[4], M[5]);
    c += link_count(reach_fresh(v.w, t5x2, lim) & al[3], M[6], M[7]);
    return c;
}

// Link pass: reach_multi_scale_from's work item, a 512-column strip x a block of 256 rows, a
// wave taking every fourth row.  Lane b is observer b.  The strip's member words are kept
// transposed: per entry q of a lane vector one 64-bit word per observer, whose bit l says that
// column gc0 + 8 l + q is in N(observers[b]) -- the bit order of a ballot over "entry q of my
// vector is an edge".  The four waves transpose two entries each by ballots into 4 KiB of LDS,
// and every lane then holds its observer's eight words in registers for the whole block.  A row
// u is loaded only if member[u] != 0 (one coalesced read and one ballot select the wave's rows);
// lane b adds the eight popcounts where bit b of member[u] is set.  At the end one 64-bit
// atomicAdd per lane and wave with a non-zero sum.
__global__ void __launch_bounds__(256) cluster_scale_links_kernel(ClusterScaleArgs a) {
    __shared__ uint64_t s_m[kEntriesPerLane][64];
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kReachRows;
    const int64_t c0 = int64_t(blockIdx.x) * kReachStrip;
    const int64_t gc0 = int64_t(a.col0) + c0;                    // a multiple of 512

    const int32_t lr = rb + wave + 4 * lane;                     // the wave's lane-th row
    const uint64_t mw = lr < a.rows ? a.c.member[a.row0 + lr] : 0ull;
    uint64_t rows = __ballot(mw != 0ull);

    const uint64_t *mcol = a.c.member + gc0 + lane * kEntriesPerLane;   // inside cluster_nodes(n)
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
        const int q = wave * 2 + qq;
        const uint64_t m = mcol[q];
        const uint32_t lo = uint32_t(m), hi = uint32_t(m >> 32);
        uint64_t mine = 0;
        if (__ballot(m != 0ull)) {                               // wave-uniform
#pragma unroll 2
            for (int b = 0; b < 32; ++b) {
                const uint64_t w0 = __ballot(((lo >> b) & 1u) != 0u), w1 = __ballot(((hi >> b) & 1u) != 0u);
                if (lane == b) mine = w0;
                if (lane == b + 32) mine = w1;
            }
        }
        s_m[q][lane] = mine;
    }
    __syncthreads();
    if (!rows) return;
    uint64_t M[kEntriesPerLane];
    uint64_t any = 0;
#pragma unroll
    for (int q = 0; q < kEntriesPerLane; ++q) {
        M[q] = s_m[q][lane];
        any |= M[q];
    }
    if (__ballot(any != 0ull) == 0ull) return;                   // no column of the strip is listed

    const uint32_t t5 = uint32_t(a.c.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t lim = uint32_t(a.c.age_limit) | (uint32_t(a.c.age_limit) << 16);
    uint32_t al[4];
    alive_words(a.c.alive[gc0 / 8 + lane], al);
    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    uint32_t acc = 0;                                            // <= 64 rows x 512 columns
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
        for (int q = 0; q < 4; ++q) {
            const uint32_t sel = uint32_t(lane_of(mw, js[q]) >> lane) & 1u;
            acc += link_row(v[q], al, M, t5x2, lim) * sel;
        }
    }
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const uint32_t sel = uint32_t(lane_of(mw, j) >> lane) & 1u;
        acc += link_row(ld16<true>(base + j * step), al, M, t5x2, lim) * sel;
    }
    const uint32_t item = (blockIdx.y * gridDim.x + blockIdx.x) * 4u + uint32_t(wave);
    if (acc) atomicAdd(ctr_at(a.c, item, kCluLinks, lane), (unsigned long long)acc);
}

// Mutual pass: per observer b whose column this shard holds, one thread per row u; a row with
// bit b of member[u] reads its one entry for the observer.  The wave's count by one ballot.
__global__ void __launch_bounds__(256) cluster_scale_mutual_kernel(ClusterScaleArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int b = int(blockIdx.y);
    if (!((a.c.want >> b) & 1ull)) return;
    const int64_t lc = int64_t(a.c.obs[b]) - a.col0;
    if (lc < 0 || lc >= a.stride) return;                        // another tile's column
    const int32_t lr = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    bool hit = false;
    if (lr < a.rows && ((a.c.member[a.row0 + lr] >> b) & 1ull)) {
        const uint32_t e = a.table[int64_t(lr) * a.stride + lc];
        hit = e != 0u && ((uint32_t(a.c.tick) - e) & 31u) < uint32_t(a.c.age_limit);
    }
    const uint32_t c = uint32_t(__builtin_popcountll(__ballot(hit)));
    if (lane == 0 && c) atomicAdd(ctr_at(a.c, blockIdx.x, kCluMutual, b), (unsigned long long)c);
}

// ---- partial view ----------------------------------------------------------------------------
// Member pass: one wave per observer whose row this shard holds, 64 slots at a time below len.
__global__ void __launch_bounds__(64) cluster_pview_member_kernel(ClusterPviewArgs a) {
    const int lane = int(threadIdx.x);
    const int b = int(blockIdx.x);
    if (!((a.c.want >> b) & 1ull)) return;
    const int64_t lr = int64_t(a.c.obs[b]) - a.row0;
    if (lr < 0 || lr >= a.rows) return;                          // another shard's row
    const int32_t len = a.len[lr] < a.view ? a.len[lr] : a.view;
    const uint64_t *view = a.table + lr * a.view;
    uint32_t total = 0;
    for (int32_t s0 = 0; s0 < len; s0 += 64) {
        uint32_t id;
        const bool edge = s0 + lane < len && reach_entry_at(view[s0 + lane], a.c.n, a.c.tick, a.c.age_limit, id) &&
                          alive_bit(a.c.alive, id);
        if (edge) or_into(&a.c.member[id], 1ull << b);
        total += uint32_t(__builtin_popcountll(__ballot(edge)));
    }
    if (lane == 0 && total) atomicAdd(ctr_at(a.c, 0u, kCluDegree, b), (unsigned long long)total);
}

// Link and mutual pass: a wave takes 64 consecutive rows, tests their member words with one
// coalesced read and one ballot, and walks only the listed rows (at most 64 x view of them in
// the whole table).  Per fresh entry u -> v the lane gathers member[v]; a set bit there says v is
// alive, so no alive lookup is needed.  For each set bit b of the wave-uniform member[u] (usually
// one to three) one ballot counts the entries with bit b in member[v] and one the entry that is
// observers[b] itself, and lane b keeps both sums.
__global__ void __launch_bounds__(256) cluster_pview_links_kernel(ClusterPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t base = (int32_t(blockIdx.x) * 4 + wave) * 64;
    const int32_t lr = base + lane;
    const uint64_t mw = lr < a.rows ? a.c.member[a.row0 + lr] : 0ull;
    uint64_t rows = __ballot(mw != 0ull);
    if (!rows) return;
    const uint32_t my_obs = lane < a.c.n_observers ? uint32_t(a.c.obs[lane]) : ~0u;
    uint32_t links = 0, mutual = 0;                              // <= 64 rows x view each
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1;
        const int32_t row = base + j;
        const uint64_t mu = lane_of(mw, j);
        const int32_t len = a.len[row] < a.view ? a.len[row] : a.view;
        const uint64_t *view = a.table + int64_t(row) * a.view;
        for (int32_t s0 = 0; s0 < len; s0 += 64) {
            uint32_t id = ~0u;
            const bool edge = s0 + lane < len && reach_entry_at(view[s0 + lane], a.c.n, a.c.tick, a.c.age_limit, id);
            const uint64_t w = edge ? mu & a.c.member[id] : 0ull;
            uint64_t left = mu;
            while (left) {                                       // wave-uniform
                const int b = __builtin_ctzll(left);
                left &= left - 1;
                const uint32_t cl = uint32_t(__builtin_popcountll(__ballot(((w >> b) & 1ull) != 0ull)));
                const uint32_t cm = uint32_t(__builtin_popcountll(__ballot(edge && id == lane_of(my_obs, b))));
                if (lane == b) {
                    links += cl;
                    mutual += cm;
                }
            }
        }
    }
    const uint32_t item = blockIdx.x * 4u + uint32_t(wave);
    if (links) atomicAdd(ctr_at(a.c, item, kCluLinks, lane), (unsigned long long)links);
    if (mutual) atomicAdd(ctr_at(a.c, item, kCluMutual, lane), (unsigned long long)mutual);
}

}  // namespace

hipError_t launch_cluster_scale(const ClusterScaleArgs &a, int phase, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.c.n) - a.col0 ? a.stride : int64_t(a.c.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kReachStrip || a.col0 % kReachStrip || a.col0 < 0 || a.row0 < 0 ||
        int64_t(a.row0) + a.rows > a.c.n || a.c.n_observers < 1 || a.c.n_observers > kClusterMax)
        return hipErrorInvalidValue;
    const int32_t strips = int32_t((cols + kReachStrip - 1) / kReachStrip);
    const unsigned k = unsigned(a.c.n_observers);
    if (phase == kClusterMembers) {
        hipLaunchKernelGGL(cluster_scale_member_kernel, dim3(unsigned((strips + 3) / 4), k), dim3(256), 0, st, a,
                           strips);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(cluster_scale_links_kernel, dim3(unsigned(strips), unsigned((a.rows + kReachRows - 1) / kReachRows)),
                       dim3(256), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cluster_scale_mutual_kernel, dim3(unsigned((a.rows + 255) / 256), k), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cluster_pview(const ClusterPviewArgs &a, int phase, hipStream_t st) {
    if (a.rows <= 0 || a.view <= 0) return hipSuccess;
    if (a.row0 < 0 || int64_t(a.row0) + a.rows > a.c.n || a.c.n_observers < 1 || a.c.n_observers > kClusterMax)
        return hipErrorInvalidValue;
    if (phase == kClusterMembers)
        hipLaunchKernelGGL(cluster_pview_member_kernel, dim3(unsigned(a.c.n_observers)), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(cluster_pview_links_kernel, dim3(unsigned((a.rows + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
