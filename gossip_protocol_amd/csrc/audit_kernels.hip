// gossip_protocol_amd/csrc/audit_kernels.hip -- the view audit kernels (audit_kernels.hpp).
#include "audit_kernels.hpp"
#include "scale_row.hpp"

namespace gsp {
namespace {

__device__ __forceinline__ bool audit_alive(const int32_t *start_tick, const int32_t *fail_tick,
                                            int32_t r, int32_t t) {
    return (start_tick ? start_tick[r] : 0) <= t && t <= fail_tick[r];
}

// ---- the truth of the call: one thread per 8 members writes their alive byte and fingerprints
__global__ void __launch_bounds__(256) audit_truth_kernel(AuditTruthArgs a) {
    const int32_t b = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    const int32_t x0 = b * 8;
    if (x0 >= a.n) return;
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int32_t x = x0 + k;
        if (x >= a.n) break;
        bits |= (audit_alive(a.start_tick, a.fail_tick, x, a.tick) ? 1u : 0u) << k;
        if (a.fp) a.fp[x] = audit_fp(uint32_t(x));
    }
    a.alive[b] = uint8_t(bits);
}

// The per-lane partial sums of one row, and the wave's totals after audit_reduce.  size, live,
// suspect and age_sum are packed 16-bit while they are added up (two columns per dword): a lane
// adds at most 16 entries per half and row, and a wave's totals stay below 2^16 (2,048 entries of
// age <= 31).
struct AuditAcc {
    uint32_t size = 0, live = 0, suspect = 0, age_sum = 0, age_max = 0;
    uint64_t print = 0;
};

__device__ __forceinline__ uint32_t fold16(uint32_t x) { return (x & 0xFFFFu) + (x >> 16); }

// One wave reduction per row: two packed sums, one maximum, one 64-bit sum
__device__ __forceinline__ void audit_reduce(AuditAcc &c) {
    const uint32_t a = wave_sum32(c.size | (c.live << 16));
    const uint32_t b = wave_sum32(c.suspect | (c.age_sum << 16));
    c.age_max = wave_max32(c.age_max);
    c.print = wave_sum64(c.print);
    c.size = a & 0xFFFFu;
    c.live = a >> 16;
    c.suspect = b & 0xFFFFu;
    c.age_sum = b >> 16;
}

// ---- full view: a row reduction over rows x stride packed u16 entries -----------------------
// Work item = (kAuditStrips strips of 512 columns, block of 256 rows), the census' work item
// turned on its side.  A wave takes every fourth row of the block; the alive test of a row is
// wave-uniform (one ballot over the wave's 64 rows) and a dead row is never loaded.  For the
// whole block a lane keeps, per strip, the truth of its 8 columns in registers: the alive bits
// as four packed 0/1 words and the 8 fingerprints.  A row's strips are loaded together, each as
// one 1-KiB non-temporal instruction (16 B per lane), one row ahead of the arithmetic, so the
// loads of the next row are in flight while this one is added up.  Per row the wave does one
// reduction and issues integer atomics into the n-length arrays, the four sums as one
// instruction.
struct AuditStripTruth {
    uint32_t al[4];                  // alive, 0 / 1 in both halves of word i
    uint64_t fp[kEntriesPerLane];
};

__device__ __forceinline__ void audit_add(AuditAcc &c, const uint32_t (&w)[4], const AuditStripTruth &tr,
                                          uint32_t t5x2, uint32_t limm1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t pe = pk_min(w[i], 0x00010001u);                 // present: e != 0
        const uint32_t pa = pe & tr.al[i];                              // ... of an alive member
        const uint32_t age = pk_sub(t5x2, w[i]) & 0x001F001Fu;          // (T - ts) mod 32
        const uint32_t agea = age & pk_sub(0u, pa);
        c.size += pe;
        c.live += pa;
        c.suspect += pk_min(pk_subc(agea, limm1), 0x00010001u);         // age >= age_limit
        c.age_sum += agea;
        c.age_max = pk_max(c.age_max, agea);
        c.print += (w[i] & 0xFFFFu) ? tr.fp[2 * i] : 0ull;
        c.print += (w[i] >> 16) ? tr.fp[2 * i + 1] : 0ull;
    }
}

__global__ void __launch_bounds__(256) audit_scale_kernel(AuditScaleArgs a, int64_t cols) {
    const int lane = int(threadIdx.x) & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int32_t rb = int32_t(blockIdx.y) * kAuditRows;
    const int64_t c0 = int64_t(blockIdx.x) * (kAuditStrips * kAuditStrip);
    const uint32_t t5 = uint32_t(a.tick) & 31u;
    const uint32_t t5x2 = t5 | (t5 << 16);
    const uint32_t limm1 = uint32_t(a.age_limit - 1) | (uint32_t(a.age_limit - 1) << 16);

    // lane j: is the wave's j-th row (rb + wave + 4 j) alive at T?
    const int32_t lr = rb + wave + 4 * lane;
    const bool alive = lr < a.rows && audit_alive(a.start_tick, a.fail_tick, a.row0 + lr, a.tick);
    uint64_t live = __ballot(alive);
    if (!live) return;

    // the strips below `cols` (the table's columns < n) are read; the one that holds the edge
    // masks its entries from `cols` on (stride padding is not counted)
    bool act[kAuditStrips];
    AuditStripTruth tr[kAuditStrips];
    uint32_t edge[4] = {~0u, ~0u, ~0u, ~0u};
    int es = -1;
#pragma unroll
    for (int s = 0; s < kAuditStrips; ++s) {
        const int64_t sc = c0 + int64_t(s) * kAuditStrip;             // wave-uniform
        act[s] = sc < cols;
        const int64_t lc = sc + lane * kEntriesPerLane;               // the lane's first local column
        const int64_t gc = int64_t(a.col0) + lc;
        uint32_t ab = 0;
        if (act[s] && lc < cols) ab = a.alive[gc >> 3];               // gc < n, a multiple of 8
#pragma unroll
        for (int i = 0; i < 4; ++i)
            tr[s].al[i] = ((ab >> (2 * i)) & 1u) | (((ab >> (2 * i + 1)) & 1u) << 16);
#pragma unroll
        for (int k = 0; k < kEntriesPerLane; ++k)
            tr[s].fp[k] = (act[s] && lc + k < cols) ? a.fp[gc + k] : 0ull;
        if (act[s] && sc + kAuditStrip > cols) {
            es = s;
            const int64_t nv = cols - lc;                              // valid entries of the lane
#pragma unroll
            for (int i = 0; i < 4; ++i)
                edge[i] = nv >= 2 * i + 2 ? ~0u : nv == 2 * i + 1 ? 0xFFFFu : 0u;
        }
    }

    const uint16_t *base = a.table + int64_t(rb + wave) * a.stride + c0 + lane * kEntriesPerLane;
    const int64_t step = 4 * a.stride;
    auto load = [&](uint4 (&v)[kAuditStrips], int j) {
#pragma unroll
        for (int s = 0; s < kAuditStrips; ++s)
            if (act[s]) v[s] = ld16<true>(base + j * step + s * kAuditStrip);
    };

    uint4 cur[kAuditStrips] = {}, nxt[kAuditStrips] = {};
    int j = __builtin_ctzll(live);
    live &= live - 1;
    load(cur, j);
    for (;;) {
        const bool more = live != 0;
        int jn = 0;
        if (more) {
            jn = __builtin_ctzll(live);
            live &= live - 1;
            load(nxt, jn);
        }
        AuditAcc c;
#pragma unroll
        for (int s = 0; s < kAuditStrips; ++s) {
            if (!act[s]) continue;
            uint32_t w[4] = {cur[s].x, cur[s].y, cur[s].z, cur[s].w};
            if (s == es) {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] &= edge[i];
            }
            audit_add(c, w, tr[s], t5x2, limm1);
        }
        c.size = fold16(c.size);
        c.live = fold16(c.live);
        c.suspect = fold16(c.suspect);
        c.age_sum = fold16(c.age_sum);
        c.age_max = max(c.age_max & 0xFFFFu, c.age_max >> 16);
        audit_reduce(c);
        if (c.size) {                                      // wave-uniform
            const int64_t r = int64_t(a.row0) + rb + wave + 4 * j;
            // lanes 0..3: the four sums, one atomic instruction
            const uint32_t v = lane == kAudSize ? c.size : lane == kAudDead ? c.size - c.live
                             : lane == kAudSuspect ? c.suspect : c.age_sum;
            if (lane < 4 && v) atomicAdd(&a.arr[int64_t(lane) * a.n + r], v);
            if (lane == 0) {
                if (c.age_max) atomicMax(&a.arr[int64_t(kAudAgeMax) * a.n + r], c.age_max);
                atomicAdd(&a.print[r], (unsigned long long)c.print);
            }
        }
        if (!more) break;
        j = jn;
#pragma unroll
        for (int s = 0; s < kAuditStrips; ++s) cur[s] = nxt[s];
    }
}

// ---- partial view: a wave per row of rows x view 64-bit entries ------------------------------
// Lane l takes the slots l, l + 64, ... below len of an alive row (a view of 256 is one 2-KiB
// coalesced read and three more); the alive bit of an id is gathered from the bitmap (128 KiB at
// 1,048,576 nodes), an id >= n (the empty slot's ~0 among them) is dropped before it becomes an
// address, and the fingerprint is computed per entry.  One reduction and plain stores per row:
// a row lives in one shard.
__global__ void __launch_bounds__(256) audit_pview_kernel(AuditPviewArgs a) {
    const int lane = int(threadIdx.x) & 63;
    const int32_t lr = int32_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    if (lr >= a.rows) return;
    const int32_t r = a.row0 + lr;
    if (!audit_alive(a.start_tick, a.fail_tick, r, a.tick)) return;     // wave-uniform
    int32_t len = a.len[lr];
    len = len < a.view ? len : a.view;
    const uint64_t *row = a.table + int64_t(lr) * a.view;
    AuditAcc c;
    for (int32_t slot = lane; slot < len; slot += 64) {
        const uint64_t e = __builtin_nontemporal_load(row + slot);
        const uint32_t id = uint32_t(e >> 32);
        if (id >= uint32_t(a.n)) continue;
        const uint32_t al = (uint32_t(a.alive[id >> 3]) >> (id & 7u)) & 1u;
        const uint32_t age = ((uint32_t(a.tick) - uint32_t(e)) & 31u) * al;
        c.size += 1u;
        c.live += al;
        c.suspect += (al && age >= uint32_t(a.age_limit)) ? 1u : 0u;
        c.age_sum += age;
        c.age_max = max(c.age_max, age);
        c.print += audit_fp(id);
    }
    audit_reduce(c);                                        // view <= 256: the packed sums fit
    if (lane == 0 && c.size) {
        a.arr[int64_t(kAudSize) * a.n + r] = c.size;
        a.arr[int64_t(kAudDead) * a.n + r] = c.size - c.live;
        a.arr[int64_t(kAudSuspect) * a.n + r] = c.suspect;
        a.arr[int64_t(kAudAgeSum) * a.n + r] = c.age_sum;
        a.arr[int64_t(kAudAgeMax) * a.n + r] = c.age_max;
        a.print[r] = (unsigned long long)c.print;
    }
}

}  // namespace

hipError_t launch_audit_truth(const AuditTruthArgs &a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    const int64_t bytes = (int64_t(a.n) + 7) / 8;
    hipLaunchKernelGGL(audit_truth_kernel, dim3(unsigned((bytes + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_audit_scale(const AuditScaleArgs &a, hipStream_t st) {
    const int64_t cols = a.stride < int64_t(a.n) - a.col0 ? a.stride : int64_t(a.n) - a.col0;
    if (cols <= 0 || a.rows <= 0) return hipSuccess;      // a tile wholly in the stride padding
    if (a.stride % kAuditStrip) return hipErrorInvalidValue;
    const int64_t span = int64_t(kAuditStrips) * kAuditStrip;
    const dim3 grid(unsigned((cols + span - 1) / span), unsigned((a.rows + kAuditRows - 1) / kAuditRows));
    hipLaunchKernelGGL(audit_scale_kernel, grid, dim3(256), 0, st, a, cols);
    return hipGetLastError();
}

hipError_t launch_audit_pview(const AuditPviewArgs &a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    if (a.view > 2048) return hipErrorInvalidValue;       // the packed wave sums (audit_reduce)
    hipLaunchKernelGGL(audit_pview_kernel, dim3(unsigned((a.rows + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsp
