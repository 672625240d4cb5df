// gossip_protocol_amd/csrc/scale_row.hpp -- the full-view protocol tick of one 16-byte lane
// vector (8 packed entries, hb << 5 | ts5, 0 = absent), one function per step.  Device-only:
// included by scale_kernels.hip, whose three row forms (the workgroup-per-row chunk loop, the
// long-segment premerge, the sub-slab sweep) are sequences of these calls.  A protocol step is
// written here once and every row form that has the step calls it; the MP1Node.cpp rule a step
// encodes is cited on its function and nowhere else.
#pragma once
#include "join_kernels.hpp"
#include "scale_kernels.hpp"
#include "wave_ops.hpp"

namespace gsp {

__device__ inline uint64_t event_mix(uint32_t kind, uint32_t t, uint32_t r, uint32_t x) {
    uint64_t z = (uint64_t(kind) << 62) | (uint64_t(t & 0xFFFFF) << 42) |
                 (uint64_t(r & 0x1FFFFF) << 21) | uint64_t(x & 0x1FFFFF);
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- scalar form: one entry at a time ---------------------------------------------------
// Merge one payload entry v (the sender's) into the receiver's entry e (MP1Node::recvCallBack,
// GOSSIP branch):
//   present: max-merge, ts = now only on a strict heartbeat increase (MP1Node.cpp:247-251)
//   absent:  copy v when v is present and fresh, t - ts_v < TREMOVE (MP1Node.cpp:294)
__device__ inline uint32_t merge_entry(uint32_t e, uint32_t v, uint32_t t5, uint32_t tr) {
    const uint32_t he = e >> 5, hv = v >> 5;
    const uint32_t upd = (hv > he) ? ((v & 0xFFE0u) | t5) : e;
    const uint32_t fresh = ((t5 - v) & 31u) < tr;
    const uint32_t add = (v != 0u && fresh) ? v : 0u;
    return e ? upd : add;
}

__device__ inline uint32_t merge_word_scalar(uint32_t e, uint32_t v, uint32_t t5, uint32_t tr) {
    const uint32_t lo = merge_entry(e & 0xFFFFu, v & 0xFFFFu, t5, tr);
    const uint32_t hi = merge_entry(e >> 16, v >> 16, t5, tr);
    return lo | (hi << 16);
}

// ---- packed form: two entries per 32-bit word on the v_pk_*_u16 ALUs --------------------
// hipcc folds min(sub_sat(a, b), 1) back into compares + selects, so the packed ops are
// spelled out; every operand is a VGPR and nothing reads EXEC or the memory counters.
__device__ inline uint32_t pk_max(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ inline uint32_t pk_min(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ inline uint32_t pk_sub(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_sub_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ inline uint32_t pk_subc(uint32_t a, uint32_t b) {   // saturating at 0
    uint32_t r; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ inline uint32_t pk_mad(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r; asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
__device__ inline uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) {   // (m & a) | (~m & b)
    uint32_t r; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b)); return r;
}

struct PackedConsts {
    uint32_t one, t5x2, t32, tr, trm1, low5, hbmask, zero;
};

__device__ inline PackedConsts packed_consts(uint32_t t5, uint32_t tr) {
    PackedConsts c;
    c.one = 0x00010001u;
    c.t5x2 = t5 | (t5 << 16);
    c.t32 = c.t5x2 + 0x00200020u;
    c.tr = tr | (tr << 16);
    c.trm1 = (tr - 1) | ((tr - 1) << 16);
    c.low5 = 0x001F001Fu;
    c.hbmask = 0xFFE0FFE0u;
    c.zero = 0u;
    return c;
}

// Same function as merge_word_scalar; tests/test_param_edges_gpu.py runs both forms against the
// CPU oracle at the ends of the ranges (hb 2040..2047 and across 1023 -> 1024, tr 1, and tr 31
// over two wraps of ts5; the workloads are tests/param_edges.py's):
//   present e:  m = max(v & hbmask, e); e' = m + (m != e) * t5
//   absent e:   e' = v if v present and (t5 + 32 - ts5(v)) mod 32 < tr, else 0
__device__ inline uint32_t merge_word_packed(uint32_t e, uint32_t v, const PackedConsts &c) {
    const uint32_t m = pk_max(v & c.hbmask, e);
    const uint32_t rp = pk_mad(pk_min(pk_sub(m, e), c.one), c.t5x2, m);
    const uint32_t age = (c.t32 - (v & c.low5)) & c.low5;
    const uint32_t ok = pk_min(pk_subc(c.tr, age), pk_min(v, c.one));
    const uint32_t ra = v & pk_sub(c.zero, ok);
    return bfi(pk_sub(c.zero, pk_min(e, c.one)), rp, ra);
}

// Replace entry i (runtime, 0..7) of a 16-B lane vector.  Only ever reached on the one
// lane whose chunk holds the sender's or the receiver's own column, so the compare-select
// chain (which keeps every index compile-time: no scratch) costs nothing in the stream.
template <typename F>
__device__ inline void patch16(uint4 &w, int i, F f) {
    uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < kEntriesPerLane; ++q) {
        const int sh = (q & 1) * 16;
        const uint32_t old = (ws[q >> 1] >> sh) & 0xFFFFu;
        const uint32_t nv = f(old) & 0xFFFFu;
        if (q == i) ws[q >> 1] = (ws[q >> 1] & ~(0xFFFFu << sh)) | (nv << sh);
    }
    w = make_uint4(ws[0], ws[1], ws[2], ws[3]);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 16-byte row accesses; kNT selects the non-temporal (streaming) cache policy.  It must be
// a compile-time choice: a runtime select between the two forms is CSE'd into one plain load.
template <bool kNT>
__device__ inline uint4 ld16(const uint16_t *p) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    u32x4 v;
    if constexpr (kNT) v = __builtin_nontemporal_load(q);
    else v = *q;
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <bool kNT>
__device__ inline void st16(uint16_t *p, const uint32_t (&w)[4]) {
    u32x4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    if constexpr (kNT) __builtin_nontemporal_store(v, q);
    else *q = v;
}

// ---- the steps of one lane vector, in tick order: gc0 is the global column of the vector's
// entry 0, r the receiver, t the tick (t5 = t mod 32)

// The CSR slot of the message at CSR position i from sender sj: a local row index, or (row
// exchange, recorded beside the sender) -1 - (index into the rows it received); and the sender's
// previous-tick row from the slot (local_row: without a row exchange there is no other kind).
__device__ __forceinline__ int32_t sender_slot(const ScaleTickArgs &a, int32_t i, int32_t sj) {
    return a.csr_slot ? a.csr_slot[i] : sj - a.row0;
}
__device__ __forceinline__ const uint16_t *local_row(const ScaleTickArgs &a, int32_t slot) {
    return a.prev + int64_t(slot) * a.stride;
}
__device__ __forceinline__ const uint16_t *sender_row(const ScaleTickArgs &a, int32_t slot) {
    return slot >= 0 ? local_row(a, slot) : a.remote + int64_t(-slot - 1) * a.stride;
}

// TFAIL: drop the payload entries the sender had suspected when it sent, t - 1 - ts >= tfail
// (tfx2: tfail in both halves; t32m1: (t - 1) mod 32 in both halves, + 32)
__device__ __forceinline__ void gossiped_vec(uint4 &v, const PackedConsts &pc, uint32_t tfx2, uint32_t t32m1) {
    auto gossiped = [&](uint32_t w) -> uint32_t {
        const uint32_t age = (t32m1 - (w & pc.low5)) & pc.low5;
        return w & pk_sub(pc.zero, pk_min(pk_subc(tfx2, age), pc.one));
    };
    v = make_uint4(gossiped(v.x), gossiped(v.y), gossiped(v.z), gossiped(v.w));
}

// One sender vector v merged into the receiver's e (merge_entry on each of the 8 entries)
template <int kMerge>
__device__ __forceinline__ void merge_vec(uint4 &e, const uint4 &v, const PackedConsts &pc, uint32_t t5, uint32_t tr) {
    auto word = [&](uint32_t ew, uint32_t vw) -> uint32_t {
        if constexpr (kMerge == 1) return merge_word_packed(ew, vw, pc);
        else return merge_word_scalar(ew, vw, t5, tr);
    };
    e = make_uint4(word(e.x, v.x), word(e.y, v.y), word(e.z, v.z), word(e.w, v.w));
}

// The sender's own entry: hb + 1 and ts = now, or add (1, now) (MP1Node.cpp:237-243); the
// sender's row never holds itself, so this follows the merge of its vector
__device__ __forceinline__ void bump_sender(uint4 &e, int32_t sender, int64_t gc0, uint32_t t5) {
    const int64_t ds = int64_t(sender) - gc0;
    if (ds >= 0 && ds < kEntriesPerLane)
        patch16(e, int(ds), [t5](uint32_t old) { return (((old >> 5) + 1u) << 5) | t5; });
}

// The JOINREP: the introducer's (node 0's) sender entry (MP1Node.cpp:237-243), then the njc
// members it chose (join_kernels.hpp), column jc[q] with entry jv[q]
__device__ __forceinline__ void merge_joinrep(uint4 &e, int64_t gc0, int32_t njc, const int32_t *jc,
                                              const uint32_t *jv, uint32_t t5, uint32_t tr) {
    const int64_t d0 = -gc0;
    if (d0 >= 0 && d0 < kEntriesPerLane)
        patch16(e, int(d0), [t5](uint32_t old) { return old ? ((((old >> 5) + 1u) << 5) | t5)
                                                            : ((1u << 5) | t5); });
    for (int32_t q = 0; q < njc; ++q) {
        const int64_t dq = int64_t(jc[q]) - gc0;
        const uint32_t v = jv[q];
        if (dq >= 0 && dq < kEntriesPerLane)
            patch16(e, int(dq), [v, t5, tr](uint32_t old) { return merge_entry(old, v, t5, tr); });
    }
}

// Merges a JOINREP counts in the digest: its sender entry and the min(intro_list, cnt0)
// members it carries
__device__ __forceinline__ unsigned long long joinrep_merges(const ScaleTickArgs &a) {
    const int32_t c0 = a.cnt_prev[0];
    return 1ull + uint64_t(a.intro_list < c0 ? a.intro_list : c0);
}

// Never list yourself (MP1Node.cpp:290): the own column is cleared after the merges
__device__ __forceinline__ void clear_own(uint4 &e, int32_t r, int64_t gc0) {
    const int64_t dr = int64_t(r) - gc0;
    if (dr >= 0 && dr < kEntriesPerLane) patch16(e, int(dr), [](uint32_t) { return 0u; });
}

// Packed screen of the merged vector ws against the vector before the tick w0: true when an
// entry is stale (TREMOVE) or new, i.e. scan_entries has something to do; otherwise `bits` are
// the presence bits (kTfail: of the unsuspected entries, tfx2 = tfail in both halves).
template <bool kTfail>
__device__ __forceinline__ bool screen_vec(const uint32_t (&ws)[4], const uint32_t (&w0)[4], const PackedConsts &pc,
                                           uint32_t tfx2, uint32_t &bits) {
    uint32_t ev = 0;
    bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t pe = pk_min(ws[i], pc.one);
        const uint32_t age = (pc.t32 - (ws[i] & pc.low5)) & pc.low5;
        ev |= pk_min(pk_subc(age, pc.trm1), pe);          // present and stale
        ev |= pk_subc(pe, pk_min(w0[i], pc.one));          // absent before, present now
        const uint32_t pg = kTfail ? pk_min(pe, pk_min(pk_subc(tfx2, age), pc.one)) : pe;
        bits |= ((pg | (pg >> 15)) & 3u) << (2 * i);
    }
    return ev != 0;
}

// The per-entry pass (MP1Node::nodeLoopOps): the TREMOVE scan removes an entry with t - ts >=
// TREMOVE (MP1Node.cpp:340); an entry absent before the tick and present after it is a join.
// Both are counted, hashed into the order-independent digest and flagged in evr / evj (bit i =
// entry i; outputs) for the event stream.  Returns the presence bits: the entries left (kTfail:
// and not suspected, t - ts < tf).  kInit: no scan and no events, the presence bits only.
// (The flags are gathered in locals: or-ed through the references they end up in scratch.)
template <bool kInit, bool kTfail>
__device__ __forceinline__ uint32_t scan_entries(uint32_t (&ws)[4], const uint32_t (&w0)[4], int32_t t, int32_t r,
                                                 int64_t gc0, uint32_t tr, uint32_t tf, uint32_t &joins,
                                                 uint32_t &removes, uint64_t &hsum, uint32_t &evj, uint32_t &evr) {
    const uint32_t t5 = uint32_t(t) & 31u;
    uint32_t bits = 0, fj = 0, fr = 0;
#pragma unroll
    for (int i = 0; i < kEntriesPerLane; ++i) {
        const int sh = (i & 1) * 16;
        uint32_t ent = (ws[i >> 1] >> sh) & 0xFFFFu;
        if (!kInit && ent) {
            const uint32_t before = (w0[i >> 1] >> sh) & 0xFFFFu;
            if (((t5 - ent) & 31u) >= tr) {
                removes++;
                hsum += event_mix(2, uint32_t(t), uint32_t(r), uint32_t(gc0 + i));
                ws[i >> 1] &= ~(0xFFFFu << sh);
                ent = 0;
                fr |= 1u << i;
            } else if (!before) {
                joins++;
                hsum += event_mix(1, uint32_t(t), uint32_t(r), uint32_t(gc0 + i));
                fj |= 1u << i;
            }
        }
        const bool counted = ent && (!kTfail || ((t5 - ent) & 31u) < tf);
        bits |= (counted ? 1u : 0u) << i;
    }
    evj = fj;
    evr = fr;
    return bits;
}

// ---- the event stream: a wave stages its records as kind << 30 | column in LDS (s_ev) and
// moves them to the ring in runs, one reservation (ev_reserve) and one flush (ev_flush) per run
// Stage the join / remove records of one vector (evj / evr of scan_entries, the kinds the ring
// records) behind the wave's `fill` staged records; returns the new fill.  room(fill, total) is
// called, wave-uniformly, before `total` records are written and returns the fill to write
// them at (a form whose stage can overflow flushes it there and returns 0).
template <typename F>
__device__ __forceinline__ uint32_t ev_stage(uint32_t *s_ev, uint32_t fill, uint32_t evj, uint32_t evr,
                                             uint32_t kinds, int64_t gc0, F room) {
    uint32_t both = ((kinds & GSP_EVENTS_JOIN) ? evj : 0u) | ((kinds & GSP_EVENTS_REMOVE) ? (evr << 8) : 0u);
    const uint32_t cnt = uint32_t(__builtin_popcount(both));
    if (!__ballot(cnt > 0)) return fill;          // wave-uniform
    const uint32_t incl = wave_incl_scan(cnt);
    const uint32_t total = lane_of(incl, 63);
    fill = room(fill, total);
    uint32_t p = fill + incl - cnt;
    while (both) {
        const uint32_t b = uint32_t(__builtin_ffs(both) - 1);
        both &= both - 1;
        s_ev[p++] = ((b < 8 ? 1u : 2u) << 30) | uint32_t(gc0 + (b & 7u));
    }
    return fill + total;
}

// Reserve `fill` (wave-uniform: the readfirstlane says so, which keeps the add one atomic of a
// scalar value, not a loop over the lanes) ring records by lane 0; every lane gets the base
__device__ __forceinline__ unsigned long long ev_reserve(unsigned long long *ev_count, uint32_t fill, int32_t lane) {
    unsigned long long base = 0;
    fill = uint32_t(__builtin_amdgcn_readfirstlane(int(fill)));
    if (lane == 0) base = atomicAdd(ev_count, (unsigned long long)fill);
    return lane_of(uint64_t(base), 0);
}

// The wave's `fill` staged records of row r, tick t -> ring records [base, base + fill), those
// below the ring's capacity
__device__ __forceinline__ void ev_flush(unsigned long long *ev_buf, const uint32_t *s_ev, uint32_t fill,
                                         unsigned long long base, int64_t cap, int32_t t, int32_t r, int32_t lane) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = uint32_t(lane); i < fill; i += 64) {
        const uint32_t s = s_ev[i];
        if (int64_t(base + i) < cap)
            ev_buf[base + i] = event_record(s >> 30, uint32_t(t), uint32_t(r), s & 0x3FFFFFFFu);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Tile g's args of this tick from the tile table (scale_kernels.hpp): its template of the tick's
// parity with the tick's own values patched in.  The one list of per-tick fields on the device:
// the sweep and the long kernel both build their args here.
// A pointer read from memory is a generic one to the compiler, unlike a kernel argument, and
// generic accesses (flat_*) count on both memory counters: every wait for an LDS permute would
// also wait for the row vectors in flight.  The table's pointers are all device memory.
template <typename T>
__device__ __forceinline__ void to_global(T *&p) {
    p = (T *)(__attribute__((address_space(1))) T *)(uintptr_t)p;     // (through an integer: a cast pair folds away)
}

__device__ __forceinline__ ScaleTickArgs tile_args(const ScaleTickArgs *tpl, int32_t g, const ScaleTickVals &tv) {
    ScaleTickArgs a = tpl[2 * g + (tv.tick & 1)];
    a.tick = tv.tick;
    a.drop_pct = tv.drop_pct;
    a.drop_prev = tv.drop_prev;
    a.dig += size_t(tv.tick) * kDigSlots * kDigFields;
    to_global(a.prev); to_global(a.cur); to_global(a.remote); to_global(a.fail_tick);
    to_global(a.start_tick); to_global(a.intro); to_global(a.intro_cnt); to_global(a.own_hb);
    to_global(a.cnt_prev); to_global(a.cnt_cur); to_global(a.off); to_global(a.csr_src);
    to_global(a.csr_slot); to_global(a.out_dst); to_global(a.deg); to_global(a.ping);
    to_global(a.bitmap); to_global(a.dig); to_global(a.ev.buf); to_global(a.ev.count);
    to_global(a.err); to_global(a.long_list); to_global(a.cnt_sub); to_global(a.mid_list);
    return a;
}

// Append row lr to a deferred-row list (list[0]: its length), by one lane of the CSR's owner
__device__ __forceinline__ void defer_row(int32_t *list, int32_t lr) {
    if (list) list[1 + atomicAdd(&list[0], 1)] = lr;
}

}  // namespace gsp
