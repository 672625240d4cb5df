// gossip_protocol_amd/csrc/scale_kernels.hip -- SCALE-mode HIP kernels for gfx950.
//
// scale_tick_kernel is the per-tick hot path of one receiver row, fused:
//   merge   (MP1Node::recvCallBack GOSSIP branch, MP1Node.cpp:234-256) of every message the
//           row received, in ascending sender order, 8 packed entries per lane per 16-B load;
//   ops     (MP1Node::nodeLoopOps, MP1Node.cpp:335-348): own heartbeat bump, TREMOVE scan;
//   events  join/remove detection, counted and hashed (order-independent digest);
//   send    (one GPU) peer choice by Philox rank-select over the row's presence bitmap in
//           LDS, the drop draw and the destination count for next tick's CSR; (column
//           shards) the slice's presence bitmap and count, resolved after an all-gather by
//           scale_resolve_kernel / scale_finalize_kernel.
// One 256-lane workgroup per row streams the row in 2048-column chunks: it reads its own
// row and each sender's row once (16 B per lane, fully coalesced) and writes its row once,
// so the kernel is HBM-bound at (2 + k) * stride * 2 bytes per row with k messages.
// scale_sweep_kernel runs the same tick of a column tile of the plain protocol one wave per
// (row, 512-column sub-slab), sub-slab by sub-slab, so that the sender re-reads of the previous
// table are served by the Infinity Cache.
// The steps of one lane vector (merge, sender bump, JOINREP, own column, TREMOVE scan, event
// staging and flush, row deferral) are the functions of scale_row.hpp: the row forms here call
// them in tick order and hold no copy of a protocol rule (DESIGN.md "One step, one function").
#include "join_kernels.hpp"
#include "philox.hpp"
#include "scale_row.hpp"

namespace gsp {

namespace {

// rank-th set bit (0-based) of a bitmap of `words` 32-bit words, by one wave; -1 if none.
// lane_cnt / pre: this lane's popcount over its words and the exclusive prefix.
template <typename W>
__device__ inline int32_t wave_select(W word, int32_t per, uint32_t lane_cnt, uint32_t pre,
                                      uint32_t rank, int32_t lane) {
    const bool mine = rank >= pre && rank < pre + lane_cnt;
    int32_t col = -1;
    if (mine) {
        uint32_t m = rank - pre;
        for (int32_t w = 0; w < per; ++w) {
            uint32_t bw = word(lane * per + w);
            const uint32_t pc = __builtin_popcount(bw);
            if (m < pc) {
                for (uint32_t q = 0; q < m; ++q) bw &= bw - 1;
                col = (lane * per + w) * 32 + (__builtin_ffs(bw) - 1);
                break;
            }
            m -= pc;
        }
    }
    const unsigned long long owner = __ballot(mine);
    if (!owner) return -1;
    return int32_t(lane_of(uint32_t(col), __builtin_ffsll(owner) - 1));
}

__device__ inline uint32_t wave_excl_prefix(uint32_t v, uint32_t *total) {
    const uint32_t incl = wave_incl_scan(v);
    *total = lane_of(incl, 63);
    return incl - v;
}

// JOINREP payload (the bounded introducer list, join_kernels.hpp): the B = min(intro_list,
// cnt0) ranks Philox(JOIN; t - 1, 0, r, i) chooses among node 0's cnt0 gossipable members of
// tick t - 1, resolved to this slice's columns by one forward pass of wave 0 over the
// introducer's row (512 columns per step: a ballot-free wave prefix of the step's member
// counts).  Writes the chosen (global column, entry) pairs this slice holds to jc / jv and
// returns their number (wave 0 only; every lane gets the same result).
__device__ inline int32_t join_choose(const ScaleTickArgs &a, int32_t r, int32_t t, int32_t *jc,
                                      uint32_t *jv) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t cnt0 = a.cnt_prev[0];
    const int32_t B = a.intro_list < cnt0 ? a.intro_list : cnt0;
    int32_t ranks[kMaxIntro];
    int32_t nch = 0;
    for (int32_t i = 0; i < B; ++i)
        next_distinct_rank(draw_u31(kDomainJoin, a.seed, uint32_t(t - 1), 0u, uint32_t(r), uint32_t(i)),
                           cnt0, i, ranks, nch);
    int32_t pre = 0, own = cnt0;          // ranks [pre, pre + own) live in this slice
    if (a.intro_cnt) {
        own = a.intro_cnt[int64_t(a.shard) * a.n];
        for (int32_t g = 0; g < a.shard; ++g) pre += a.intro_cnt[int64_t(g) * a.n];
    }
    const uint32_t tf = uint32_t(a.tfail), t5m1 = uint32_t(t - 1) & 31u;
    int32_t q = 0, found = 0;
    while (q < B && ranks[q] < pre) ++q;
    int32_t seen = pre;                   // gossipable members before the current step
    for (int64_t c0 = 0; c0 < a.stride && q < B && ranks[q] < pre + own; c0 += 512) {
        const int64_t c = c0 + int64_t(lane) * 8;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (c < a.stride) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.intro + c);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t ent = (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
            const bool g = ent && (tf == 0 || ((t5m1 - ent) & 31u) < tf);
            bits |= (g ? 1u : 0u) << e;
        }
        const uint32_t cnt = __builtin_popcount(bits);
        const uint32_t incl = wave_incl_scan(cnt);
        const int32_t total = int32_t(lane_of(incl, 63));
        while (q < B && ranks[q] < seen + total) {
            const uint32_t want = uint32_t(ranks[q] - seen);          // rank within the step
            const bool mine = want >= incl - cnt && want < incl;
            const unsigned long long who = __ballot(mine);
            const int32_t l = __builtin_ffsll(who) - 1;
            uint32_t col = 0, val = 0;
            if (mine) {
                uint32_t m = want - (incl - cnt), bb = bits;
                for (uint32_t z = 0; z < m; ++z) bb &= bb - 1;
                const int e = __builtin_ffs(bb) - 1;
                col = uint32_t(c) + uint32_t(e);
                val = (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
            }
            col = lane_of(col, l);
            val = lane_of(val, l);
            if (found < kMaxIntro) {
                jc[found] = int32_t(int64_t(a.col0) + col);
                jv[found] = val;
            }
            found++;
            q++;
        }
        seen += total;
    }
    return found;
}

// A receiver segment longer than the LDS sort holds (k > kMaxSegment, e.g. a join burst on the
// introducer): sorted in place in HBM by the row's workgroup into the canonical receipt order
// (ascending sender; MP1Node::checkMessages drains a queue of any length, MP1Node.cpp:200-212),
// slots moved along.  An all-ascending bitonic network over the next power of two: every
// compare-exchange keeps the smaller key at the lower index, so the virtual +inf keys past k
// never move and pairs reaching past k are skipped.  A segment belongs to one workgroup per
// launch, and the launches that share a CSR (column tiles) run in stream order, so a later
// launch re-sorts a sorted segment.
__device__ inline void sort_long_segment(int32_t *src, int32_t *slot, int32_t k) {
    int32_t P = 1;
    while (P < k) P <<= 1;
    for (int32_t size = 2; size <= P; size <<= 1) {
        for (int32_t half = size >> 1; half > 0; half >>= 1) {
            for (int32_t i = int32_t(threadIdx.x); i < (P >> 1); i += kScaleBlock) {
                const int32_t b = i / half, o = i - b * half;
                const bool flip = half == (size >> 1);   // pair i with its mirror in the block
                const int32_t lo = flip ? b * size + o : b * 2 * half + o;
                const int32_t hi = flip ? b * size + size - 1 - o : lo + half;
                if (hi >= k) continue;
                const int32_t x = src[lo], y = src[hi];
                if (y < x) {
                    src[lo] = y;
                    src[hi] = x;
                    if (slot) {
                        const int32_t u = slot[lo];
                        slot[lo] = slot[hi];
                        slot[hi] = u;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// kPolicy bit 0: non-temporal own-row loads/stores; bit 1: non-temporal sender-row loads.
// kPipe: software-pipelined chunk loads (the next chunk is requested before this one merges).
// kTfail: TFAIL suspicion (a.tfail > 0): a sender's payload holds only the members it could
// gossip at send time (t - 1 - ts < tfail), and only members with t - ts < tfail get a
// presence bit (peer choice) and count.
// kSwim: SWIM ping/ack probing (a.swim paths, oracle/scale_oracle.c): the probe this row sent at
// t - 1 is resolved after the merges (answered: ts of the target = t; unanswered: ts = t -
// TREMOVE, so the TREMOVE scan removes it), and wave 0 picks this tick's probe target.
// The row's LDS (namespace scope: one set per kernel, shared by both row forms below).
extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[];   // fused: stride/32 words
__shared__ int32_t s_src[kMaxSegment];
__shared__ int32_t s_slot[kMaxSegment];
__shared__ unsigned long long s_red[4][4];
__shared__ int32_t s_jc[kMaxIntro];      // JOINREP payload: chosen columns / entries
__shared__ uint32_t s_jv[kMaxIntro];
__shared__ int32_t s_njc;
__shared__ uint32_t s_evf[4];            // event stream: staged records per wave
__shared__ unsigned long long s_evbase;

// One row lr of the tick.  kLong: a row whose segment is longer than the LDS sort (k >
// kMaxSegment, a join burst on the introducer), run by scale_long_kernel -- its own kernel,
// because any share of its state in the tick kernel's body (one body with a runtime branch, an
// inlined second copy, a called function) cost the plain rows registers: +1.1 % to +30 %
// VGPRs or SGPR spills at config 3.  The tick kernel only defers such a row (a list entry).
template <bool kInit, bool kSlice, int kMerge, int kPolicy, bool kPipe, bool kTfail, bool kSwim,
          bool kLong>
__device__ __forceinline__ void scale_tick_row(const ScaleTickArgs &a, const int32_t lr) {
    constexpr bool kNtOwn = (kPolicy & 1) != 0, kNtSrc = (kPolicy & 2) != 0;

    const int32_t tid = threadIdx.x;
    const int32_t lane = tid & 63, wave = tid >> 6;
    const int32_t r = a.row0 + lr;
    const int32_t t = a.tick;
    const int32_t F = a.fanout;

    if (!kInit && *a.err) return;      // a capacity error froze the job at an earlier tick
    // crashed (Application.cpp:186) or not started yet (Application.cpp:143): no recv, no
    // ops, no send
    if (t > a.fail_tick[r] || (a.start_tick && t < a.start_tick[r])) {
        if (!kSlice && tid < F) a.out_dst[int64_t(lr) * F + tid] = -1;
        return;
    }

    int32_t k = 0;
    // a long segment (k > kMaxSegment): sorted in HBM, its first k - kMaxSegment messages are
    // merged by the premerge below and the chunk loop merges the rest from LDS
    if (!kInit) {
        const int32_t o0 = a.off[lr];
        k = a.off[lr + 1] - o0;
        if (k > a.max_segment) {      // tests only (GSP_TEST_MAX_SEGMENT): a capacity error
            if (tid == 0) atomicCAS(a.err, 0, t);
            if (!kSlice && tid < F) a.out_dst[int64_t(lr) * F + tid] = -1;
            return;
        }
        if (!kLong && k > kMaxSegment) {   // deferred to scale_long_kernel (one list per CSR)
            if (tid == 0) defer_row(a.long_list, lr);
            return;
        }
    }
    if constexpr (kLong) {
        const int32_t o0 = a.off[lr];
        sort_long_segment(a.csr_src + o0, a.csr_slot ? a.csr_slot + o0 : nullptr, k);
        if (tid == 0) s_src[0] = a.csr_src[o0];           // the JOINREP test below
        __syncthreads();
    } else if (!kInit) {
        const int32_t o0 = a.off[lr];
        for (int32_t i = tid; i < k; i += kScaleBlock) s_src[i] = a.csr_src[o0 + i];
        __syncthreads();
        // canonical receipt order: ascending sender (senders are distinct per receiver)
        int32_t rank[kMaxSegment / kScaleBlock], val[kMaxSegment / kScaleBlock],
            slot[kMaxSegment / kScaleBlock];
#pragma unroll
        for (int q = 0; q < kMaxSegment / kScaleBlock; ++q) {
            const int32_t i = tid + q * kScaleBlock;
            rank[q] = -1;
            if (i < k) {
                val[q] = s_src[i];
                slot[q] = sender_slot(a, o0 + i, val[q]);
                int32_t rk = 0;
                for (int32_t j = 0; j < k; ++j) rk += s_src[j] < val[q];
                rank[q] = rk;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kMaxSegment / kScaleBlock; ++q)
            if (rank[q] >= 0) { s_src[rank[q]] = val[q]; s_slot[rank[q]] = slot[q]; }
        __syncthreads();
    }
    // a JOINREP (sender kJoinRepSrc, sorted first) is merged apart from the GOSSIP loop: wave 0
    // resolves its payload columns, and the GOSSIPs are s_src[jr .. k)
    int32_t jr = (!kInit && k > 0 && s_src[0] == kJoinRepSrc) ? 1 : 0;
    if (jr) {
        if (wave == 0) {
            const int32_t nj = join_choose(a, r, t, s_jc, s_jv);
            if (lane == 0) s_njc = nj < kMaxIntro ? nj : kMaxIntro;
        }
        __syncthreads();
    }
    const int32_t njc = jr ? s_njc : 0;

    const uint32_t t5 = uint32_t(t) & 31u;
    const uint32_t tr = uint32_t(a.tremove);
    const PackedConsts pc = packed_consts(t5, tr);
    const uint32_t tf = uint32_t(a.tfail);
    const uint32_t tfx2 = tf | (tf << 16);
    const uint32_t t5m1 = uint32_t(t - 1) & 31u;                  // the senders' tick, mod 32
    const uint32_t t32m1 = (t5m1 | (t5m1 << 16)) + 0x00200020u;
    // kSwim: the probe of t - 1 (target pcol, read before wave 0 rewrites a.ping[lr] below the
    // block reduction's barrier); one direct + a.swim - 1 indirect paths, each with a drop draw
    int32_t pcol = -1;
    uint32_t pts = 0;                  // the target's new ts mod 32
    if (kSwim && !kInit) {
        pcol = a.ping[lr];
        if (pcol >= 0) {
            bool ok = false;
            for (int32_t i = 0; i < a.swim; ++i) {
                const uint32_t dr = draw_u31(kDomainPing, a.seed, uint32_t(t - 1), uint32_t(r),
                                             uint32_t(pcol), uint32_t(i));
                ok = ok || int32_t(dr % 100u) >= a.drop_prev;     // paths sent at t - 1
            }
            ok = ok && t <= a.fail_tick[pcol] && (!a.start_tick || t >= a.start_tick[pcol]);
            pts = ok ? t5 : ((t5 - tr) & 31u);
        }
    }
    const int64_t stride = a.stride;
    const uint16_t *own_prev = a.prev + int64_t(lr) * stride;
    uint16_t *own_cur = a.cur + int64_t(lr) * stride;
    uint32_t live = 0, joins = 0, removes = 0;
    uint64_t hsum = 0;
    if constexpr (kLong) {
        // Premerge of a long segment: the JOINREP and the GOSSIPs at sorted positions [jr, pend)
        // merged in order into the own row, written to this tick's row (read back by the chunk
        // loop as its own row, so the chunk loop merges senders [pend, k) after them: the same
        // order).  The joins made here are counted here: absent before the tick, present after
        // the premerge -- such an entry is fresh, and later merges only raise it, so the TREMOVE
        // scan never removes it -- except the own column (cleared after the merges) and an
        // unanswered probe target (made stale, then removed by the TREMOVE scan).
        const int32_t o0 = a.off[lr], pend = k - kMaxSegment;
        unsigned long long *const evb = (a.ev.buf && (a.ev.kinds & GSP_EVENTS_JOIN)) ? ev_stripe_buf(a.ev) : nullptr;
        for (int64_t c0 = 0; c0 < stride; c0 += kChunk) {
            const int64_t lc0 = c0 + int64_t(tid) * kEntriesPerLane, gc0 = a.col0 + lc0;
            uint4 e = ld16<false>(own_prev + lc0);
            const uint4 b = e;
            if (jr) merge_joinrep(e, gc0, njc, s_jc, s_jv, t5, tr);
            for (int32_t j = jr; j < pend; ++j) {
                const int32_t sj = a.csr_src[o0 + j];
                uint4 v = ld16<false>(sender_row(a, sender_slot(a, o0 + j, sj)) + lc0);
                if (kTfail) gossiped_vec(v, pc, tfx2, t32m1);
                merge_vec<0>(e, v, pc, t5, tr);
                bump_sender(e, sj, gc0, t5);
            }
            // The join count is spelled out here, not scan_entries: no TREMOVE scan runs yet (the
            // chunk loop's does), and the two exclusions above are this premerge's alone.
            const uint32_t bw[4] = {b.x, b.y, b.z, b.w};
            const uint32_t ew[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int i = 0; i < kEntriesPerLane; ++i) {
                const int sh = (i & 1) * 16;
                const int64_t col = gc0 + i;
                const bool before = (bw[i >> 1] >> sh) & 0xFFFFu, after = (ew[i >> 1] >> sh) & 0xFFFFu;
                if (!before && after && col != r && !(kSwim && col == pcol && pts != t5)) {
                    joins++;
                    hsum += event_mix(1, uint32_t(t), uint32_t(r), uint32_t(col));
                    if (evb) {
                        const unsigned long long p = atomicAdd(ev_stripe_count(a.ev), 1ull);
                        if (int64_t(p) < a.ev.cap) evb[p] = event_record(1u, uint32_t(t), uint32_t(r), uint32_t(col));
                    }
                }
            }
            st16<false>(own_cur + lc0, ew);
        }
        // the chunk loop: the own row is the premerged one, the senders the last kMaxSegment
        for (int32_t i = tid; i < kMaxSegment; i += kScaleBlock) {
            const int32_t sj = a.csr_src[o0 + pend + i];
            s_src[i] = sj;
            s_slot[i] = sender_slot(a, o0 + pend + i, sj);
        }
        __syncthreads();
        own_prev = own_cur;
        jr = 0;
        k = kMaxSegment;
    }
    // event stream: each wave stages its records as kind << 30 | column in LDS (after the
    // bitmap, kEvStage words per wave) and the row takes one ring reservation at its end; a
    // wave whose stage would overflow flushes it with a reservation of its own
    uint32_t *const s_ev = s_bits + (kSlice ? 4 : (stride >> 5)) + wave * kEvStage;
    uint32_t ev_fill = 0;                                           // wave-uniform
    unsigned long long *const ev_buf = a.ev.buf ? ev_stripe_buf(a.ev) : nullptr;
    unsigned long long *const ev_count = ev_stripe_count(a.ev);

    // kPipe: the first 4 sender rows as wave-uniform (scalar) pointers, and the request of one
    // chunk's own + sender vectors (16 B per lane each) issued one chunk ahead
    const uint16_t *srow[4];
    uint4 pe = make_uint4(0u, 0u, 0u, 0u), pv[4];
    auto issue = [&](int64_t col) {
        pe = ld16<kNtOwn>(own_prev + col);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (jr + u < k) pv[u] = ld16<kNtSrc>(srow[u] + col);
    };
    if (kPipe && !kInit) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pv[u] = make_uint4(0u, 0u, 0u, 0u);
            srow[u] = sender_row(a, __builtin_amdgcn_readfirstlane(jr + u < k ? s_slot[jr + u] : 0));
        }
        issue(int64_t(tid) * kEntriesPerLane);
    }

    for (int64_t c0 = 0; c0 < stride; c0 += kChunk) {
        const int64_t lc0 = c0 + int64_t(tid) * kEntriesPerLane;   // column in this table
        const int64_t gc0 = a.col0 + lc0;                            // global column
        uint32_t ws[4];
        uint32_t w0[4] = {0u, 0u, 0u, 0u};
        if (kInit) {
            // pre-joined: the nodes that start at tick 0 list each other (h0, ts 0)
            const bool late_row = a.start_tick && a.start_tick[r] > 0;
            const uint32_t h = uint32_t(a.h0) << 5;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t x0 = gc0 + 2 * i, x1 = x0 + 1;
                bool on0 = x0 < a.n && x0 != r && !late_row, on1 = x1 < a.n && x1 != r && !late_row;
                if (a.start_tick) {
                    on0 = on0 && a.start_tick[x0] == 0;
                    on1 = on1 && a.start_tick[x1] == 0;
                }
                ws[i] = (on0 ? h : 0u) | ((on1 ? h : 0u) << 16);
            }
        } else {
            uint4 e;
            uint4 cv[4];
            if (kPipe) {
                // chunk c's own and first 4 sender vectors arrived with the previous request;
                // chunk c + 1's are requested before chunk c is merged
                e = pe;
#pragma unroll
                for (int u = 0; u < 4; ++u) cv[u] = pv[u];
                if (c0 + kChunk < stride) issue(lc0 + kChunk);
            } else {
                e = ld16<kNtOwn>(own_prev + lc0);
            }
            w0[0] = e.x; w0[1] = e.y; w0[2] = e.z; w0[3] = e.w;
            if (jr) merge_joinrep(e, gc0, njc, s_jc, s_jv, t5, tr);
            for (int32_t j0 = jr; j0 < k; j0 += 4) {
                uint4 v[4];
                if (kPipe && j0 == jr) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = cv[u];
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (j0 + u < k) v[u] = ld16<kNtSrc>(sender_row(a, s_slot[j0 + u]) + lc0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j0 + u >= k) break;
                    if (kTfail) gossiped_vec(v[u], pc, tfx2, t32m1);
                    merge_vec<kMerge>(e, v[u], pc, t5, tr);
                    bump_sender(e, s_src[j0 + u], gc0, t5);
                }
            }
            clear_own(e, r, gc0);
            if (kSwim && pcol >= 0) {                 // the probe's answer (or its absence)
                const int64_t dp = int64_t(pcol) - gc0;
                if (dp >= 0 && dp < kEntriesPerLane)
                    patch16(e, int(dp), [pts](uint32_t old) { return old ? ((old & 0xFFE0u) | pts) : 0u; });
            }
            ws[0] = e.x; ws[1] = e.y; ws[2] = e.z; ws[3] = e.w;
        }

        // TREMOVE scan, events and presence bits of the 8 entries
        uint32_t bits = 0, evj = 0, evr = 0;  // evj / evr: this chunk's join / remove entries
        bool slow = true;
        if constexpr (kMerge == 1 && !kInit) slow = screen_vec<kTfail>(ws, w0, pc, tfx2, bits);
        if (slow) bits = scan_entries<kInit, kTfail>(ws, w0, t, r, gc0, tr, tf, joins, removes, hsum, evj, evr);
        if (!kInit && ev_buf)                 // the event stream: stage this chunk's records
            ev_fill = ev_stage(s_ev, ev_fill, evj, evr, a.ev.kinds, gc0, [&](uint32_t fill, uint32_t total) {
                if (fill + total <= uint32_t(kEvStage)) return fill;
                ev_flush(ev_buf, s_ev, fill, ev_reserve(ev_count, fill, lane), a.ev.cap, t, r, lane);
                return 0u;
            });
        live += __builtin_popcount(bits);
        st16<kNtOwn>(own_cur + lc0, ws);
        // presence bitmap: 8 bits per lane -> byte (lc0 / 8)
        if (kSlice)
            a.bitmap[int64_t(lr) * (stride >> 3) + (lc0 >> 3)] = uint8_t(bits);
        else
            reinterpret_cast<uint8_t *>(s_bits)[lc0 >> 3] = uint8_t(bits);
    }

    // block reduction: live, joins, removes, hash
    const uint64_t v0 = wave_sum64(live), v1 = wave_sum64(joins), v2 = wave_sum64(removes);
    const uint64_t v3 = wave_sum64(hsum);
    if (lane == 0) { s_red[wave][0] = v0; s_red[wave][1] = v1; s_red[wave][2] = v2; s_red[wave][3] = v3; }
    if (!kInit && ev_buf && lane == 0) s_evf[wave] = ev_fill;
    __syncthreads();
    const uint64_t tot_live = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
    if (!kInit && ev_buf) {                   // the row's one ring reservation
        const uint32_t f0 = s_evf[0], f1 = s_evf[1], f2 = s_evf[2], f3 = s_evf[3];
        if (tid == 0 && f0 + f1 + f2 + f3) s_evbase = atomicAdd(ev_count, (unsigned long long)(f0 + f1 + f2 + f3));
        __syncthreads();
        if (f0 + f1 + f2 + f3) {
            const uint32_t before = (wave > 0 ? f0 : 0u) + (wave > 1 ? f1 : 0u) + (wave > 2 ? f2 : 0u);
            ev_flush(ev_buf, s_ev, ev_fill, s_evbase + before, a.ev.cap, t, r, lane);
        }
    }

    unsigned long long *dig = a.dig + (blockIdx.x % kDigSlots) * kDigFields;
    if (tid == 0) {
        a.cnt_cur[r] = int32_t(tot_live);
        if (!kInit) {
            a.own_hb[lr] += 1;
            if (a.count_rounds) {
                unsigned long long merges = 0;
                if (jr) merges += joinrep_merges(a);
                // the whole segment (a long one's premerged part too, from the sorted CSR)
                int32_t ka = k;
                if constexpr (kLong) {
                    const int32_t o0 = a.off[lr];
                    ka = a.off[lr + 1] - o0;
                    if (a.csr_src[o0] == kJoinRepSrc) merges += joinrep_merges(a);   // it went to the premerge
                    for (int32_t j = a.csr_src[o0] == kJoinRepSrc ? 1 : 0; j < ka; ++j)
                        merges += 1ull + uint64_t(a.cnt_prev[a.csr_src[o0 + j]]);
                } else {
                    for (int32_t j = jr; j < k; ++j) merges += 1ull + uint64_t(a.cnt_prev[s_src[j]]);
                }
                atomicAdd(&dig[kDigRounds], 1ull);
                atomicAdd(&dig[kDigMerges], merges);
                atomicAdd(&dig[kDigDelivered], (unsigned long long)ka);
            }
            atomicAdd(&dig[kDigJoins], s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1]);
            atomicAdd(&dig[kDigRemoves], s_red[0][2] + s_red[1][2] + s_red[2][2] + s_red[3][2]);
            atomicAdd(&dig[kDigHash], s_red[0][3] + s_red[1][3] + s_red[2][3] + s_red[3][3]);
        }
    }
    if (kSlice) return;

    // send: wave 0 picks min(F, live) distinct members by Philox rank-select
    if (wave == 0) {
        const int32_t per = int32_t(stride >> 5) >> 6;   // bitmap words per lane
        uint32_t lane_cnt = 0;
        for (int32_t w = 0; w < per; ++w) lane_cnt += __builtin_popcount(s_bits[lane * per + w]);
        uint32_t total = 0;
        const uint32_t pre = wave_excl_prefix(lane_cnt, &total);
        const int32_t cnt = int32_t(tot_live);
        const int32_t keff = F < cnt ? F : cnt;
        int32_t chosen[16];
        int32_t nch = 0;
        unsigned long long sent = 0, dropped = 0;
        for (int32_t kk = 0; kk < F; ++kk) {
            int32_t dst = -1;
            if (kk < keff) {
                const uint32_t u = draw_u31(kDomainPeer, a.seed, uint32_t(t), uint32_t(r),
                                            uint32_t(kk), 0u);
                const int32_t rk = next_distinct_rank(u, cnt, kk, chosen, nch);
                dst = wave_select([&](int32_t w) { return s_bits[w]; }, per, lane_cnt, pre,
                                  uint32_t(rk), lane);
                sent++;
                const uint32_t dr = draw_u31(kDomainSend, a.seed, uint32_t(t), uint32_t(r),
                                             uint32_t(dst), 3u);
                if (int32_t(dr % 100u) < a.drop_pct) { dropped++; dst = -1; }
            }
            if (lane == 0) {
                a.out_dst[int64_t(lr) * F + kk] = dst;
                if (dst >= 0) atomicAdd(&a.deg[dst], 1);
            }
        }
        if (lane == 0 && sent) {
            atomicAdd(&dig[kDigSent], sent);
            atomicAdd(&dig[kDigDropped], dropped);
        }
        if (kSwim) {                                  // this tick's probe target
            int32_t p = -1;
            if (cnt > 0) {
                const uint32_t u = draw_u31(kDomainPing, a.seed, uint32_t(t), uint32_t(r), 0u, 0x100u);
                p = wave_select([&](int32_t w) { return s_bits[w]; }, per, lane_cnt, pre,
                                u % uint32_t(cnt), lane);
            }
            if (lane == 0) a.ping[lr] = p;
        }
    }
}

template <bool kInit, bool kSlice, int kMerge, int kPolicy, bool kPipe = false, bool kTfail = false,
          bool kSwim = false>
__global__ void __launch_bounds__(kScaleBlock) scale_tick_kernel(ScaleTickArgs a) {
    scale_tick_row<kInit, kSlice, kMerge, kPolicy, kPipe, kTfail, kSwim, false>(a, int32_t(blockIdx.x));
}

// The sub-slab sweep of a column tile (slice form, plain protocol; DESIGN.md "Column tiles"):
// the tile's stride columns are cut into stride / W sub-slabs of W = 512 * kV columns and the
// grid walks them sub-slab-major (within a tile: item = sub-slab * batches + batch), so that between two
// reads of a previous-table line the chip touches one sub-slab of prev and one of cur, which
// the Infinity Cache holds.  A work item is one wave on (row, sub-slab): a workgroup takes
// kSweepBatch consecutive rows of one sub-slab, 16 per wave, with no barrier and no LDS on
// the row path (LDS stages event records only).
//   prologue  lane i of a wave loads row i's CSR bounds and crash tick, and the wave loads the
//             16 rows' (contiguous) sender ids in one request; rows are walked by readlane
//   order     ascending sender, ranked in registers (one id per lane, k <= sweep_seg <= kSweepMaxSeg)
//   deferred  rows with more messages go to mid_list (k <= kMaxSegment) or long_list, appended
//             by the sub-slab-0 item of the CSR's owner; scale_long_kernel runs them
//   results   the presence byte per lane as in the block form; the slice member count as one
//             plain store per (sub-slab, row) to cnt_sub, summed by sweep_count_kernel; digest
//             sums kept in registers over the wave's rows and added once, when non-zero; the
//             per-row quantities (rounds, merges, delivered, own_hb) by the sub-slab-0 item
// 5 waves per SIMD (96 VGPRs; 9 dwords spilled, in a 40-byte scratch frame of 10 dwords, for
// values the row loop does not touch):
// measured at config 3 against 4 waves (107 VGPRs, no scratch) and 6 (80 VGPRs, 26 dwords):
// 6.21 ms per tick against 7.07 and 6.97 (DESIGN.md "Column tiles").
// One launch runs every local tile of the tick: the grid is tile-major, then sub-slab-major, then
// batch (gridDim = ntiles * sub-slabs * batches; the tiles agree in rows and stride), so the
// order inside a tile is the one above and tile g + 1's first sub-slab fills the CUs that tile
// g's last one frees.  A workgroup's tile is wave-uniform: its args are scalar loads from the tile
// table (tile_args), all issued before the first store.
template <bool kNtCur>
__global__ void __launch_bounds__(kScaleBlock) __attribute__((amdgpu_waves_per_eu(5, 8)))
scale_sweep_kernel(const ScaleTickArgs *__restrict__ tpl, int32_t ntiles, ScaleTickVals tv) {
    constexpr int W = kSweepWidth;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t per_tile = int32_t(gridDim.x) / ntiles;
    const int32_t tile = int32_t(blockIdx.x) / per_tile, item = int32_t(blockIdx.x) - tile * per_tile;
    const ScaleTickArgs a = tile_args(tpl, tile, tv);
    const int32_t batches = (a.rows + kSweepBatch - 1) / kSweepBatch;
    const int32_t sub = item / batches, batch = item - sub * batches;
    if (*a.err) return;
    const int32_t t = a.tick;
    const int32_t lr0 = batch * kSweepBatch + wave * (kSweepBatch / 4);
    if (lr0 >= a.rows) return;
    const int64_t stride = a.stride;
    const uint32_t t5 = uint32_t(t) & 31u, tr = uint32_t(a.tremove);
    const PackedConsts pc = packed_consts(t5, tr);

    // batch prologue: lane i holds row lr0 + i (m_k = -1: crashed, or past the last row)
    const int32_t mlr = lr0 + (lane & 15);
    int32_t m_off = 0, m_k = -1;
    if (lane < kSweepBatch / 4 && mlr < a.rows) {
        m_off = a.off[mlr];
        if (t <= a.fail_tick[a.row0 + mlr]) m_k = a.off[mlr + 1] - m_off;
    }
    const int32_t nrows = a.rows - lr0 < kSweepBatch / 4 ? a.rows - lr0 : kSweepBatch / 4;
    const int32_t seg0 = int32_t(lane_of(uint32_t(m_off), 0));
    const int32_t seg1 = a.off[lr0 + nrows];
    const int32_t seg = seg0 + lane < seg1 ? a.csr_src[seg0 + lane] : 0;   // the first 64 senders

    uint32_t *const s_ev = s_bits + wave * W;
    unsigned long long *const ev_buf = a.ev.buf ? ev_stripe_buf(a.ev) : nullptr;
    unsigned long long *const ev_count = ev_stripe_count(a.ev);
    uint32_t joins = 0, removes = 0, delivered = 0, m_cnt = 0;
    uint64_t hsum = 0, merges = 0;

    const int64_t lc0 = int64_t(sub) * W + lane * kEntriesPerLane;     // column in this table
    const int64_t gc0 = a.col0 + lc0;                                   // global column
    // the next row the wave runs, from row i on (nrows: none); a row with more messages than
    // the wave orders is deferred on the way
    auto next_row = [&](int32_t i) {
        for (; i < nrows; ++i) {
            const int32_t k = int32_t(lane_of(uint32_t(m_k), i));
            if (k < 0) continue;
            if (k <= a.sweep_seg) break;
            if (sub == 0 && a.appends && lane == 0) defer_row(k > kMaxSegment ? a.long_list : a.mid_list, lr0 + i);
        }
        return i;
    };
    // row i's senders in ascending order, one per lane (ids are distinct), and the request of
    // its own vector and its first 4 senders' vectors (16 B per lane each)
    auto request = [&](int32_t i, int32_t &k, int32_t &sorted, uint4 &e, uint4 (&sv)[4]) {
        k = int32_t(lane_of(uint32_t(m_k), i));
        const int32_t o0 = int32_t(lane_of(uint32_t(m_off), i));
        int32_t sid;
        if (o0 - seg0 + k <= 64) sid = __builtin_amdgcn_ds_bpermute((o0 - seg0 + lane) << 2, seg);
        else sid = lane < k ? a.csr_src[o0 + lane] : 0;
        if (lane >= k) sid = INT32_MAX;
        int32_t rk = 0;
        for (int32_t j = 0; j < k; ++j) rk += int32_t(lane_of(uint32_t(sid), j)) < sid ? 1 : 0;
        sorted = __builtin_amdgcn_ds_permute((lane < k ? rk : lane) << 2, sid);
        if (sub == 0 && a.count_rounds) {
            if (lane < k) merges += 1ull + uint64_t(a.cnt_prev[sid]);
            delivered += lane == 0 ? uint32_t(k) : 0u;
        }
        e = ld16<false>(local_row(a, lr0 + i) + lc0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < k)
                sv[u] = ld16<false>(local_row(a, int32_t(lane_of(uint32_t(sorted), u)) - a.row0) + lc0);
    };

    // the rows are pipelined: row i + 1's vectors are requested before row i is merged
    int32_t k = 0, sorted = 0, nk = 0, nsorted = 0;
    uint4 e = make_uint4(0u, 0u, 0u, 0u), ne = e, sv[4], nsv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) sv[u] = nsv[u] = e;
    int32_t i = next_row(0);
    if (i < nrows) request(i, k, sorted, e, sv);
    while (i < nrows) {
        const int32_t lr = lr0 + i, r = a.row0 + lr;
        const int32_t ni = next_row(i + 1);
        if (ni < nrows) request(ni, nk, nsorted, ne, nsv);
        uint16_t *own_cur = a.cur + int64_t(lr) * stride;
        uint32_t live = 0, ev_fill = 0;
        {
            const uint32_t w0[4] = {e.x, e.y, e.z, e.w};
            for (int32_t j0 = 0; j0 < k; j0 += 4) {
                int32_t ss[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j0 + u < k) {
                        ss[u] = int32_t(lane_of(uint32_t(sorted), j0 + u));
                        if (j0) sv[u] = ld16<false>(local_row(a, ss[u] - a.row0) + lc0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j0 + u >= k) break;
                    merge_vec<1>(e, sv[u], pc, t5, tr);
                    bump_sender(e, ss[u], gc0, t5);
                }
            }
            clear_own(e, r, gc0);
            uint32_t ws[4] = {e.x, e.y, e.z, e.w};

            uint32_t bits = 0, evj = 0, evr = 0;
            if (screen_vec<false>(ws, w0, pc, 0u, bits))
                bits = scan_entries<false, false>(ws, w0, t, r, gc0, tr, 0u, joins, removes, hsum, evj, evr);
            if (ev_buf)                           // the event stream: a sub-slab's records always fit
                ev_fill = ev_stage(s_ev, ev_fill, evj, evr, a.ev.kinds, gc0, [](uint32_t fill, uint32_t) { return fill; });
            live += __builtin_popcount(bits);
            st16<kNtCur>(own_cur + lc0, ws);
            a.bitmap[int64_t(lr) * (stride >> 3) + (lc0 >> 3)] = uint8_t(bits);
        }
        const uint32_t row_live = wave_sum32(live);
        if (lane == i) m_cnt = row_live;
        if (ev_fill)                              // the item's one ring reservation
            ev_flush(ev_buf, s_ev, ev_fill, ev_reserve(ev_count, ev_fill, lane), a.ev.cap, t, r, lane);
        i = ni;
        k = nk;
        sorted = nsorted;
        e = ne;
#pragma unroll
        for (int u = 0; u < 4; ++u) sv[u] = nsv[u];
    }

    // the batch's results: counts by the lanes that hold the rows, the digest once per wave
    const bool ran = lane < kSweepBatch / 4 && m_k >= 0 && m_k <= a.sweep_seg;
    if (ran) {
        a.cnt_sub[int64_t(sub) * a.n + a.row0 + mlr] = int32_t(m_cnt);
        if (sub == 0) a.own_hb[mlr] += 1;
    }
    unsigned long long *dig = a.dig + (blockIdx.x % kDigSlots) * kDigFields;
    const uint32_t tj = wave_sum32(joins), trm = wave_sum32(removes);
    const uint64_t th = wave_sum64(hsum);
    if (lane == 0) {
        if (tj) atomicAdd(&dig[kDigJoins], (unsigned long long)tj);
        if (trm) atomicAdd(&dig[kDigRemoves], (unsigned long long)trm);
        if (th) atomicAdd(&dig[kDigHash], (unsigned long long)th);
    }
    if (sub == 0 && a.count_rounds) {
        const uint32_t rounds = uint32_t(__builtin_popcountll(__ballot(ran)));
        const uint64_t tm = wave_sum64(merges);
        const uint32_t td = wave_sum32(delivered);
        if (lane == 0 && rounds) {
            atomicAdd(&dig[kDigRounds], (unsigned long long)rounds);
            atomicAdd(&dig[kDigMerges], (unsigned long long)tm);
            atomicAdd(&dig[kDigDelivered], (unsigned long long)td);
        }
    }
}

// cnt_cur[r] of every tile of the launch (blockIdx.y) = the sum of the sweep's per-sub-slab
// counts, for the rows the sweep ran: a crashed row keeps its count and a deferred row's is
// written by its own workgroup (scale_long_kernel).
__global__ void __launch_bounds__(256) sweep_count_kernel(ScaleTickArgs a, int32_t subs) {
    if (*a.err) return;
    const int32_t lr = int32_t(blockIdx.x) * 256 + int32_t(threadIdx.x);
    if (lr >= a.rows) return;
    const int32_t r = a.row0 + lr;
    if (a.tick > a.fail_tick[r] || a.off[lr + 1] - a.off[lr] > a.sweep_seg) return;
    const int32_t *sub = a.cnt_sub + int64_t(blockIdx.y) * subs * a.n + r;
    int32_t sum = 0;
    for (int32_t s = 0; s < subs; ++s) sum += sub[int64_t(s) * a.n];
    a.cnt_cur[int64_t(blockIdx.y) * a.n + r] = sum;
}

// The rows the tick kernels deferred (k > kMaxSegment), after every tick-kernel launch of the
// tick: tile g's args come from the tile table (made by the host, upload_long_tpl in
// scale_engine.cpp) through tile_args, which patches the tick's own fields; each tile's list is
// its CSR's.  shared: the tiles share one CSR (an in-process group, or one tile), so every
// tile's lists are tile 0's: their counts are read once, and with both at zero -- the usual
// tick -- no tile's args are loaded at all.  Launched once per tick.  It also clears the lists
// of the next tick's parity.
template <bool kSlice, bool kTfail, bool kSwim>
__global__ void __launch_bounds__(kScaleBlock) scale_long_kernel(ScaleTickArgs a, const ScaleTickArgs *tpl,
                                                                 int32_t ntiles, int32_t shared) {
    constexpr bool kMid = kSlice && !kTfail && !kSwim;
    const int32_t t = a.tick;
    const ScaleTickVals tv = tick_vals(a);
    int32_t cnt = 0, mid = 0;
    if (shared) {
        const ScaleTickArgs &own = tpl[t & 1];
        cnt = own.long_list[0];
        if (kMid && own.mid_list) mid = own.mid_list[0];
    }
    // shared lists, both empty: no tile has a row to run (uniform over the grid)
    const int32_t run_tiles = (shared && !(cnt | mid)) ? 0 : ntiles;
    for (int32_t g = 0; g < run_tiles; ++g) {
        const ScaleTickArgs ag = tile_args(tpl, g, tv);
        if (!shared) {
            cnt = ag.long_list[0];
            mid = (kMid && ag.mid_list) ? ag.mid_list[0] : 0;
        }
        for (int32_t i = int32_t(blockIdx.x); i < cnt; i += int32_t(gridDim.x)) {
            scale_tick_row<false, kSlice, 1, 0, false, kTfail, kSwim, true>(ag, ag.long_list[1 + i]);
            __syncthreads();                    // the row's LDS is read to its end
        }
        // the rows the sub-slab sweep left to the block form (kSweepMaxSeg < k <= kMaxSegment)
        if constexpr (kMid) {
            for (int32_t i = int32_t(blockIdx.x); i < mid; i += int32_t(gridDim.x)) {
                scale_tick_row<false, true, 1, 0, false, false, false, false>(ag, ag.mid_list[1 + i]);
                __syncthreads();
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int32_t g = 0; g < (shared ? 1 : ntiles); ++g) {
            const ScaleTickArgs &nx = tpl[2 * g + ((t + 1) & 1)];
            nx.long_list[0] = 0;
            if (nx.mid_list) nx.mid_list[0] = 0;
        }
}

// Column mode: one wave per sender.  The global member order of row s is the shards'
// slices in ascending column order, so rank rk lives on the first shard whose inclusive
// prefix of slice counts exceeds rk; that shard resolves the column from its bitmap.
__global__ void __launch_bounds__(256) scale_resolve_kernel(ScaleResolveArgs a) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t s = int32_t(blockIdx.x) * 4 + int32_t(threadIdx.x >> 6);
    if (s >= a.n) return;
    const int32_t F = a.fanout;
    const int32_t W = F + (a.swim > 0 ? 1 : 0);        // pick slots per sender
    if (a.tick > a.fail_tick[s] || (a.start_tick && a.tick < a.start_tick[s])) {
        if (lane < W) a.picks[int64_t(s) * W + lane] = -1;
        return;
    }
    const uint32_t c = lane < a.shards ? uint32_t(a.cnt_all[int64_t(lane) * a.n + s]) : 0u;
    uint32_t total = 0;
    const uint32_t cpre = wave_excl_prefix(c, &total);
    if (lane == 0) a.cnt_total[s] = int32_t(total);
    const int32_t cnt = int32_t(total);
    const int32_t keff = F < cnt ? F : cnt;
    const int32_t per = int32_t(a.stride >> 5) >> 6;
    // the bitmap of shard g's slice of row s, and its per-lane popcounts / prefix (cached for
    // the last shard used: a sender's picks fall into few shards' slices)
    const uint32_t *bm = nullptr;
    int32_t bm_g = -1;
    uint32_t lane_cnt = 0, pre = 0;
    auto resolve = [&](uint32_t rk) -> int32_t {        // wave-uniform rank -> column or -1
        const unsigned long long own = __ballot(lane < a.shards && rk >= cpre && rk < cpre + c);
        const int32_t g = __builtin_ffsll(own) - 1;
        if (a.tiled ? (g < a.tile_lo || g >= a.tile_lo + a.tile_cnt) : g != a.shard)
            return -1;                                   // another shard / rank resolves it
        if (g != bm_g) {
            bm = reinterpret_cast<const uint32_t *>(a.bitmap + (a.tiled ? int64_t(g - a.tile_lo) * a.tile_bytes : 0) +
                                                    int64_t(s) * (a.stride >> 3));
            lane_cnt = 0;
            for (int32_t w = 0; w < per; ++w) lane_cnt += __builtin_popcount(bm[lane * per + w]);
            uint32_t tot = 0;
            pre = wave_excl_prefix(lane_cnt, &tot);
            bm_g = g;
        }
        const uint32_t local = rk - __shfl(cpre, g, 64);
        const int32_t col = wave_select([&](int32_t w) { return bm[w]; }, per, lane_cnt, pre, local, lane);
        return int32_t(int64_t(g) * a.stride + col);
    };
    int32_t chosen[16];
    int32_t nch = 0;
    for (int32_t kk = 0; kk < F; ++kk) {
        int32_t pick = -1;
        if (kk < keff) {
            const uint32_t u = draw_u31(kDomainPeer, a.seed, uint32_t(a.tick), uint32_t(s),
                                        uint32_t(kk), 0u);
            pick = resolve(uint32_t(next_distinct_rank(u, cnt, kk, chosen, nch)));
        }
        if (lane == 0) a.picks[int64_t(s) * W + kk] = pick;
    }
    if (a.swim > 0) {      // the probe target: one more rank-select over the same global order
        int32_t pick = -1;
        if (cnt > 0) {
            const uint32_t u = draw_u31(kDomainPing, a.seed, uint32_t(a.tick), uint32_t(s), 0u, 0x100u);
            pick = resolve(u % uint32_t(cnt));
        }
        if (lane == 0) a.picks[int64_t(s) * W + F] = pick;
    }
    if (lane == 0 && a.count_rounds && keff > 0)
        atomicAdd(&a.dig[(s % kDigSlots) * kDigFields + kDigSent], (unsigned long long)keff);
}

__global__ void scale_finalize_kernel(ScaleResolveArgs a) {
    const int64_t slots = int64_t(a.n) * a.fanout;
    const int32_t W = a.fanout + (a.swim > 0 ? 1 : 0);
    unsigned long long dropped = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < slots;
         i += int64_t(gridDim.x) * blockDim.x) {
        const int32_t s = int32_t(i / a.fanout);
        if (a.swim > 0 && i % a.fanout == 0) a.ping[s] = a.picks[int64_t(s) * W + a.fanout];
        int32_t d = a.picks[int64_t(s) * W + (i - int64_t(s) * a.fanout)];
        if (d >= 0) {
            const uint32_t dr = draw_u31(kDomainSend, a.seed, uint32_t(a.tick), uint32_t(s),
                                         uint32_t(d), 3u);
            if (int32_t(dr % 100u) < a.drop_pct) { dropped++; d = -1; }
            else atomicAdd(&a.deg[d], 1);
        }
        a.out_dst[i] = d;
    }
    dropped = wave_sum64(dropped);
    if ((threadIdx.x & 63) == 0 && dropped && a.count_rounds)
        atomicAdd(&a.dig[(blockIdx.x % kDigSlots) * kDigFields + kDigDropped], dropped);
}

__global__ void max_into_kernel(int32_t *dst, const int32_t *src, int64_t count) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count;
         i += int64_t(gridDim.x) * blockDim.x)
        dst[i] = max(dst[i], src[i]);
}

// Exclusive scan of the destination counts, two launches: (1) every 1024-thread block sums
// its kScanTile elements; (2) every block adds the sums of the blocks before it (at most
// a few hundred values, read from L2) to an in-block scan of its tile.
constexpr int kScanThreads = 1024, kScanPer = 4, kScanTile = kScanThreads * kScanPer;

__device__ inline int32_t block_scan_incl(int32_t v, int32_t *s_wave) {
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    if (wave == 0) {
        int32_t w = lane < 16 ? s_wave[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const int32_t u = __shfl_up(w, d, 64);
            if (lane >= d) w += u;
        }
        if (lane < 16) s_wave[lane] = w;
    }
    __syncthreads();
    return v + (wave ? s_wave[wave - 1] : 0);
}

__global__ void __launch_bounds__(kScanThreads) tile_sum_kernel(const int32_t *deg, int32_t n,
                                                                int32_t *tile_sum) {
    __shared__ int32_t s_wave[16];
    const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
    int32_t v = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i)
        if (base + i < n) v += deg[base + i];
    const int32_t incl = block_scan_incl(v, s_wave);
    if (threadIdx.x == kScanThreads - 1) tile_sum[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(kScanThreads) tile_scan_kernel(const int32_t *deg, int32_t n,
                                                                 const int32_t *tile_sum,
                                                                 int32_t *off) {
    __shared__ int32_t s_wave[16];
    __shared__ int32_t s_base;
    if (threadIdx.x < 64) {
        int32_t acc = 0;
        for (int32_t b = threadIdx.x; b < int32_t(blockIdx.x); b += 64) acc += tile_sum[b];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (threadIdx.x == 0) s_base = acc;
    }
    __syncthreads();
    const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
    int32_t v[kScanPer];
    int32_t sum = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
        v[i] = base + i < n ? deg[base + i] : 0;
        sum += v[i];
    }
    int32_t run = block_scan_incl(sum, s_wave) - sum + s_base;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
        if (base + i < n) off[base + i] = run;
        run += v[i];
    }
    if (base < n && base + kScanPer >= n) off[n] = run;   // the thread holding element n-1
}

__global__ void scatter_kernel(const int32_t *out_dst, int64_t slots, int32_t fanout,
                               int32_t row0, const int32_t *off, int32_t *fill,
                               int32_t *csr_src) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < slots;
         i += int64_t(gridDim.x) * blockDim.x) {
        const int32_t d = out_dst[i];
        if (d < 0) continue;
        const int32_t p = atomicAdd(&fill[d], 1);
        csr_src[off[d] + p] = row0 + int32_t(i / fanout);
    }
}

// the capacity test of the tick kernel, ahead of it (row shards of a communicator: the flag is
// then all-reduced, so every rank's tick kernels of t see it)
__global__ void segment_check_kernel(const int32_t *off, int32_t rows, int32_t max_segment, int32_t *err,
                                     int32_t t) {
    for (int32_t i = int32_t(blockIdx.x * blockDim.x + threadIdx.x); i < rows; i += int32_t(gridDim.x * blockDim.x))
        if (off[i + 1] - off[i] > max_segment) atomicCAS(err, 0, t);
}

unsigned grid_for(int64_t items, int64_t per_block, int64_t cap) {
    int64_t b = (items + per_block - 1) / per_block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return unsigned(b);
}

}  // namespace

size_t scale_lds_bytes(int64_t stride, bool slice, bool events) {
    return (slice ? 16 : size_t(stride / 8)) + (events ? size_t(4 * kEvStage * 4) : 0);
}

hipError_t launch_scale_init(const ScaleTickArgs &a, bool slice, hipStream_t st) {
    if (a.stride % kChunk || a.fanout < 1 || a.fanout > 16) return hipErrorInvalidValue;
    const size_t lds = scale_lds_bytes(a.stride, slice, false);
    if (slice)
        hipLaunchKernelGGL((scale_tick_kernel<true, true, 1, 0>), dim3(a.rows), dim3(kScaleBlock), lds, st, a);
    else if (a.swim > 0)
        hipLaunchKernelGGL((scale_tick_kernel<true, false, 1, 0, false, false, true>), dim3(a.rows),
                           dim3(kScaleBlock), lds, st, a);
    else
        hipLaunchKernelGGL((scale_tick_kernel<true, false, 1, 0>), dim3(a.rows), dim3(kScaleBlock), lds, st, a);
    return hipGetLastError();
}

template <bool kSlice, int kMerge>
void launch_tick_policy(const ScaleTickArgs &a, int policy, size_t lds, hipStream_t st) {
    const dim3 grid(a.rows), block(kScaleBlock);
    if (a.swim > 0) {
        if (a.tfail > 0)
            hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 1, false, true, true>), grid, block, lds, st, a);
        else
            hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 1, false, false, true>), grid, block, lds, st, a);
        return;
    }
    if (a.tfail > 0) {
        hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 1, false, true>), grid, block, lds, st, a);
        return;
    }
    if (a.pipe && kMerge == 1 && (policy & 3) == 1) {
        hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 1, true>), grid, block, lds, st, a);
        return;
    }
    switch (policy & 3) {
        case 0: hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 0>), grid, block, lds, st, a); break;
        case 1: hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 1>), grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 2>), grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL((scale_tick_kernel<false, kSlice, kMerge, 3>), grid, block, lds, st, a); break;
    }
}

// one launch of the sub-slab sweep over every local tile (sweep = W); nt_own: non-temporal
// stores of cur.  The kernel cuts the grid into equal tiles and one LDS size and one store
// policy serve the launch, so the tiles must agree in what decides them.
hipError_t launch_scale_sweep(const ScaleTickArgs *tiles, int32_t ntiles, const ScaleTickArgs *tpl,
                              hipStream_t st) {
    if (ntiles < 1 || !tiles || !tpl) return hipErrorInvalidValue;
    const ScaleTickArgs &a = tiles[0];
    const int32_t W = a.sweep;
    for (int32_t g = 0; g < ntiles; ++g) {
        const ScaleTickArgs &x = tiles[g];
        if (x.sweep != kSweepWidth || x.stride % W || x.sweep_seg < 1 || x.sweep_seg > kSweepMaxSeg || !x.cnt_sub ||
            !x.bitmap || x.csr_slot || x.tfail > 0 || x.swim > 0 || x.start_tick || x.fanout < 1 || x.fanout > 16)
            return hipErrorInvalidValue;
        if (x.rows != a.rows || x.stride != a.stride || x.rows < 1 || x.tick != a.tick || x.nt_own != a.nt_own ||
            (x.ev.buf != nullptr) != (a.ev.buf != nullptr))
            return hipErrorInvalidValue;
    }
    const int64_t blocks = int64_t(ntiles) * (a.stride / W) * ((int64_t(a.rows) + kSweepBatch - 1) / kSweepBatch);
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid{unsigned(blocks)}, block(kScaleBlock);
    const size_t lds = a.ev.buf ? size_t(4) * size_t(W) * 4 : 0;
    const ScaleTickVals tv = tick_vals(a);
    if (a.nt_own) hipLaunchKernelGGL((scale_sweep_kernel<true>), grid, block, lds, st, tpl, ntiles, tv);
    else hipLaunchKernelGGL((scale_sweep_kernel<false>), grid, block, lds, st, tpl, ntiles, tv);
    return hipGetLastError();
}

hipError_t launch_sweep_counts(const ScaleTickArgs &a, int32_t tiles, hipStream_t st) {
    if (a.sweep != kSweepWidth || tiles < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sweep_count_kernel, dim3(unsigned((a.rows + 255) / 256), unsigned(tiles)), dim3(256), 0, st,
                       a, int32_t(a.stride / a.sweep));
    return hipGetLastError();
}

hipError_t launch_scale_tick(const ScaleTickArgs &a, bool slice, int merge, hipStream_t st) {
    if (a.stride % kChunk || a.fanout < 1 || a.fanout > 16) return hipErrorInvalidValue;
    if (slice && merge == 1 && a.sweep) return hipErrorInvalidValue;   // launch_scale_sweep runs those tiles
    const size_t lds = scale_lds_bytes(a.stride, slice, a.ev.buf != nullptr) + size_t(a.lds_pad);
    const int policy = (a.nt_own ? 1 : 0) | (a.nt_src ? 2 : 0);
    if (slice) {
        if (merge == 1) launch_tick_policy<true, 1>(a, policy, lds, st);
        else launch_tick_policy<true, 0>(a, policy, lds, st);
    } else {
        if (merge == 1) launch_tick_policy<false, 1>(a, policy, lds, st);
        else launch_tick_policy<false, 0>(a, policy, lds, st);
    }
    return hipGetLastError();
}

hipError_t launch_scale_long(const ScaleTickArgs &a, const ScaleTickArgs *tpl, int32_t ntiles, bool slice,
                             bool shared_lists, hipStream_t st) {
    if (ntiles < 1) return hipErrorInvalidValue;
    const size_t lds = scale_lds_bytes(a.stride, slice, a.ev.buf != nullptr) + size_t(a.lds_pad);
    const dim3 grid(64), block(kScaleBlock);
    const int v = (slice ? 4 : 0) | (a.tfail > 0 ? 2 : 0) | (a.swim > 0 ? 1 : 0);
    const int32_t sh = shared_lists ? 1 : 0;
    switch (v) {
        case 0: hipLaunchKernelGGL((scale_long_kernel<false, false, false>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 1: hipLaunchKernelGGL((scale_long_kernel<false, false, true>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 2: hipLaunchKernelGGL((scale_long_kernel<false, true, false>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 3: hipLaunchKernelGGL((scale_long_kernel<false, true, true>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 4: hipLaunchKernelGGL((scale_long_kernel<true, false, false>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 5: hipLaunchKernelGGL((scale_long_kernel<true, false, true>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        case 6: hipLaunchKernelGGL((scale_long_kernel<true, true, false>), grid, block, lds, st, a, tpl, ntiles, sh); break;
        default: hipLaunchKernelGGL((scale_long_kernel<true, true, true>), grid, block, lds, st, a, tpl, ntiles, sh); break;
    }
    return hipGetLastError();
}

hipError_t launch_scale_resolve(const ScaleResolveArgs &a, hipStream_t st) {
    if (a.stride % kChunk || a.shards < 1 || a.shards > 64 || a.fanout > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scale_resolve_kernel, dim3(unsigned((a.n + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_scale_finalize(const ScaleResolveArgs &a, hipStream_t st) {
    const int64_t slots = int64_t(a.n) * a.fanout;
    hipLaunchKernelGGL(scale_finalize_kernel, dim3(grid_for(slots, 256, 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_max_into(int32_t *dst, const int32_t *src, int64_t count, hipStream_t st) {
    hipLaunchKernelGGL(max_into_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, st, dst, src,
                       count);
    return hipGetLastError();
}

hipError_t launch_exclusive_scan(const int32_t *deg, int32_t *off, int32_t n, int32_t *tile_sum,
                                 hipStream_t st) {
    const int32_t tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(tile_sum_kernel, dim3(tiles), dim3(kScanThreads), 0, st, deg, n, tile_sum);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(tiles), dim3(kScanThreads), 0, st, deg, n, tile_sum,
                       off);
    return hipGetLastError();
}

hipError_t launch_segment_check(const int32_t *off, int32_t rows, int32_t max_segment, int32_t *err,
                                int32_t t, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(segment_check_kernel, dim3(grid_for(rows, 256, 1024)), dim3(256), 0, st, off, rows,
                       max_segment, err, t);
    return hipGetLastError();
}

hipError_t launch_scatter(const int32_t *out_dst, int64_t slots, int32_t fanout, int32_t row0,
                          const int32_t *off, int32_t *fill, int32_t *csr_src, hipStream_t st) {
    hipLaunchKernelGGL(scatter_kernel, dim3(grid_for(slots, 256, 4096)), dim3(256), 0, st, out_dst,
                       slots, fanout, row0, off, fill, csr_src);
    return hipGetLastError();
}

}  // namespace gsp
