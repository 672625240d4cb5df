// gossip_protocol_amd/csrc/probes_host.hpp -- the host side of the eight read-only probes of the
// two scale-mode engines, on top of the engine core (engine_host.hpp): five snapshot probes of the
// current tick (census, view audit, overlay reach -- reach in a single-source-set and a 64-tree
// form, reach_run and reach_multi_run -- overlay clustering, cluster_run, and overlay components,
// components_run) and three per-tick probes that ride along with step between open and close
// (rumor trace, detection ledger, traffic ledger).  The engines derive
// from ProbeCore and pass themselves as E; kernels and their argument structs are in the
// *_kernels.hpp of each probe.
//
// What all eight keep:
//   - A probe reads the engine and writes only its own buffers, on the engine's stream: digests,
//     rows and events are the same with any set of probes open, and step with none open makes the
//     launches it makes without this header.
//   - A snapshot or a get comes after the engine has synchronised and reported any pending
//     capacity error; with a communicator it is collective (same tick, same arguments on every
//     rank).  It never sums the device state twice: per-tick probes all-reduce out of place into
//     staging, the snapshot probes in place into arrays zeroed per call.
//   - Host staging vectors persist across calls (no allocation per get); buffers come with the
//     first call (snapshot) or with open (per-tick) and go with close or the engine.
//   - state[x] is node_state() at the engine's tick.  kernel_ms is GPU time between two events,
//     accumulated only while the engine's timing is on and reported as 0.0 while it is off.
//   - Open, seed and close are made between steps and synchronise the stream: the caller's arrays
//     are free on return and no queued launch uses a freed buffer.
//   - Messages begin with the entry point's own name (`fn`).
#pragma once
#include <utility>

#include "audit_kernels.hpp"
#include "census_kernels.hpp"
#include "cluster_kernels.hpp"
#include "components_kernels.hpp"
#include "detect_kernels.hpp"
#include "engine_host.hpp"
#include "reach_kernels.hpp"
#include "reach_multi_kernels.hpp"
#include "rumor_kernels.hpp"
#include "traffic_kernels.hpp"

namespace gsp {

// ---- the shared pieces ----

// 0 not started, 1 alive, 2 crashed: the one definition of "alive at T"
inline uint8_t node_state(const EngineCore &c, int32_t T, size_t x) {
    return T < c.h_start[x] ? 0 : T <= c.h_fail[x] ? 1 : 2;
}

// a non-empty list of ids inside [0, n); `name` is the argument's name in the messages
inline int check_ids(const char *fn, const char *name, const int32_t *ids, int32_t count, int32_t n) {
    GSP_REQUIRE(ids && count > 0, GSP_ERR_INVALID, "%s: no %s (n_%s=%d)", fn, name, name, count);
    for (int32_t i = 0; i < count; ++i)
        GSP_REQUIRE(ids[i] >= 0 && ids[i] < n, GSP_ERR_INVALID, "%s: %s[%d]=%d outside [0,%d)", fn, name, i,
                    ids[i], n);
    return GSP_OK;
}

// the preamble of the entry points that do not go through the engine's sync
template <class E>
int probe_enter(E *s, const char *fn) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "%s: NULL", fn);
    GSP_HIP(hipSetDevice(s->device));
    return GSP_OK;
}

// The GPU time of one snapshot call: a pair of events the probe owns, recorded only while the
// engine's timing is on.  `ready` is set by arm(), which the probe calls last in its first-call
// block: a first call that failed half-way starts over on the next call.  Like DevBuf::alloc the
// members return the HIP status for the caller's GSP_HIP.
struct SpanTimer {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool ready = false;

    hipError_t arm() {
        hipError_t e = t0 ? hipSuccess : hipEventCreate(&t0);
        if (e == hipSuccess && !t1) e = hipEventCreate(&t1);
        ready = e == hipSuccess;
        return e;
    }
    hipError_t begin(const EngineCore &c) { return c.timing ? hipEventRecord(t0, c.st) : hipSuccess; }
    hipError_t end(const EngineCore &c) { return c.timing ? hipEventRecord(t1, c.st) : hipSuccess; }
    hipError_t elapsed(const EngineCore &c, double *ms) {     // once the stream has been synchronised
        float f = 0.f;
        const hipError_t e = c.timing ? hipEventElapsedTime(&f, t0, t1) : hipSuccess;
        *ms = double(f);
        return e;
    }
    void release() {
        for (hipEvent_t e : {t0, t1})
            if (e) (void)hipEventDestroy(e);
        t0 = t1 = nullptr;
        ready = false;
    }
};

// The GPU time of a per-tick probe: event pairs from the engine's pool around each timed span,
// summed into kernel_ms when the engine collects (sync, hence every get).
struct TickTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // timed spans not yet collected
    double kernel_ms = 0.0;

    // body()'s launches on the engine's stream as one timed span, with no host wait
    template <class E, class Body>
    int timed(E *s, Body body) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (s->timing) {
            e0 = s->event();
            e1 = s->event();
            GSP_HIP(hipEventRecord(e0, s->st));
        }
        if (int rc = body()) return rc;
        if (s->timing) {
            GSP_HIP(hipEventRecord(e1, s->st));
            pending.emplace_back(e0, e1);
        }
        return GSP_OK;
    }

    // the pending spans into kernel_ms (waits for their events)
    int collect(EngineCore &c) {
        for (auto &e : pending) {
            float ms = 0.f;
            GSP_HIP(hipEventSynchronize(e.second));
            GSP_HIP(hipEventElapsedTime(&ms, e.first, e.second));
            kernel_ms += ms;
        }
        give_back(c);
        return GSP_OK;
    }

    // the pending events back to the pool, uncounted (close; the engine's end, ahead of the pool's)
    void give_back(EngineCore &c) {
        for (auto &e : pending) {
            c.free_events.push_back(e.first);
            c.free_events.push_back(e.second);
        }
        pending.clear();
    }

    double ms(const EngineCore &c) const { return c.timing ? kernel_ms : 0.0; }
};

// The device arrays of a ledger (detection, traffic): 32-bit per-node fields `arr`, 64-bit sums
// `wide`, their staging twins for a get's all-reduce across ranks, and the host copies a get
// reads them into.
struct LedgerBufs {
    DevBuf<uint32_t> arr, red;
    DevBuf<unsigned long long> wide, red64;
    std::vector<uint32_t> h_arr;
    std::vector<unsigned long long> h_wide;
    size_t words = 0, wides = 0;                 // the extents in use

    // open: allocated (the twins where a get will stage) and zeroed on `st`
    int reset(size_t n_words, size_t n_wides, bool staging, hipStream_t st) {
        GSP_HIP(arr.alloc(n_words));
        GSP_HIP(wide.alloc(n_wides));
        if (staging) {
            GSP_HIP(red.alloc(n_words));
            GSP_HIP(red64.alloc(n_wides));
        }
        words = n_words;
        wides = n_wides;
        GSP_HIP(hipMemsetAsync(arr.p, 0, words * 4, st));
        GSP_HIP(hipMemsetAsync(wide.p, 0, wides * 8, st));
        return GSP_OK;
    }
    // A get's readback into h_arr / h_wide, waited for.  staged: the caller has all-reduced the
    // ledger into red / red64 on `st`, so the device state itself is never summed twice.
    int read(bool staged, hipStream_t st) {
        h_arr.resize(words);
        h_wide.resize(wides);
        GSP_HIP(hipMemcpyAsync(h_arr.data(), staged ? red.p : arr.p, words * 4, hipMemcpyDeviceToHost, st));
        GSP_HIP(hipMemcpyAsync(h_wide.data(), staged ? red64.p : wide.p, wides * 8, hipMemcpyDeviceToHost, st));
        GSP_HIP(hipStreamSynchronize(st));
        return GSP_OK;
    }
    void release() { release_all(arr, red, wide, red64); }
};

// ---- the probes' state ----

// The census accumulators (gsp_scale_census / gsp_pview_census), allocated by the first call:
// n-length device arrays and their host staging; the full view counts into listed / fresh, the
// partial view into counts (fresh << 32 | listed, split at readback).
struct CensusBufs {
    DevBuf<uint32_t> listed, fresh, max_hb;
    DevBuf<unsigned long long> counts;
    std::vector<uint32_t> h32;
    std::vector<unsigned long long> h64;
    SpanTimer span;

    void release() { release_all(listed, fresh, max_hb, counts, span); }
};

// The view-audit accumulators (gsp_scale_audit / gsp_pview_audit), allocated by the first call:
// arr holds the five n-length uint32 arrays (audit_kernels.hpp), print the fingerprints; alive /
// fp are the per-call truth the prologue kernel writes (fp: full view only).
struct AuditBufs {
    DevBuf<uint32_t> arr;
    DevBuf<unsigned long long> print;
    DevBuf<uint8_t> alive;
    DevBuf<uint64_t> fp;
    std::vector<uint32_t> h32;
    std::vector<unsigned long long> h64;
    SpanTimer span;

    void release() { release_all(arr, print, alive, fp, span); }
};

// The overlay-reach state (gsp_scale_reach / gsp_pview_reach), allocated by the first call and
// shared by every local shard: hops[n], the two n-bit maps reach_level rewrites per level, the
// cumulative count of reached nodes with its pinned mirror, and the sources' device copy.
struct ReachBufs {
    DevBuf<uint32_t> hops, count;
    DevBuf<uint64_t> front, todo;
    DevBuf<int32_t> src;
    uint32_t *h_count = nullptr;   // pinned
    SpanTimer span;

    void release() {
        release_all(hops, count, front, todo, src, span);
        if (h_count) (void)hipHostFree(h_count);
        h_count = nullptr;
    }
};

// The multi-source reach state (gsp_scale_reach_multi / gsp_pview_reach_multi,
// reach_multi_kernels.hpp), allocated by the first call and shared by every local shard: the three
// 64-bit words per node, the two bitmaps the level kernel rewrites, the 64 cumulative per-tree
// counters with their pinned mirror, and the sources' device copy.  hops[n_sources][n] comes with
// the first call that asks for hops, stage[world][nodes] with a communicator.
struct ReachMultiBufs {
    DevBuf<uint64_t> seen, front, next, hot, open, stage;
    DevBuf<uint32_t> count, hops;
    DevBuf<int32_t> src;
    uint32_t *h_count = nullptr;   // pinned, kReachMultiMax words
    SpanTimer span;

    void release() {
        release_all(seen, front, next, hot, open, stage, count, hops, src, span);
        if (h_count) (void)hipHostFree(h_count);
        h_count = nullptr;
    }
};

// The overlay-clustering state (gsp_scale_cluster / gsp_pview_cluster, cluster_kernels.hpp),
// allocated by the first call and shared by every local shard: the member word per node, the
// alive bitmap of the call (launch_audit_truth), the 64-bit counters and the observers' device
// copy, with the host staging of member and the counters.
struct ClusterBufs {
    DevBuf<uint64_t> member;
    DevBuf<uint8_t> alive;
    DevBuf<unsigned long long> ctr;
    DevBuf<int32_t> obs;
    std::vector<uint64_t> h_member;
    std::vector<unsigned long long> h_ctr;
    SpanTimer span;

    void release() { release_all(member, alive, ctr, obs, span); }
};

// The overlay-components state (gsp_scale_components / gsp_pview_components,
// components_kernels.hpp), allocated by the first call and shared by every local shard: arr holds
// the kCompArrays n-length uint32 arrays, active the bitmap of the nodes still at work, ctr the
// cumulative counters with their pinned mirror, h_label the host's copy of the labels and h_size
// the component sizes the counts are made from.
enum { kCompLab = 0, kCompFcol, kCompBcol, kCompPf, kCompPb, kCompIn, kCompOut, kCompComp, kCompArrays };
struct ComponentsBufs {
    DevBuf<uint32_t> arr;
    DevBuf<uint64_t> active;
    DevBuf<unsigned long long> ctr;
    unsigned long long *h_ctr = nullptr;   // pinned, kCompCounters words
    std::vector<uint32_t> h_label, h_size;
    SpanTimer span;

    void release() {
        release_all(arr, active, ctr, span);
        if (h_ctr) (void)hipHostFree(h_ctr);
        h_ctr = nullptr;
    }
};

// The rumor trace (gsp_*_rumor_*, rumor_kernels.hpp), allocated by open and freed by close, shared
// by every local shard.  `red` stages the all-reduced heard / known of a get across row-shard
// ranks, so the device state itself is never summed twice.
struct RumorBufs {
    bool open = false;
    int32_t rumors = 0, ticks_traced = 0;
    TickTimer timer;                             // the trace launches of the timed ticks
    DevBuf<uint32_t> know, known, red;
    DevBuf<int32_t> heard, src;
    std::vector<int32_t> seed_tick;              // per rumor: first seed with an alive source
    std::vector<std::vector<int32_t>> seeded;    // per rumor: the alive sources seeded, ascending
    std::vector<int32_t> h_heard;
    std::vector<uint32_t> h_known;

    void release() { release_all(know, known, red, heard, src); }
};

// The detection ledger (gsp_*_detect_*, detect_kernels.hpp), allocated by open and freed by close,
// shared by every local shard: every shard's ring folds into the one ledger (column tiles hold
// disjoint x, row shards disjoint r).  led: arr [kDetFields][n]; wide by_tick[span][4], then
// tot[kDetTotals].
struct DetectBufs {
    bool open = false;
    int form = kDetectAggregated;                // GSP_TEST_DETECT_FORM=0|1 (tests, A/B) overrides
    int32_t open_tick = 0, ticks_folded = 0;
    TickTimer timer;                             // the folds of the timed ticks
    DevBuf<int32_t> crash;                       // [n] h_fail
    LedgerBufs led;

    void release() { release_all(crash, led); }
};

// The traffic ledger (gsp_*_traffic_*, traffic_kernels.hpp), allocated by open and freed by close,
// shared by every local shard.  led: arr holds the four per-node counters [kTrFields][n] and,
// behind them, the watch rows watch[n_watch][span][2]; wide is a TrafficLayout.
struct TrafficBufs {
    bool open = false;
    int form = kTrafficFromSlots;                // GSP_TEST_TRAFFIC_FORM=0|1 (tests, A/B) overrides
    int32_t open_tick = 0, ticks_counted = 0, n_watch = 0;
    int32_t sent_done = -1;                      // from-CSR form: the tick whose sends a get folded
    TickTimer timer;                             // the passes of the timed ticks
    LedgerBufs led;
    DevBuf<int32_t> watch_slot, psize;           // [n] each; psize: the partial view's payload sizes

    void release() { release_all(led, watch_slot, psize); }
};

// The engine core with the eight probes' state: what gsp_scale and gsp_pview derive from.
struct ProbeCore : EngineCore {
    CensusBufs census;
    AuditBufs audit;
    ReachBufs reach;
    ReachMultiBufs reach_multi;
    ClusterBufs cluster;
    ComponentsBufs components;
    RumorBufs rumor;
    DetectBufs detect;
    TrafficBufs traffic;
};

// the engine's sync: collect_timing, and the per-tick probes' timed spans into their kernel_ms
inline int collect_timing(ProbeCore &c) {
    if (int rc = collect_timing(static_cast<EngineCore &>(c))) return rc;
    for (TickTimer *t : {&c.rumor.timer, &c.detect.timer, &c.traffic.timer})
        if (int rc = t->collect(c)) return rc;
    return GSP_OK;
}

// Destroy, after the engine has synchronised the stream and released its shards.  The pending
// events go back to the pool while it exists: engine_close then destroys every event once.
inline void engine_close(ProbeCore &c) {
    for (TickTimer *t : {&c.rumor.timer, &c.detect.timer, &c.traffic.timer}) t->give_back(c);
    release_all(c.census, c.audit, c.reach, c.reach_multi, c.cluster, c.components, c.rumor, c.detect, c.traffic);
    engine_close(static_cast<EngineCore &>(c));
}

// The close of the per-tick probe whose state is s->*probe (`what`: "trace" / "ledger"), which
// is left as constructed (closed, counters and kernel_ms zero): what an open starts from.
template <class E, class B>
int probe_close(E *s, const char *fn, B ProbeCore::*probe, const char *what) {
    if (int rc = probe_enter(s, fn)) return rc;
    B &b = s->*probe;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no %s is open", fn, what);
    GSP_HIP(hipStreamSynchronize(s->st));          // no queued launch still uses the buffers
    b.timer.give_back(*s);
    b.release();
    b = B{};
    return GSP_OK;
}

// ---- the snapshot probes ----

// The census of the engine's current tick T (gossip.h, census_kernels.hpp).  `packed`: the
// engine's kernels count into census.counts (partial view) instead of listed / fresh.
// launch(shard) adds that shard's share -- its rows, its columns -- to the zeroed arrays; with a
// communicator the arrays are then all-reduced (SUM; MAX for max_hb).
template <class E, class Launch>
int census_run(E &s, const char *fn, bool packed, int32_t age_limit, uint32_t *listed, uint32_t *fresh,
               uint32_t *max_hb, uint8_t *state, gsp_census_info *info, Launch launch) {
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]", fn,
                age_limit);
    const size_t n = size_t(s.p.n);
    const int32_t T = s.tick;
    CensusBufs &c = s.census;
    if (!c.span.ready) {               // first call
        GSP_HIP(c.max_hb.alloc(n));
        if (packed) GSP_HIP(c.counts.alloc(n));
        else {
            GSP_HIP(c.listed.alloc(n));
            GSP_HIP(c.fresh.alloc(n));
        }
        GSP_HIP(c.span.arm());
    }
    c.h32.resize(packed ? n : 3 * n);
    c.h64.resize(packed ? n : 0);
    GSP_HIP(hipMemsetAsync(c.max_hb.p, 0, n * 4, s.st));
    if (packed) GSP_HIP(hipMemsetAsync(c.counts.p, 0, n * 8, s.st));
    else {
        GSP_HIP(hipMemsetAsync(c.listed.p, 0, n * 4, s.st));
        GSP_HIP(hipMemsetAsync(c.fresh.p, 0, n * 4, s.st));
    }
    GSP_HIP(c.span.begin(s));
    for (auto &sh : s.local)
        if (int rc = launch(sh)) return rc;
    GSP_HIP(c.span.end(s));
    if (s.comm) {
        if (packed) GSP_NCCL(ncclAllReduce(c.counts.p, c.counts.p, n, ncclUint64, ncclSum, s.comm, s.st));
        else {
            GSP_NCCL(ncclAllReduce(c.listed.p, c.listed.p, n, ncclUint32, ncclSum, s.comm, s.st));
            GSP_NCCL(ncclAllReduce(c.fresh.p, c.fresh.p, n, ncclUint32, ncclSum, s.comm, s.st));
        }
        GSP_NCCL(ncclAllReduce(c.max_hb.p, c.max_hb.p, n, ncclUint32, ncclMax, s.comm, s.st));
    }
    uint32_t *h_hb = c.h32.data();
    GSP_HIP(hipMemcpyAsync(h_hb, c.max_hb.p, n * 4, hipMemcpyDeviceToHost, s.st));
    if (packed) GSP_HIP(hipMemcpyAsync(c.h64.data(), c.counts.p, n * 8, hipMemcpyDeviceToHost, s.st));
    else {
        GSP_HIP(hipMemcpyAsync(h_hb + n, c.listed.p, n * 4, hipMemcpyDeviceToHost, s.st));
        GSP_HIP(hipMemcpyAsync(h_hb + 2 * n, c.fresh.p, n * 4, hipMemcpyDeviceToHost, s.st));
    }
    GSP_HIP(hipStreamSynchronize(s.st));
    int64_t entries = 0;
    int32_t alive = 0;
    for (size_t x = 0; x < n; ++x) {
        const uint32_t l = packed ? uint32_t(c.h64[x]) : h_hb[n + x];
        const uint32_t f = packed ? uint32_t(c.h64[x] >> 32) : h_hb[2 * n + x];
        const uint8_t st = node_state(s, T, x);
        entries += l;
        alive += st == 1;
        if (listed) listed[x] = l;
        if (fresh) fresh[x] = f;
        if (max_hb) max_hb[x] = h_hb[x];
        if (state) state[x] = st;
    }
    if (info) {
        *info = gsp_census_info{T, s.p.n, age_limit, alive, entries, 0.0};
        GSP_HIP(c.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// The view audit of the engine's current tick T (gossip.h, audit_kernels.hpp).  `full`: the full
// view, whose kernel reads the fingerprint table.  The prologue writes the call's truth (alive
// bitmap, fp table); launch(shard) adds that shard's share -- its rows, its columns -- to the
// zeroed arrays; with a communicator the arrays are then all-reduced (SUM for the counts and the
// wrapping print, MAX for age_max).  The observer's own fingerprint joins print in the readback
// loop.
template <class E, class Launch>
int audit_run(E &s, const char *fn, bool full, int32_t age_limit, uint32_t *size, uint32_t *dead,
              uint32_t *suspect, uint32_t *age_sum, uint8_t *age_max, uint64_t *print, uint8_t *state,
              gsp_audit_info *info, Launch launch) {
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]", fn,
                age_limit);
    const size_t n = size_t(s.p.n);
    const int32_t T = s.tick;
    AuditBufs &b = s.audit;
    if (!b.span.ready) {               // first call
        GSP_HIP(b.arr.alloc(size_t(kAuditFields) * n));
        GSP_HIP(b.print.alloc(n));
        GSP_HIP(b.alive.alloc((n + 7) / 8));
        if (full) GSP_HIP(b.fp.alloc(n));
        GSP_HIP(b.span.arm());
    }
    b.h32.resize(size_t(kAuditFields) * n);
    b.h64.resize(n);
    GSP_HIP(hipMemsetAsync(b.arr.p, 0, size_t(kAuditFields) * n * 4, s.st));
    GSP_HIP(hipMemsetAsync(b.print.p, 0, n * 8, s.st));
    GSP_HIP(b.span.begin(s));
    AuditTruthArgs tr{};
    tr.n = s.p.n;
    tr.tick = T;
    tr.fail_tick = s.local[0].fail_tick.p;
    tr.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    tr.alive = b.alive.p;
    tr.fp = full ? b.fp.p : nullptr;
    GSP_HIP(launch_audit_truth(tr, s.st));
    for (auto &sh : s.local)
        if (int rc = launch(sh)) return rc;
    GSP_HIP(b.span.end(s));
    if (s.comm) {
        uint32_t *mx = b.arr.p + size_t(kAudAgeMax) * n;
        GSP_NCCL(ncclAllReduce(b.arr.p, b.arr.p, size_t(kAudAgeMax) * n, ncclUint32, ncclSum, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(mx, mx, n, ncclUint32, ncclMax, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(b.print.p, b.print.p, n, ncclUint64, ncclSum, s.comm, s.st));
    }
    GSP_HIP(hipMemcpyAsync(b.h32.data(), b.arr.p, size_t(kAuditFields) * n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipMemcpyAsync(b.h64.data(), b.print.p, n * 8, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    const uint32_t *h = b.h32.data();
    int64_t entries = 0;
    int32_t alive = 0;
    for (size_t r = 0; r < n; ++r) {
        const uint8_t st = node_state(s, T, r);
        entries += h[size_t(kAudSize) * n + r];
        alive += st == 1;
        if (size) size[r] = h[size_t(kAudSize) * n + r];
        if (dead) dead[r] = h[size_t(kAudDead) * n + r];
        if (suspect) suspect[r] = h[size_t(kAudSuspect) * n + r];
        if (age_sum) age_sum[r] = h[size_t(kAudAgeSum) * n + r];
        if (age_max) age_max[r] = uint8_t(h[size_t(kAudAgeMax) * n + r]);
        if (print) print[r] = st == 1 ? uint64_t(b.h64[r]) + audit_fp(uint32_t(r)) : 0;
        if (state) state[r] = st;
    }
    if (info) {
        *info = gsp_audit_info{T, s.p.n, age_limit, alive, entries, 0.0};
        GSP_HIP(b.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// The overlay reach of the engine's current tick T (gossip.h, reach_kernels.hpp): a
// level-synchronous BFS, one launch per local shard and level.  launch(shard, common, to) runs
// that shard's share of level common.cur -- its rows, its columns; with a communicator hops is
// then all-reduced (MIN).  After each level reach_level counts the nodes just reached into a
// device word the host waits for: one host wait per level, and the loop ends at the first level
// that reaches nobody.  The count word is cumulative, so it is zeroed once per call.
template <class E, class Launch>
int reach_run(E &s, const char *fn, int32_t direction, int32_t age_limit, const int32_t *sources,
              int32_t n_sources, int32_t *hops, uint8_t *state, gsp_reach_info *info, Launch launch) {
    GSP_REQUIRE(direction == GSP_REACH_FROM || direction == GSP_REACH_TO, GSP_ERR_INVALID,
                "%s: direction=%d is neither GSP_REACH_FROM (0) nor GSP_REACH_TO (1)", fn, direction);
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]",
                fn, age_limit);
    if (int rc = check_ids(fn, "sources", sources, n_sources, s.p.n)) return rc;
    const size_t n = size_t(s.p.n), words = reach_bitmap_words(s.p.n);
    const int32_t T = s.tick;
    ReachBufs &b = s.reach;
    if (!b.span.ready) {               // first call
        GSP_HIP(b.hops.alloc(n));
        GSP_HIP(b.count.alloc(1));
        GSP_HIP(b.front.alloc(words));
        GSP_HIP(b.todo.alloc(words));
        if (!b.h_count) GSP_HIP(hipHostMalloc(reinterpret_cast<void **>(&b.h_count), 4));
        GSP_HIP(b.span.arm());
    }
    GSP_HIP(b.src.alloc(size_t(n_sources)));

    ReachCommon c{};
    c.n = s.p.n;
    c.tick = T;
    c.age_limit = age_limit;
    c.fail_tick = s.local[0].fail_tick.p;
    c.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    c.hops = b.hops.p;
    c.front = b.front.p;
    c.todo = b.todo.p;

    // the nodes at `level`, from the cumulative count (waits for the stream)
    uint32_t reached = 0;
    auto count_level = [&](uint32_t level, uint32_t *found) -> int {
        GSP_HIP(launch_reach_level(c, level, b.front.p, b.todo.p, b.count.p, s.st));
        GSP_HIP(hipMemcpyAsync(b.h_count, b.count.p, 4, hipMemcpyDeviceToHost, s.st));
        GSP_HIP(hipStreamSynchronize(s.st));
        *found = *b.h_count - reached;
        reached = *b.h_count;
        return GSP_OK;
    };

    GSP_HIP(b.span.begin(s));
    GSP_HIP(hipMemcpyAsync(b.src.p, sources, size_t(n_sources) * 4, hipMemcpyHostToDevice, s.st));
    GSP_HIP(hipMemsetAsync(b.hops.p, 0xFF, n * 4, s.st));          // kReachUnset
    GSP_HIP(hipMemsetAsync(b.count.p, 0, 4, s.st));
    GSP_HIP(launch_reach_seed(b.src.p, n_sources, c, s.st));
    uint32_t level0 = 0, found = 0;
    if (int rc = count_level(0, &level0)) return rc;
    int32_t depth = -1, levels = 0;
    int64_t sum_hops = 0;
    found = level0;
    while (found) {
        depth = int32_t(c.cur);
        sum_hops += int64_t(found) * depth;
        for (auto &sh : s.local)
            if (int rc = launch(sh, c, direction == GSP_REACH_TO)) return rc;
        if (s.comm) GSP_NCCL(ncclAllReduce(b.hops.p, b.hops.p, n, ncclUint32, ncclMin, s.comm, s.st));
        ++levels;
        if (int rc = count_level(c.cur + 1, &found)) return rc;
        ++c.cur;
    }
    GSP_HIP(b.span.end(s));
    // unset is 0xFFFFFFFF: -1 as the caller's int32
    if (hops) GSP_HIP(hipMemcpyAsync(hops, b.hops.p, n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0;
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = node_state(s, T, x);
        alive += st == 1;
        if (state) state[x] = st;
    }
    if (info) {
        *info = gsp_reach_info{T, s.p.n, age_limit, direction, alive, int32_t(level0), int32_t(reached),
                               depth, levels, sum_hops, 0.0};
        GSP_HIP(b.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// The multi-source reach of the engine's current tick T (gossip.h, reach_multi_kernels.hpp): up to
// 64 single-source BFS trees, tree b from sources[b], one launch per local shard and level for all
// of them.  launch(shard, common, to) ORs that shard's share of level common.cur into next; with a
// communicator every rank's next is all-gathered and ORed down (RCCL has no bitwise-OR
// reduction), so every rank's level kernel admits and counts the same bits.  The level kernel
// adds the nodes each tree just reached to 64 cumulative counters the host waits for: one host
// wait per level, and the loop ends at the first level that sets no bit.  Every per-source output
// comes from those counters; only seen and hops are read back from the device.
template <class E, class Launch>
int reach_multi_run(E &s, const char *fn, int32_t direction, int32_t age_limit, const int32_t *sources,
                    int32_t n_sources, uint64_t *seen, int32_t *hops, int32_t *reached, int32_t *ecc,
                    int64_t *sum_hops, uint32_t *level_sizes, int32_t level_cap, uint8_t *state,
                    gsp_reach_multi_info *info, Launch launch) {
    GSP_REQUIRE(direction == GSP_REACH_FROM || direction == GSP_REACH_TO, GSP_ERR_INVALID,
                "%s: direction=%d is neither GSP_REACH_FROM (0) nor GSP_REACH_TO (1)", fn, direction);
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]",
                fn, age_limit);
    GSP_REQUIRE(n_sources >= 1 && n_sources <= GSP_REACH_MAX_SOURCES, GSP_ERR_INVALID,
                "%s: n_sources=%d outside [1,%d]", fn, n_sources, GSP_REACH_MAX_SOURCES);
    if (int rc = check_ids(fn, "sources", sources, n_sources, s.p.n)) return rc;
    GSP_REQUIRE(level_cap >= 0 || !level_sizes, GSP_ERR_INVALID, "%s: level_cap=%d", fn, level_cap);
    const size_t n = size_t(s.p.n), words = reach_bitmap_words(s.p.n), nodes = reach_multi_nodes(s.p.n);
    const size_t K = size_t(n_sources);
    const int32_t T = s.tick;
    ReachMultiBufs &b = s.reach_multi;
    int world = 1;
    if (s.comm) GSP_NCCL(ncclCommCount(s.comm, &world));
    if (!b.span.ready) {               // first call
        GSP_HIP(b.seen.alloc(nodes));
        GSP_HIP(b.front.alloc(nodes));
        GSP_HIP(b.next.alloc(nodes));
        GSP_HIP(b.hot.alloc(words));
        GSP_HIP(b.open.alloc(words));
        GSP_HIP(b.count.alloc(kReachMultiMax));
        GSP_HIP(b.src.alloc(kReachMultiMax));
        if (s.comm) GSP_HIP(b.stage.alloc(size_t(world) * nodes));
        if (!b.h_count)
            GSP_HIP(hipHostMalloc(reinterpret_cast<void **>(&b.h_count), size_t(kReachMultiMax) * 4));
        GSP_HIP(b.span.arm());
    }
    if (hops) GSP_HIP(b.hops.alloc(K * n));

    uint64_t want = 0;
    int32_t alive_sources = 0;
    for (size_t i = 0; i < K; ++i)
        if (node_state(s, T, size_t(sources[i])) == 1) {
            want |= 1ull << i;
            ++alive_sources;
        }

    ReachMultiLevelArgs lv{};
    lv.n = s.p.n;
    lv.tick = T;
    lv.n_sources = n_sources;
    lv.want = want;
    lv.fail_tick = s.local[0].fail_tick.p;
    lv.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    lv.seen = b.seen.p;
    lv.front = b.front.p;
    lv.next = b.next.p;
    lv.hot = b.hot.p;
    lv.open = b.open.p;
    lv.count = b.count.p;
    lv.hops = hops ? b.hops.p : nullptr;

    ReachMultiCommon c{};
    c.n = s.p.n;
    c.tick = T;
    c.age_limit = age_limit;
    c.want = want;
    c.seen = b.seen.p;
    c.front = b.front.p;
    c.next = b.next.p;
    c.hot = b.hot.p;
    c.open = b.open.p;

    // per tree: the cumulative count as of the last level, and what the outputs are built from
    uint32_t have[kReachMultiMax] = {0};
    int32_t h_ecc[kReachMultiMax];
    int64_t h_sum[kReachMultiMax] = {0};
    std::fill(h_ecc, h_ecc + kReachMultiMax, -1);
    if (level_sizes) std::fill(level_sizes, level_sizes + K * size_t(level_cap), 0u);

    // admit what was ORed into next as `level` and count it per tree (waits for the stream)
    auto admit = [&](uint32_t level, uint64_t *found) -> int {
        lv.level = level;
        GSP_HIP(launch_reach_multi_level(lv, s.st));
        GSP_HIP(hipMemcpyAsync(b.h_count, b.count.p, size_t(kReachMultiMax) * 4, hipMemcpyDeviceToHost, s.st));
        GSP_HIP(hipStreamSynchronize(s.st));
        *found = 0;
        for (size_t i = 0; i < K; ++i) {
            const uint32_t got = b.h_count[i] - have[i];
            have[i] = b.h_count[i];
            if (!got) continue;
            *found += got;
            h_ecc[i] = int32_t(level);
            h_sum[i] += int64_t(got) * int64_t(level);
            if (level_sizes && level < uint32_t(level_cap)) level_sizes[i * size_t(level_cap) + level] = got;
        }
        return GSP_OK;
    };

    GSP_HIP(b.span.begin(s));
    GSP_HIP(hipMemcpyAsync(b.src.p, sources, K * 4, hipMemcpyHostToDevice, s.st));
    GSP_HIP(hipMemsetAsync(b.seen.p, 0, nodes * 8, s.st));
    GSP_HIP(hipMemsetAsync(b.front.p, 0, nodes * 8, s.st));
    GSP_HIP(hipMemsetAsync(b.next.p, 0, nodes * 8, s.st));
    GSP_HIP(hipMemsetAsync(b.count.p, 0, size_t(kReachMultiMax) * 4, s.st));
    if (hops) GSP_HIP(hipMemsetAsync(b.hops.p, 0xFF, K * n * 4, s.st));          // -1: not reached
    GSP_HIP(launch_reach_multi_seed(b.src.p, lv, s.st));
    uint64_t found = 0;
    if (int rc = admit(0, &found)) return rc;
    int32_t depth = -1, levels = 0;
    uint32_t cur = 0;
    while (found) {
        depth = int32_t(cur);
        for (auto &sh : s.local)
            if (int rc = launch(sh, c, direction == GSP_REACH_TO)) return rc;
        if (s.comm) {
            GSP_NCCL(ncclAllGather(b.next.p, b.stage.p, nodes, ncclUint64, s.comm, s.st));
            GSP_HIP(launch_reach_multi_fold(b.stage.p, world, nodes, b.next.p, s.st));
        }
        ++levels;
        if (int rc = admit(cur + 1, &found)) return rc;
        ++cur;
    }
    GSP_HIP(b.span.end(s));
    if (seen) GSP_HIP(hipMemcpyAsync(seen, b.seen.p, n * 8, hipMemcpyDeviceToHost, s.st));
    if (hops) GSP_HIP(hipMemcpyAsync(hops, b.hops.p, K * n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0;
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = node_state(s, T, x);
        alive += st == 1;
        if (state) state[x] = st;
    }
    int64_t pairs = 0, total = 0;
    for (size_t i = 0; i < K; ++i) {
        pairs += have[i];
        total += h_sum[i];
        if (reached) reached[i] = int32_t(have[i]);
        if (ecc) ecc[i] = h_ecc[i];
        if (sum_hops) sum_hops[i] = h_sum[i];
    }
    if (info) {
        *info = gsp_reach_multi_info{T, s.p.n, age_limit, direction, alive, n_sources, alive_sources,
                                     depth, levels, 0, pairs, total, 0.0};
        GSP_HIP(b.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// The overlay clustering of the engine's current tick T (gossip.h, cluster_kernels.hpp), for up
// to 64 observers.  The prologue writes the call's alive bitmap; launch(shard, common, phase) runs
// that shard's share -- its rows, its columns -- of the member pass (kClusterMembers) and then of
// the link and mutual passes (kClusterLinks), which read the member words the first phase left.
// With a communicator the member words are all-reduced between the phases.  SUM is exact there:
// the words start from zero, and bit b of member[x] is written only by the one rank that holds
// both observers[b]'s row and column x, so no two ranks ever add the same bit and no carry
// exists.  The counters, zeroed per call, are all-reduced (SUM) in place after the second phase.
// `rows` and the sums of the info come from the host's copy of member and the counters.
template <class E, class Launch>
int cluster_run(E &s, const char *fn, int32_t age_limit, const int32_t *observers, int32_t n_observers,
                uint64_t *member, uint32_t *degree, uint64_t *links, uint32_t *mutual, uint8_t *state,
                gsp_cluster_info *info, Launch launch) {
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]", fn,
                age_limit);
    GSP_REQUIRE(n_observers >= 1 && n_observers <= GSP_CLUSTER_MAX_OBSERVERS, GSP_ERR_INVALID,
                "%s: n_observers=%d outside [1,%d]", fn, n_observers, GSP_CLUSTER_MAX_OBSERVERS);
    if (int rc = check_ids(fn, "observers", observers, n_observers, s.p.n)) return rc;
    const size_t n = size_t(s.p.n), nodes = cluster_nodes(s.p.n), K = size_t(n_observers);
    const size_t counters = kClusterCtrWords;
    const int32_t T = s.tick;
    ClusterBufs &b = s.cluster;
    if (!b.span.ready) {               // first call
        GSP_HIP(b.member.alloc(nodes));
        GSP_HIP(b.alive.alloc(nodes / 8));
        GSP_HIP(b.ctr.alloc(counters));
        GSP_HIP(b.obs.alloc(kClusterMax));
        // the prologue rewrites the bytes below (n + 7) / 8 per call; the rest stay 0
        GSP_HIP(hipMemsetAsync(b.alive.p, 0, nodes / 8, s.st));
        GSP_HIP(b.span.arm());
    }
    b.h_member.resize(n);
    b.h_ctr.resize(counters);

    uint64_t want = 0;
    int32_t alive_observers = 0;
    int32_t h_obs[kClusterMax] = {0};
    for (size_t i = 0; i < K; ++i) {
        h_obs[i] = observers[i];
        if (node_state(s, T, size_t(observers[i])) == 1) {
            want |= 1ull << i;
            ++alive_observers;
        }
    }

    ClusterCommon c{};
    c.n = s.p.n;
    c.tick = T;
    c.age_limit = age_limit;
    c.n_observers = n_observers;
    c.want = want;
    c.obs = b.obs.p;
    c.alive = b.alive.p;
    c.member = b.member.p;
    c.ctr = b.ctr.p;

    GSP_HIP(hipMemsetAsync(b.member.p, 0, nodes * 8, s.st));
    GSP_HIP(hipMemsetAsync(b.ctr.p, 0, counters * 8, s.st));
    GSP_HIP(b.span.begin(s));
    // h_obs is on this frame: the stream is synchronised before the call returns
    GSP_HIP(hipMemcpyAsync(b.obs.p, h_obs, size_t(kClusterMax) * 4, hipMemcpyHostToDevice, s.st));
    AuditTruthArgs tr{};
    tr.n = s.p.n;
    tr.tick = T;
    tr.fail_tick = s.local[0].fail_tick.p;
    tr.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    tr.alive = b.alive.p;
    tr.fp = nullptr;
    GSP_HIP(launch_audit_truth(tr, s.st));
    for (auto &sh : s.local)
        if (int rc = launch(sh, c, int(kClusterMembers))) return rc;
    if (s.comm) GSP_NCCL(ncclAllReduce(b.member.p, b.member.p, nodes, ncclUint64, ncclSum, s.comm, s.st));
    for (auto &sh : s.local)
        if (int rc = launch(sh, c, int(kClusterLinks))) return rc;
    GSP_HIP(b.span.end(s));
    if (s.comm) GSP_NCCL(ncclAllReduce(b.ctr.p, b.ctr.p, counters, ncclUint64, ncclSum, s.comm, s.st));
    GSP_HIP(hipMemcpyAsync(b.h_member.data(), b.member.p, n * 8, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipMemcpyAsync(b.h_ctr.data(), b.ctr.p, counters * 8, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0, rows = 0;
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = node_state(s, T, x);
        alive += st == 1;
        rows += b.h_member[x] != 0;
        if (member) member[x] = b.h_member[x];
        if (state) state[x] = st;
    }
    const unsigned long long *h = b.h_ctr.data();
    int64_t sum_degree = 0, sum_links = 0, sum_mutual = 0;
    for (size_t i = 0; i < K; ++i) {
        unsigned long long d = 0, l = 0, m = 0;               // the copies of the counters, summed
        for (size_t slot = 0; slot < size_t(kClusterSlots); ++slot) {
            const unsigned long long *copy = h + slot * kClusterCounters * kClusterMax;
            d += copy[size_t(kCluDegree) * kClusterMax + i];
            l += copy[size_t(kCluLinks) * kClusterMax + i];
            m += copy[size_t(kCluMutual) * kClusterMax + i];
        }
        sum_degree += int64_t(d);
        sum_links += int64_t(l);
        sum_mutual += int64_t(m);
        if (degree) degree[i] = uint32_t(d);
        if (links) links[i] = uint64_t(l);
        if (mutual) mutual[i] = uint32_t(m);
    }
    if (info) {
        *info = gsp_cluster_info{T, s.p.n, age_limit, alive, n_observers, alive_observers, rows, 0,
                                 sum_degree, sum_links, sum_mutual, 0.0};
        GSP_HIP(b.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// The overlay components of the engine's current tick T (gossip.h, components_kernels.hpp).  A
// round is one sweep -- launch(shard, common) for every local shard: its rows, its columns --
// then, with a communicator, the all-reduce of what the sweep moved (weak: lab, MIN; strong: fcol,
// bcol and, after a turn's first sweep, has_in / has_out, MAX; every word only ever moves one
// way, so MIN / MAX of the ranks' words is what one rank sweeping all shards would hold), the jump
// kernel, and one host wait for the counters.  The jump runs on the reduced arrays, so every rank
// reads the same checksum and takes the same branch.  Weak ends with the round that repeats the
// checksum; strong then makes a turn, and ends when a turn leaves nobody unassigned.  The counts
// of the info are made from the host's copy of the labels.
template <class E, class Launch>
int components_run(E &s, const char *fn, int32_t kind, int32_t age_limit, int32_t max_sweeps, int32_t *label,
                   uint8_t *state, gsp_components_info *info, Launch launch) {
    GSP_REQUIRE(kind == GSP_COMPONENTS_WEAK || kind == GSP_COMPONENTS_STRONG, GSP_ERR_INVALID,
                "%s: kind=%d is neither GSP_COMPONENTS_WEAK (0) nor GSP_COMPONENTS_STRONG (1)", fn, kind);
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]", fn,
                age_limit);
    GSP_REQUIRE(max_sweeps >= 0, GSP_ERR_INVALID, "%s: max_sweeps=%d is negative", fn, max_sweeps);
    const int32_t cap = max_sweeps ? max_sweeps : GSP_COMPONENTS_DEFAULT_SWEEPS;
    const size_t n = size_t(s.p.n), nodes = components_nodes(s.p.n);
    const int32_t T = s.tick;
    const bool weak = kind == GSP_COMPONENTS_WEAK;
    ComponentsBufs &b = s.components;
    if (!b.span.ready) {               // first call
        GSP_HIP(b.arr.alloc(size_t(kCompArrays) * nodes));
        GSP_HIP(b.active.alloc(nodes / 64));
        GSP_HIP(b.ctr.alloc(kCompCounters));
        if (!b.h_ctr)
            GSP_HIP(hipHostMalloc(reinterpret_cast<void **>(&b.h_ctr), size_t(kCompCounters) * 8));
        GSP_HIP(b.span.arm());
    }
    b.h_label.resize(n);
    auto arr = [&](int which) { return b.arr.p + size_t(which) * nodes; };

    CompCommon c{};
    c.n = s.p.n;
    c.tick = T;
    c.age_limit = age_limit;
    c.kind = kind;
    c.fail_tick = s.local[0].fail_tick.p;
    c.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    c.active = b.active.p;
    c.lab = arr(kCompLab);
    c.fcol = arr(kCompFcol);
    c.bcol = arr(kCompBcol);
    c.pf = arr(kCompPf);
    c.pb = arr(kCompPb);
    c.has_in = arr(kCompIn);
    c.has_out = arr(kCompOut);
    c.comp = arr(kCompComp);
    c.ctr = b.ctr.p;

    // the counters since the last wait (waits for the stream).  Only the n-length kernels count,
    // and they run on the reduced arrays: every rank holds the same counters, nothing to reduce.
    unsigned long long seen[kCompCounters] = {0}, got[kCompCounters] = {0};
    int32_t sweeps = 0, rounds = 0;
    auto wait = [&]() -> int {
        GSP_HIP(hipMemcpyAsync(b.h_ctr, b.ctr.p, size_t(kCompCounters) * 8, hipMemcpyDeviceToHost, s.st));
        GSP_HIP(hipStreamSynchronize(s.st));
        ++rounds;
        for (int i = 0; i < kCompCounters; ++i) {
            got[i] = b.h_ctr[i] - seen[i];
            seen[i] = b.h_ctr[i];
        }
        return GSP_OK;
    };
    auto reduce = [&](uint32_t *p, size_t words, ncclRedOp_t op) -> int {
        if (s.comm) GSP_NCCL(ncclAllReduce(p, p, words, ncclUint32, op, s.comm, s.st));
        return GSP_OK;
    };
    // one round; *sum: the checksum after it
    auto round = [&](unsigned long long *sum) -> int {
        for (auto &sh : s.local)
            if (int rc = launch(sh, c)) return rc;
        ++sweeps;
        if (weak) {
            if (int rc = reduce(c.lab, nodes, ncclMin)) return rc;
        } else {
            if (int rc = reduce(c.fcol, 2 * nodes, ncclMax)) return rc;               // fcol, bcol
            if (c.first)
                if (int rc = reduce(c.has_in, 2 * nodes, ncclMax)) return rc;         // has_in, has_out
        }
        GSP_HIP(launch_components_jump(c, s.st));
        if (int rc = wait()) return rc;
        *sum = got[kCompSum];
        return GSP_OK;
    };

    GSP_HIP(b.span.begin(s));
    GSP_HIP(hipMemsetAsync(b.ctr.p, 0, size_t(kCompCounters) * 8, s.st));
    bool converged = false;
    if (weak) {
        GSP_HIP(launch_components_weak_init(c, s.st));
        unsigned long long last = 0, sum = 0;
        bool based = false;
        while (!converged && sweeps < cap) {
            if (int rc = round(&sum)) return rc;
            if (!based) last = got[kCompBase];           // the init's checksum came with this wait
            based = true;
            converged = sum == last;
            last = sum;
        }
    } else {
        GSP_HIP(hipMemsetAsync(c.comp, 0xFF, nodes * 4, s.st));       // kCompNone
        bool opening = true, turn = true;
        unsigned long long last = 0, sum = 0;
        while (!converged && sweeps < cap) {
            if (turn) GSP_HIP(launch_components_turn(c, opening, s.st));
            c.first = turn;
            if (int rc = round(&sum)) return rc;
            if (turn) {                                   // the turn's counters came with this wait
                last = got[kCompBase];
                converged = got[kCompLeft] == 0;
            }
            opening = false;
            turn = sum == last;                           // an idle round: the turn is over
            last = sum;
        }
        if (converged) GSP_HIP(launch_components_canon(c, s.st));
    }
    GSP_HIP(b.span.end(s));
    if (converged)
        GSP_HIP(hipMemcpyAsync(b.h_label.data(), c.lab, n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0, components = 0, largest = 0, largest_label = -1, singletons = 0;
    b.h_size.assign(converged ? n : 0, 0u);
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = node_state(s, T, x);
        alive += st == 1;
        if (state) state[x] = st;
        // kCompNone is -1 as the caller's int32
        if (label) label[x] = converged ? int32_t(b.h_label[x]) : (st == 1 ? int32_t(x) : -1);
        if (converged && b.h_label[x] < n) ++b.h_size[b.h_label[x]];
    }
    for (size_t x = 0; x < b.h_size.size(); ++x) {
        const uint32_t sz = b.h_size[x];
        components += sz != 0;
        singletons += sz == 1;
        if (sz > uint32_t(largest)) {
            largest = int32_t(sz);
            largest_label = int32_t(x);
        }
    }
    if (info) {
        *info = gsp_components_info{T,       s.p.n,         age_limit,  kind,   alive,  components,
                                    largest, largest_label, singletons, sweeps, rounds, converged ? 1 : 0,
                                    0.0};
        GSP_HIP(b.span.elapsed(s, &info->kernel_ms));
    }
    return GSP_OK;
}

// ---- the rumor trace (gossip.h "Rumor trace", rumor_kernels.hpp) ----
// Who computes what: without row shards (fused, column tiles, column shards across ranks) every
// engine holds the job's whole receiver CSR in local[0] and runs all n rows from it, so ranks
// need no exchange.  Row shards write their own rows of the shared know; across ranks know_cur is
// zeroed, the held rows are written and the n words are all-reduced (MAX is exact: only the
// holder writes a word, and a mask only gains bits, so a superset is never the smaller number),
// while heard / known stay per rank until a get all-reduces them (MIN over an unset 0xFFFFFFFF,
// SUM) into a staging buffer.

template <class E>
int rumor_open(E *s, const char *fn, int32_t rumors) {
    if (int rc = probe_enter(s, fn)) return rc;
    RumorBufs &b = s->rumor;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a trace is already open (%d rumors)", fn, b.rumors);
    GSP_REQUIRE(rumors >= 1 && rumors <= kRumorMax, GSP_ERR_INVALID, "%s: rumors=%d outside [1,%d]", fn,
                rumors, kRumorMax);
    const size_t n = size_t(s->p.n), span = size_t(s->p.max_ticks) + 1;
    GSP_HIP(b.know.alloc(2 * n));
    GSP_HIP(b.heard.alloc(size_t(rumors) * n));
    GSP_HIP(b.known.alloc(size_t(rumors) * span));
    if (s->rowmode && s->comm) GSP_HIP(b.red.alloc(n + span));
    GSP_HIP(hipMemsetAsync(b.know.p, 0, 2 * n * 4, s->st));
    GSP_HIP(hipMemsetAsync(b.heard.p, 0xFF, size_t(rumors) * n * 4, s->st));     // -1: not heard
    GSP_HIP(hipMemsetAsync(b.known.p, 0, size_t(rumors) * span * 4, s->st));
    b.seed_tick.assign(size_t(rumors), -1);
    b.seeded.assign(size_t(rumors), {});
    b.rumors = rumors;
    b.open = true;
    return GSP_OK;
}

// The seed rule at the engine's tick T, stream-ordered.  The host keeps the distinct alive
// sources per rumor from its own copy of the schedule.
template <class E>
int rumor_seed(E *s, const char *fn, int32_t rumor, const int32_t *sources, int32_t n_sources) {
    if (int rc = probe_enter(s, fn)) return rc;
    RumorBufs &b = s->rumor;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no trace is open", fn);
    GSP_REQUIRE(rumor >= 0 && rumor < b.rumors, GSP_ERR_INVALID, "%s: rumor=%d outside [0,%d)", fn, rumor,
                b.rumors);
    if (int rc = check_ids(fn, "sources", sources, n_sources, s->p.n)) return rc;
    const size_t n = size_t(s->p.n);
    const int32_t T = s->tick;
    GSP_HIP(b.src.alloc(size_t(n_sources)));
    GSP_HIP(hipMemcpyAsync(b.src.p, sources, size_t(n_sources) * 4, hipMemcpyHostToDevice, s->st));
    RumorSeedArgs a{};
    a.n = s->p.n;
    a.tick = T;
    a.rumor = rumor;
    a.lo = 0;
    a.hi = s->p.n;
    if (s->rowmode && s->comm) {                     // this rank records its own rows only
        a.lo = s->local.front().row0;
        a.hi = s->local.back().row0 + s->local.back().rows;
    }
    a.sources = b.src.p;
    a.n_sources = n_sources;
    a.fail_tick = s->local[0].fail_tick.p;
    a.start_tick = s->joins ? s->local[0].start_tick.p : nullptr;
    a.know = b.know.p + size_t(T & 1) * n;
    a.heard = b.heard.p + size_t(rumor) * n;
    a.known = b.known.p + size_t(rumor) * (size_t(s->p.max_ticks) + 1) + size_t(T);
    GSP_HIP(launch_rumor_seed(a, s->st));
    GSP_HIP(hipStreamSynchronize(s->st));           // seeding is between steps: the caller's array
                                                   // and b.src are free again on return
    std::vector<int32_t> &set = b.seeded[size_t(rumor)];
    for (int32_t i = 0; i < n_sources; ++i)
        if (node_state(*s, T, size_t(sources[i])) == 1) set.push_back(sources[i]);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    if (!set.empty() && b.seed_tick[size_t(rumor)] < 0) b.seed_tick[size_t(rumor)] = T;
    return GSP_OK;
}

// Tick t of an open trace, on the engine's stream with no host wait: called where the receiver
// CSR of t is complete and before the tick kernels.  fill(shard, args) adds what only the engine
// knows (the partial view's receipt records).
template <class E, class Fill>
int rumor_step(E *s, int32_t t, Fill fill) {
    RumorBufs &b = s->rumor;
    const size_t n = size_t(s->p.n);
    const uint32_t *prev = b.know.p + size_t((t + 1) & 1) * n;
    uint32_t *cur = b.know.p + size_t(t & 1) * n;
    const bool reduce = s->rowmode && s->comm;
    if (int rc = b.timer.timed(s, [&]() -> int {
            if (reduce) GSP_HIP(hipMemsetAsync(cur, 0, n * 4, s->st));
            for (auto &sh : s->local) {
                if (!s->rowmode && &sh != &s->local[0]) continue;   // one CSR of all n rows
                RumorTickArgs a{};
                a.n = s->p.n;
                a.tick = t;
                a.row0 = sh.row0;
                a.rows = sh.rows;
                a.off = sh.off.p;
                a.csr_src = sh.csr_src.p;
                a.fail_tick = sh.fail_tick.p;
                a.start_tick = s->joins ? sh.start_tick.p : nullptr;
                a.know_prev = prev;
                a.know_cur = cur;
                a.heard = b.heard.p;
                a.known = b.known.p;
                a.known_stride = s->p.max_ticks + 1;
                fill(sh, a);
                GSP_HIP(launch_rumor_tick(a, s->st));
            }
            if (reduce) GSP_NCCL(ncclAllReduce(cur, cur, n, ncclUint32, ncclMax, s->comm, s->st));
            return GSP_OK;
        }))
        return rc;
    ++b.ticks_traced;
    return GSP_OK;
}

// One rumor's result at the engine's tick T.
template <class E>
int rumor_get(E &s, const char *fn, int32_t rumor, int32_t *heard, uint8_t *state, int32_t *known,
              int32_t known_cap, gsp_rumor_info *info) {
    RumorBufs &b = s.rumor;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no trace is open", fn);
    GSP_REQUIRE(rumor >= 0 && rumor < b.rumors, GSP_ERR_INVALID, "%s: rumor=%d outside [0,%d)", fn, rumor,
                b.rumors);
    GSP_REQUIRE(known_cap >= 0 || !known, GSP_ERR_INVALID, "%s: known_cap=%d", fn, known_cap);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1;
    const int32_t T = s.tick;
    const int32_t *d_heard = b.heard.p + size_t(rumor) * n;
    const uint32_t *d_known = b.known.p + size_t(rumor) * span;
    if (s.rowmode && s.comm) {
        GSP_NCCL(ncclAllReduce(d_heard, b.red.p, n, ncclUint32, ncclMin, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(d_known, b.red.p + n, span, ncclUint32, ncclSum, s.comm, s.st));
        d_heard = reinterpret_cast<const int32_t *>(b.red.p);
        d_known = b.red.p + n;
    }
    b.h_heard.resize(n);
    b.h_known.resize(span);
    GSP_HIP(hipMemcpyAsync(b.h_heard.data(), d_heard, n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipMemcpyAsync(b.h_known.data(), d_known, span * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0, cnt = 0, cnt_alive = 0, last = -1;
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = node_state(s, T, x);
        const int32_t h = b.h_heard[x];
        alive += st == 1;
        cnt += h >= 0;
        cnt_alive += h >= 0 && st == 1;
        last = std::max(last, h);
        if (state) state[x] = st;
    }
    if (heard) std::memcpy(heard, b.h_heard.data(), n * 4);
    if (known)
        for (int32_t t = 0; t < known_cap && t <= T; ++t) known[t] = int32_t(b.h_known[size_t(t)]);
    if (info)
        *info = gsp_rumor_info{T, s.p.n, rumor, b.seed_tick[size_t(rumor)],
                               int32_t(b.seeded[size_t(rumor)].size()), alive, cnt, cnt_alive, last,
                               b.ticks_traced, b.timer.ms(s)};
    return GSP_OK;
}

// ---- the detection ledger (gossip.h "Detection ledger", detect_kernels.hpp) ----
// Every rank folds its own rings, so a get stages its all-reduce whenever there is a communicator.

// One fold, stream-ordered with no host wait: every local shard's ring into the ledger, then the
// shard's counters zeroed by a memset behind its launch.  Called where every writer of the tick
// has been queued on the engine's stream.
template <class E>
int detect_fold(E *s) {
    DetectBufs &b = s->detect;
    const size_t span = size_t(s->p.max_ticks) + 1;
    return b.timer.timed(s, [&]() -> int {
        for (auto &sh : s->local) {
            DetectFoldArgs a{};
            a.ev = sh.ev.args();
            a.n = s->p.n;
            a.span = int32_t(span);
            a.crash = b.crash.p;
            a.arr = b.led.arr.p;
            a.by_tick = b.led.wide.p;
            a.tot = b.led.wide.p + span * 4;
            GSP_HIP(launch_detect_fold(a, b.form, s->st));
            GSP_HIP(hipMemsetAsync(sh.ev.count.p, 0, size_t(kEvStripes) * kEvCounterStride * 8, s->st));
        }
        return GSP_OK;
    });
}

template <class E>
int detect_open(E *s, const char *fn) {
    if (int rc = probe_enter(s, fn)) return rc;
    DetectBufs &b = s->detect;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a ledger is already open (since tick %d)", fn, b.open_tick);
    GSP_REQUIRE(s->p.events != 0 && (s->local[0].ev.kinds & GSP_EVENTS_REMOVE), GSP_ERR_INVALID,
                "%s: the engine does not record removes (params.events = %d; needs GSP_EVENTS_ALL or "
                "GSP_EVENTS_REMOVE)", fn, s->p.events);
    const size_t n = size_t(s->p.n), span = size_t(s->p.max_ticks) + 1;
    GSP_HIP(b.crash.alloc(n));
    if (int rc = b.led.reset(size_t(kDetFields) * n, span * 4 + kDetTotals, s->comm != nullptr, s->st)) return rc;
    GSP_HIP(hipMemcpyAsync(b.crash.p, s->h_fail.data(), n * 4, hipMemcpyHostToDevice, s->st));
    for (int f : {int(kDetFirst), int(kDetFirstFalse)})                        // ~0: none
        GSP_HIP(hipMemsetAsync(b.led.arr.p + size_t(f) * n, 0xFF, n * 4, s->st));
    b.form = kDetectAggregated;
    if (const char *f = std::getenv("GSP_TEST_DETECT_FORM")) b.form = std::atoi(f) ? kDetectAggregated : kDetectPlain;
    b.open_tick = s->tick;
    b.open = true;
    if (int rc = detect_fold(s)) {            // what the ring holds now: every record since the last drain
        b.open = false;
        return rc;
    }
    GSP_HIP(hipStreamSynchronize(s->st));       // open is between steps: the schedule's copy is done on return
    return GSP_OK;
}

// the fold of one stepped tick
template <class E>
int detect_step(E *s) {
    if (int rc = detect_fold(s)) return rc;
    ++s->detect.ticks_folded;
    return GSP_OK;
}

// The ledger at the engine's tick T.
template <class E>
int detect_get(E &s, const char *fn, int32_t *first_remove, int32_t *last_remove, uint32_t *removers,
               uint32_t *false_removes, int32_t *first_false, uint32_t *revivals, uint32_t *evicts,
               uint8_t *state, uint64_t *by_tick, int32_t by_tick_cap, gsp_detect_info *info) {
    DetectBufs &b = s.detect;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no ledger is open", fn);
    GSP_REQUIRE(by_tick_cap >= 0 || !by_tick, GSP_ERR_INVALID, "%s: by_tick_cap=%d", fn, by_tick_cap);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1;
    const int32_t T = s.tick;
    LedgerBufs &l = b.led;
    const bool staged = s.comm != nullptr;
    if (staged) {
        auto reduce = [&](int f, int fields, ncclRedOp_t op) {
            return ncclAllReduce(l.arr.p + size_t(f) * n, l.red.p + size_t(f) * n, size_t(fields) * n,
                                 ncclUint32, op, s.comm, s.st);
        };
        GSP_NCCL(reduce(kDetFirst, 1, ncclMin));
        GSP_NCCL(reduce(kDetLast, 1, ncclMax));
        GSP_NCCL(reduce(kDetRemovers, 2, ncclSum));        // removers, false_removes
        GSP_NCCL(reduce(kDetFirstFalse, 1, ncclMin));
        GSP_NCCL(reduce(kDetRevivals, 2, ncclSum));        // revivals, evicts
        GSP_NCCL(ncclAllReduce(l.wide.p, l.red64.p, l.wides, ncclUint64, ncclSum, s.comm, s.st));
    }
    if (int rc = l.read(staged, s.st)) return rc;
    const uint32_t *h = l.h_arr.data();
    for (size_t x = 0; x < n; ++x) {
        // first_*: ~0 is -1 as the caller's int32; last_remove holds t + 1
        if (first_remove) first_remove[x] = int32_t(h[size_t(kDetFirst) * n + x]);
        if (last_remove) last_remove[x] = int32_t(h[size_t(kDetLast) * n + x]) - 1;
        if (removers) removers[x] = h[size_t(kDetRemovers) * n + x];
        if (false_removes) false_removes[x] = h[size_t(kDetFalse) * n + x];
        if (first_false) first_false[x] = int32_t(h[size_t(kDetFirstFalse) * n + x]);
        if (revivals) revivals[x] = h[size_t(kDetRevivals) * n + x];
        if (evicts) evicts[x] = h[size_t(kDetEvicts) * n + x];
        if (state) state[x] = node_state(s, T, x);
    }
    if (by_tick)
        for (int32_t t = 0; t < by_tick_cap && t <= T; ++t)
            for (int c = 0; c < 4; ++c) by_tick[size_t(t) * 4 + c] = l.h_wide[size_t(t) * 4 + c];
    if (info) {
        const unsigned long long *tot = l.h_wide.data() + span * 4;
        *info = gsp_detect_info{T, s.p.n, b.open_tick, int32_t(s.local[0].ev.kinds), b.ticks_folded, 0,
                                int64_t(tot[kDetRecords]), int64_t(tot[kDetLost]), int64_t(tot[kDetTrue]),
                                int64_t(tot[kDetFalseTot]), int64_t(tot[kDetJoins]),
                                int64_t(tot[kDetRevived]), int64_t(tot[kDetEvicted]), b.timer.ms(s)};
    }
    return GSP_OK;
}

// ---- the traffic ledger (gossip.h "Traffic ledger", traffic_kernels.hpp) ----
// Who computes what, as for the rumor trace: without row shards every engine holds the job's whole
// receiver CSR and every send slot in local[0] and runs all n rows from it, so ranks need no
// exchange; row shards write their own rows of the shared ledger, and across ranks a get
// all-reduces the buffers (SUM; MAX for the peaks) into staging.

template <class E>
int traffic_open(E *s, const char *fn, const int32_t *watch, int32_t n_watch, bool own_sizes) {
    if (int rc = probe_enter(s, fn)) return rc;
    TrafficBufs &b = s->traffic;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a ledger is already open (since tick %d)", fn, b.open_tick);
    GSP_REQUIRE(n_watch >= 0 && n_watch <= kTrMaxWatch && (watch || n_watch == 0), GSP_ERR_INVALID,
                "%s: n_watch=%d outside [0,%d], or no ids", fn, n_watch, kTrMaxWatch);
    if (n_watch > 0)                           // the list may be empty
        if (int rc = check_ids(fn, "watch", watch, n_watch, s->p.n)) return rc;
    const size_t n = size_t(s->p.n), span = size_t(s->p.max_ticks) + 1;
    std::vector<int32_t> slot(n, -1);
    for (int32_t w = 0; w < n_watch; ++w) {
        GSP_REQUIRE(slot[size_t(watch[w])] < 0, GSP_ERR_INVALID, "%s: watch[%d]=%d is listed twice", fn, w,
                    watch[w]);
        slot[size_t(watch[w])] = w;
    }
    const TrafficLayout L{n, span};
    const size_t words = size_t(kTrFields) * n + std::max<size_t>(1, size_t(n_watch)) * span * 2;
    if (int rc = b.led.reset(words, L.total(), s->rowmode && s->comm, s->st)) return rc;
    GSP_HIP(b.watch_slot.alloc(n));
    if (own_sizes) GSP_HIP(b.psize.alloc(n));
    GSP_HIP(hipMemcpyAsync(b.watch_slot.p, slot.data(), n * 4, hipMemcpyHostToDevice, s->st));
    GSP_HIP(hipStreamSynchronize(s->st));       // open is between steps: the map's copy is done on return
    b.form = kTrafficFromSlots;
    if (const char *f = std::getenv("GSP_TEST_TRAFFIC_FORM")) b.form = std::atoi(f) ? kTrafficFromCsr : kTrafficFromSlots;
    b.open_tick = s->tick;
    b.n_watch = n_watch;
    b.open = true;
    return GSP_OK;
}

// The receiver pass of tick t, on the engine's stream with no host wait: called where the receiver
// CSR of t is complete and before the tick kernels.  prep() queues what the sizes need (the
// partial view's count pass or length copies); fill(shard, args) adds what only the engine knows:
// psize, intro_list and the partial view's receipt records.
template <class E, class Prep, class Fill>
int traffic_step_recv(E *s, int32_t t, Prep prep, Fill fill) {
    TrafficBufs &b = s->traffic;
    const size_t n = size_t(s->p.n);
    // the from-CSR form charges the sends of t - 1 here, unless a get has folded them already
    const bool charge = b.form == kTrafficFromCsr && t - 1 > b.open_tick && b.sent_done != t - 1;
    return b.timer.timed(s, [&]() -> int {
        if (int rc = prep()) return rc;
        for (auto &sh : s->local) {
            if (!s->rowmode && &sh != &s->local[0]) continue;   // one CSR of all n rows
            TrafficRecvArgs a{};
            a.n = s->p.n;
            a.tick = t;
            a.span = s->p.max_ticks + 1;
            a.row0 = sh.row0;
            a.rows = sh.rows;
            a.off = sh.off.p;
            a.csr_src = sh.csr_src.p;
            a.fail_tick = sh.fail_tick.p;
            a.start_tick = s->joins ? sh.start_tick.p : nullptr;
            a.intro_list = s->p.policy.intro_list;
            a.form = charge ? kTrafficFromCsr : kTrafficFromSlots;
            a.arr = b.led.arr.p;
            a.wide = b.led.wide.p;
            a.watch_slot = b.watch_slot.p;
            a.watch = b.led.arr.p + size_t(kTrFields) * n;
            fill(sh, a);
            GSP_HIP(launch_traffic_recv(a, s->st));
        }
        return GSP_OK;
    });
}

// The sender pass of tick t: the send slots and, behind them, node 0's delivered JOINREPs (to the
// joiners of t + 1).  Called once every writer of the tick's slots has been queued.
template <class E>
int traffic_send_pass(E *s, int32_t t) {
    TrafficBufs &b = s->traffic;
    const size_t n = size_t(s->p.n);
    const int64_t cnt = s->joins ? s->plan.count(t + 1) : 0;
    return b.timer.timed(s, [&]() -> int {
        for (auto &sh : s->local) {
            if (!s->rowmode && &sh != &s->local[0]) continue;   // local[0] holds every slot
            TrafficSendArgs a{};
            a.n = s->p.n;
            a.tick = t;
            a.span = s->p.max_ticks + 1;
            a.row0 = sh.row0;
            a.rows = sh.rows;
            a.fanout = s->p.fanout;
            a.out_dst = sh.out_dst.p;
            a.arr = b.led.arr.p;
            a.wide = b.led.wide.p;
            a.watch_slot = b.watch_slot.p;
            a.watch = b.led.arr.p + size_t(kTrFields) * n;
            GSP_HIP(launch_traffic_send(a, s->st));
            if (cnt == 0) continue;
            TrafficJoinArgs j{};
            j.n = a.n;
            j.tick = t;
            j.span = a.span;
            j.ok = sh.join_ok.p + s->plan.first(t + 1);   // a row shard flags the joiners it holds
            j.count = int32_t(cnt);
            j.arr = a.arr;
            j.wide = a.wide;
            j.watch_slot = a.watch_slot;
            j.watch = a.watch;
            GSP_HIP(launch_traffic_join(j, s->st));
        }
        return GSP_OK;
    });
}

// the end of one stepped tick (the from-CSR form takes the sends from the next tick's CSR)
template <class E>
int traffic_step_send(E *s, int32_t t) {
    ++s->traffic.ticks_counted;
    if (s->traffic.form == kTrafficFromCsr) return GSP_OK;
    return traffic_send_pass(s, t);
}

// The ledger at the engine's tick T.
template <class E>
int traffic_get(E &s, const char *fn, uint32_t *sent, uint32_t *recv, uint32_t *merged, uint32_t *lost,
                uint64_t *entries_in, uint32_t *peak_recv, int32_t *peak_tick, uint8_t *state,
                uint64_t *by_tick, uint64_t *fanin, uint32_t *watch, int32_t tick_cap,
                gsp_traffic_info *info) {
    TrafficBufs &b = s.traffic;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no ledger is open", fn);
    GSP_REQUIRE(tick_cap >= 0 || !(by_tick || fanin || watch), GSP_ERR_INVALID, "%s: tick_cap=%d", fn, tick_cap);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1;
    const int32_t T = s.tick;
    const TrafficLayout L{n, span};
    LedgerBufs &l = b.led;
    if (b.form == kTrafficFromCsr && T > b.open_tick && b.sent_done != T) {
        if (int rc = traffic_send_pass(&s, T)) return rc;      // the last tick's sends are in no CSR yet
        b.sent_done = T;
    }
    const bool staged = s.rowmode && s.comm;
    if (staged) {
        GSP_NCCL(ncclAllReduce(l.arr.p, l.red.p, l.words, ncclUint32, ncclSum, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(l.wide.p, l.red64.p, L.added(), ncclUint64, ncclSum, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(l.wide.p + L.peak(), l.red64.p + L.peak(), L.total() - L.added(), ncclUint64,
                               ncclMax, s.comm, s.st));
    }
    if (int rc = l.read(staged, s.st)) return rc;
    if (int rc = b.timer.collect(s)) return rc;                // a fold queued by this get
    const uint32_t *h = l.h_arr.data();
    const unsigned long long *w = l.h_wide.data();
    unsigned long long best = 0ull;
    int32_t best_node = -1;
    for (size_t x = 0; x < n; ++x) {
        const unsigned long long pk = w[L.peak() + x];
        if (pk > best) {
            best = pk;
            best_node = int32_t(x);
        }
        if (sent) sent[x] = h[size_t(kTrSent) * n + x];
        if (recv) recv[x] = h[size_t(kTrRecv) * n + x];
        if (merged) merged[x] = h[size_t(kTrMerged) * n + x];
        if (lost) lost[x] = h[size_t(kTrLost) * n + x];
        if (entries_in) entries_in[x] = w[L.entries() + x];
        if (peak_recv) peak_recv[x] = uint32_t(pk >> 32);
        if (peak_tick) peak_tick[x] = pk ? int32_t(~uint32_t(pk)) : -1;
        if (state) state[x] = node_state(s, T, x);
    }
    unsigned long long tot[kTrSums] = {0};
    for (int32_t t = 0; t <= T; ++t) {
        for (int c = 0; c < kTrSums; ++c) tot[c] += w[L.sums() + size_t(t) * kTrSums + c];
        if (t >= tick_cap) continue;
        if (by_tick) {
            for (int c = 0; c < kTrSums; ++c) by_tick[size_t(t) * 6 + c] = w[L.sums() + size_t(t) * kTrSums + c];
            by_tick[size_t(t) * 6 + 5] = w[L.tmax() + size_t(t)];
        }
        if (fanin)
            for (int c = 0; c < kTrBuckets; ++c)
                fanin[size_t(t) * kTrBuckets + c] = w[L.fanin() + size_t(t) * kTrBuckets + c];
        if (watch)
            for (int32_t i = 0; i < b.n_watch; ++i)
                for (int c = 0; c < 2; ++c)
                    watch[(size_t(i) * size_t(tick_cap) + size_t(t)) * 2 + c] =
                        h[size_t(kTrFields) * n + (size_t(i) * span + size_t(t)) * 2 + c];
    }
    if (info)
        *info = gsp_traffic_info{T, s.p.n, b.open_tick, b.ticks_counted, b.n_watch, 0,
                                 int64_t(tot[kTrSumSent]), int64_t(tot[kTrSumRecv]), int64_t(tot[kTrSumMerged]),
                                 int64_t(tot[kTrSumLost]), int64_t(tot[kTrSumEntries]),
                                 int64_t(tot[kTrSumRecv] - tot[kTrSumMerged]), int32_t(best >> 32), best_node,
                                 b.timer.ms(s)};
    return GSP_OK;
}

}  // namespace gsp
