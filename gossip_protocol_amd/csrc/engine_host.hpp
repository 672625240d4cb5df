// gossip_protocol_amd/csrc/engine_host.hpp -- the host engine core shared by the two scale-mode
// engines (scale_engine.cpp: full view, pview_engine.cpp: partial view).
//
// Both engines are an EngineCore plus their own parameters `p` and shards `local` (a ShardCore
// plus their own tables each); the function templates below take the engine type E and read
// only those members.  Here: the stream, the timing-event pool, the failure / join schedule,
// the communicator, the capacity flag and its host mirror, the single-shard CSR build, the
// JOINREP sends, the call into the row exchange (rowx_host.hpp), the host side of the census,
// of the view audit, of the overlay reach, of the rumor trace, of the detection ledger and of the traffic ledger, and
// the C-ABI bodies that are the same code.
// Tables, tick arguments, kernels launched and test knobs stay with each engine.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "audit_kernels.hpp"
#include "census_kernels.hpp"
#include "common.hpp"
#include "detect_kernels.hpp"
#include "event_ring.hpp"
#include "join_kernels.hpp"
#include "policy.hpp"
#include "reach_kernels.hpp"
#include "rowx_host.hpp"
#include "rumor_kernels.hpp"
#include "scale_kernels.hpp"
#include "traffic_kernels.hpp"

namespace gsp {

struct ShardCore {
    int32_t g = 0;
    int32_t row0 = 0, rows = 0;    // row layout: rows [row0, row0 + rows); else all n rows
    DevBuf<int32_t> own_hb, fail_tick, out_dst, deg, off, fill, csr_src, err, tile_sum, start_tick,
        joiners, join_ok, ping;
    DevBuf<unsigned long long> dig;
    EvRing ev;
    RowxBufs x;                    // row layout exchange buffers

    void release() {
        for (auto *b : {&own_hb, &fail_tick, &out_dst, &deg, &off, &fill, &csr_src, &err, &tile_sum,
                        &start_tick, &joiners, &join_ok, &ping})
            b->release();
        dig.release();
        ev.release();
        x.release();
    }
};

// The census accumulators (gsp_scale_census / gsp_pview_census), allocated by the first call:
// n-length device arrays and their host staging; the full view counts into listed / fresh, the
// partial view into counts (fresh << 32 | listed, split at readback).
struct CensusBufs {
    DevBuf<uint32_t> listed, fresh, max_hb;
    DevBuf<unsigned long long> counts;
    std::vector<uint32_t> h32;
    std::vector<unsigned long long> h64;
    hipEvent_t t0 = nullptr, t1 = nullptr;

    void release() {
        for (auto *b : {&listed, &fresh, &max_hb}) b->release();
        counts.release();
        for (hipEvent_t e : {t0, t1})
            if (e) (void)hipEventDestroy(e);
        t0 = t1 = nullptr;
    }
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
    hipEvent_t t0 = nullptr, t1 = nullptr;

    void release() {
        arr.release();
        print.release();
        alive.release();
        fp.release();
        for (hipEvent_t e : {t0, t1})
            if (e) (void)hipEventDestroy(e);
        t0 = t1 = nullptr;
    }
};

// The overlay-reach state (gsp_scale_reach / gsp_pview_reach), allocated by the first call and
// shared by every local shard: hops[n], the two n-bit maps reach_level rewrites per level, the
// cumulative count of reached nodes with its pinned mirror, and the sources' device copy.
struct ReachBufs {
    DevBuf<uint32_t> hops, count;
    DevBuf<uint64_t> front, todo;
    DevBuf<int32_t> src;
    uint32_t *h_count = nullptr;   // pinned
    hipEvent_t t0 = nullptr, t1 = nullptr;

    void release() {
        hops.release();
        count.release();
        front.release();
        todo.release();
        src.release();
        if (h_count) (void)hipHostFree(h_count);
        h_count = nullptr;
        for (hipEvent_t e : {t0, t1})
            if (e) (void)hipEventDestroy(e);
        t0 = t1 = nullptr;
    }
};

// The rumor trace (gsp_*_rumor_*, rumor_kernels.hpp), allocated by open and freed by close, shared
// by every local shard.  `red` stages the all-reduced heard / known of a get across row-shard
// ranks, so the device state itself is never summed twice.
struct RumorBufs {
    bool open = false;
    int32_t rumors = 0, ticks_traced = 0;
    double kernel_ms = 0.0;
    DevBuf<uint32_t> know, known, red;
    DevBuf<int32_t> heard, src;
    std::vector<int32_t> seed_tick;              // per rumor: first seed with an alive source
    std::vector<std::vector<int32_t>> seeded;    // per rumor: the alive sources seeded, ascending
    std::vector<int32_t> h_heard;
    std::vector<uint32_t> h_known;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // timed ticks not yet collected

    void release() {
        for (auto *b : {&know, &known, &red}) b->release();
        heard.release();
        src.release();
        seed_tick.clear();
        seeded.clear();
        open = false;
        rumors = ticks_traced = 0;
        kernel_ms = 0.0;
    }
};

// The detection ledger (gsp_*_detect_*, detect_kernels.hpp), allocated by open and freed by close,
// shared by every local shard: every shard's ring folds into the one ledger (column tiles hold
// disjoint x, row shards disjoint r).  `red` / `red64` stage the all-reduced arrays of a get
// across ranks, so the device state itself is never summed twice.
struct DetectBufs {
    bool open = false;
    int form = kDetectAggregated;                // GSP_TEST_DETECT_FORM=0|1 (tests, A/B) overrides
    int32_t open_tick = 0, ticks_folded = 0;
    double kernel_ms = 0.0;
    DevBuf<int32_t> crash;                       // [n] h_fail
    DevBuf<uint32_t> arr, red;                   // [kDetFields][n]
    DevBuf<unsigned long long> wide, red64;      // by_tick[span][4], then tot[kDetTotals]
    std::vector<uint32_t> h_arr;
    std::vector<unsigned long long> h_wide;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // timed folds not yet collected

    void release() {
        crash.release();
        for (auto *b : {&arr, &red}) b->release();
        for (auto *b : {&wide, &red64}) b->release();
        open = false;
        open_tick = ticks_folded = 0;
        kernel_ms = 0.0;
    }
};

// The traffic ledger (gsp_*_traffic_*, traffic_kernels.hpp), allocated by open and freed by close,
// shared by every local shard.  arr holds the four per-node counters and, behind them, the watch
// rows; `red` / `red64` stage the all-reduced buffers of a get across row-shard ranks, so the
// device state itself is never summed twice.
struct TrafficBufs {
    bool open = false;
    int form = kTrafficFromSlots;                // GSP_TEST_TRAFFIC_FORM=0|1 (tests, A/B) overrides
    int32_t open_tick = 0, ticks_counted = 0, n_watch = 0;
    int32_t sent_done = -1;                      // from-CSR form: the tick whose sends a get folded
    double kernel_ms = 0.0;
    DevBuf<uint32_t> arr, red;                   // [kTrFields][n], then watch[n_watch][span][2]
    DevBuf<unsigned long long> wide, red64;      // TrafficLayout
    DevBuf<int32_t> watch_slot, psize;           // [n] each; psize: the partial view's payload sizes
    std::vector<uint32_t> h_arr;
    std::vector<unsigned long long> h_wide;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // timed passes not yet collected

    void release() {
        for (auto *b : {&arr, &red}) b->release();
        for (auto *b : {&wide, &red64}) b->release();
        for (auto *b : {&watch_slot, &psize}) b->release();
        open = false;
        open_tick = ticks_counted = n_watch = 0;
        sent_done = -1;
        kernel_ms = 0.0;
    }
};

struct EngineCore {
    int device = 0;
    hipStream_t st = nullptr;
    int32_t shards = 1;        // G: shards in the whole job
    int32_t rank = 0;          // first shard index held by this engine
    bool rowmode = false;      // row layout (G > 1, or any communicator): sender rows move
                               // between shards
    ncclComm_t comm = nullptr; // one process per GPU when set
    int64_t pair_cap = 0, msg_cap = 0;
    RowxState rowx;            // row layout: the exchange's count ring and posted sizes
    int32_t *h_err = nullptr;  // pinned mirror of the shards' capacity flags, refreshed by an
                               // async copy at the end of every step call
    int32_t tick = 0;
    bool timing = true;
    std::vector<int32_t> h_fail, h_start;
    bool joins = false;        // a join schedule is set (some node starts after tick 0)
    JoinPlan plan;             // the joiners of every start tick
    struct Timed { hipEvent_t a, b, c; };
    std::vector<Timed> pending;
    std::vector<hipEvent_t> free_events;
    gsp_scale_perf perf{};
    CensusBufs census;
    AuditBufs audit;
    ReachBufs reach;
    RumorBufs rumor;
    DetectBufs detect;
    TrafficBufs traffic;

    void recycle(const Timed &t) {     // a tick's three events back to the pool
        for (hipEvent_t e : {t.a, t.b, t.c}) free_events.push_back(e);
    }

    hipEvent_t event() {
        if (!free_events.empty()) {
            hipEvent_t e = free_events.back();
            free_events.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};

// The parameter ranges common to gsp_scale_params and gsp_pview_params (n is each engine's).
template <class P>
int validate_common(const P &p) {
    GSP_REQUIRE(p.fanout >= 1 && p.fanout <= 16, GSP_ERR_INVALID, "fanout=%d outside [1,16]", p.fanout);
    GSP_REQUIRE(p.tremove >= 1 && p.tremove <= 31, GSP_ERR_INVALID,
                "tremove=%d outside [1,31] (ts is stored mod 32)", p.tremove);
    GSP_REQUIRE(p.h0 >= 1 && p.h0 < 2047, GSP_ERR_INVALID, "h0=%d outside [1,2046]", p.h0);
    GSP_REQUIRE(p.drop_pct >= 0 && p.drop_pct <= 100, GSP_ERR_INVALID, "drop_pct=%d", p.drop_pct);
    GSP_REQUIRE(p.fail_mode >= 0 && p.fail_mode <= 2, GSP_ERR_INVALID, "fail_mode=%d", p.fail_mode);
    GSP_REQUIRE(p.max_ticks >= 1 && int64_t(p.h0) + p.max_ticks <= 2047, GSP_ERR_RANGE,
                "h0 + max_ticks = %d exceeds the 11-bit packed heartbeat (2047)", p.h0 + p.max_ticks);
    GSP_REQUIRE(p.tfail == 0 || (p.tfail >= 1 && p.tfail < p.tremove), GSP_ERR_INVALID,
                "tfail=%d: 0 (off) or 1..tremove-1", p.tfail);
    GSP_REQUIRE(p.swim >= 0 && p.swim <= 8, GSP_ERR_INVALID, "swim=%d: 0 (off) or 1..8 paths", p.swim);
    GSP_REQUIRE(p.events >= 0 && p.events <= 15, GSP_ERR_INVALID,
                "events=%d: 0 off, 1 all, or an OR of GSP_EVENTS_*", p.events);
    GSP_REQUIRE(p.event_cap >= 0, GSP_ERR_INVALID, "event_cap=%lld", (long long)p.event_cap);
    return validate_policy(p.policy, p.n);
}

// Build, first half (s.p is set): the device, and the failure / join schedule.  Failure
// schedule: the same Philox draws as the oracle (policy.hpp; DESIGN.md "Scale mode").
template <class E>
int engine_begin(E &s, const char *who, int device, int32_t shards, int32_t rank) {
    int ndev = 0;
    GSP_HIP(hipGetDeviceCount(&ndev));
    GSP_REQUIRE(device >= 0 && device < ndev, GSP_ERR_HIP, "%s: device %d of %d", who, device, ndev);
    GSP_HIP(hipSetDevice(device));
    s.device = device;
    s.shards = shards;
    s.rank = rank;
    s.h_fail = fail_ticks(s.p.policy, s.p.n, s.p.seed, s.p.fail_mode, s.p.fail_tick, s.p.fail_ppm);
    s.h_start = start_ticks(s.p.policy, s.p.n);
    s.joins = s.p.policy.step_rate > 0 && *std::max_element(s.h_start.begin(), s.h_start.end()) > 0;
    if (s.joins) s.plan = join_plan(s.h_start, s.p.max_ticks + 1);
    return GSP_OK;
}

// Build, second half (rowmode is set): the stream, the flag mirror, the exchange state and the
// communicator of `world` ranks.
inline int engine_open(EngineCore &c, int32_t local_shards, const void *nccl_id, int32_t world,
                       int32_t comm_rank) {
    GSP_HIP(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    GSP_HIP(hipHostMalloc(reinterpret_cast<void **>(&c.h_err), size_t(local_shards) * 4));
    std::memset(c.h_err, 0, size_t(local_shards) * 4);
    if (c.rowmode) GSP_HIP(c.rowx.init(c.shards, nccl_id != nullptr));
    if (nccl_id) {
        ncclUniqueId id;
        std::memcpy(&id, nccl_id, sizeof id);
        GSP_NCCL(ncclCommInitRank(&c.comm, world, id, comm_rank));
    }
    return GSP_OK;
}

// Destroy, after the engine has synchronised the stream and released its shards.
inline void engine_close(EngineCore &c) {
    for (auto &t : c.pending) c.recycle(t);
    for (hipEvent_t e : c.free_events) (void)hipEventDestroy(e);
    if (c.comm) (void)ncclCommDestroy(c.comm);
    c.census.release();
    c.audit.release();
    c.reach.release();
    for (auto &e : c.rumor.pending) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
    c.rumor.pending.clear();
    c.rumor.release();
    for (auto &e : c.detect.pending) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
    c.detect.pending.clear();
    c.detect.release();
    for (auto &e : c.traffic.pending) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
    c.traffic.pending.clear();
    c.traffic.release();
    c.rowx.release();
    if (c.h_err) (void)hipHostFree(c.h_err);
    if (c.st) (void)hipStreamDestroy(c.st);
}

// The buffers of a shard that both engines have, `dig_words` digest words among them; the
// engine allocates its tables (and pre-fills them for a join schedule) itself.
template <class E>
int shard_alloc_core(E &s, ShardCore &sh, size_t dig_words) {
    const size_t n = size_t(s.p.n), rows = size_t(sh.rows), F = size_t(s.p.fanout);
    hipStream_t st = s.st;
    GSP_HIP(sh.own_hb.alloc(rows));
    GSP_HIP(sh.fail_tick.alloc(n));
    GSP_HIP(sh.out_dst.alloc(rows * F));
    GSP_HIP(sh.deg.alloc(n));
    GSP_HIP(sh.off.alloc(rows + 1));
    GSP_HIP(sh.fill.alloc(rows));
    GSP_HIP(sh.csr_src.alloc(n * F));      // every message of the job, at most
    GSP_HIP(sh.err.alloc(1));
    GSP_HIP(sh.tile_sum.alloc(n / 4096 + 1));
    GSP_HIP(sh.dig.alloc(dig_words));
    if (s.p.swim > 0) {
        GSP_HIP(sh.ping.alloc(rows));
        GSP_HIP(hipMemsetAsync(sh.ping.p, 0xFF, rows * 4, st));   // -1: no probe yet
    }
    if (s.joins) {
        GSP_HIP(sh.start_tick.alloc(n));
        GSP_HIP(hipMemcpyAsync(sh.start_tick.p, s.h_start.data(), n * 4, hipMemcpyHostToDevice, st));
        const size_t nj = std::max<size_t>(1, s.plan.joiners.size());
        GSP_HIP(sh.joiners.alloc(nj));
        GSP_HIP(sh.join_ok.alloc(nj));
        if (!s.plan.joiners.empty())
            GSP_HIP(hipMemcpyAsync(sh.joiners.p, s.plan.joiners.data(), s.plan.joiners.size() * 4,
                                   hipMemcpyHostToDevice, st));
    }
    if (s.p.events) GSP_HIP(sh.ev.alloc(s.p.events, s.p.event_cap, st));
    GSP_HIP(hipMemsetAsync(sh.dig.p, 0, dig_words * sizeof(unsigned long long), st));
    GSP_HIP(hipMemsetAsync(sh.own_hb.p, 0, rows * 4, st));
    GSP_HIP(hipMemsetAsync(sh.deg.p, 0, n * 4, st));
    GSP_HIP(hipMemsetAsync(sh.err.p, 0, 4, st));
    GSP_HIP(hipMemcpyAsync(sh.fail_tick.p, s.h_fail.data(), n * 4, hipMemcpyHostToDevice, st));
    return GSP_OK;
}

// Row layout: the sender rows (full view: row_words = stride / 4; partial view: packed views of
// row_words = V entries) of tick t_sent's cross-shard messages move to their receivers' shards
// and every local shard gets the receiver CSR of tick t_sent + 1 (rowx_host.cpp).
template <class E>
int exchange_rows(E *s, int32_t t_sent, int32_t row_words, bool packed) {
    RowxJob job{s->p.n, s->shards, s->p.fanout, row_words, packed, s->pair_cap, s->msg_cap,
                s->comm, s->st, t_sent + 1, &s->rowx};
    // a joiner's sends ramp up to F over its first ticks (its view grows): the joiners of the
    // last three send ticks count as new senders
    job.new_senders = s->joins ? s->plan.count(t_sent) + s->plan.count(t_sent - 1) + s->plan.count(t_sent - 2) : 0;
    job.drop_now = drop_at(s->p.policy, s->p.drop_pct, t_sent);
    job.drop_before = drop_at(s->p.policy, s->p.drop_pct, t_sent - 1);
    std::vector<RowxShard> v;
    for (auto &sh : s->local)
        v.push_back(RowxShard{sh.g, sh.row0, sh.rows, sh.out_dst.p,
                              reinterpret_cast<const uint64_t *>(sh.table[t_sent & 1].p), sh.deg.p,
                              sh.off.p, sh.fill.p, sh.csr_src.p, sh.tile_sum.p, s->local[0].err.p,
                              &sh.x});
    return rowx_exchange(job, v, &s->perf.xgmi_bytes);
}

// One shard's receiver CSR of this tick from last tick's sends, stream-ordered:
//   exclusive_scan(deg) -> off, scatter(out_dst) -> csr_src, deg re-armed for this tick's sends
inline int csr_build(ShardCore &sh, int32_t n, int32_t fanout, hipStream_t st) {
    GSP_HIP(launch_exclusive_scan(sh.deg.p, sh.off.p, n, sh.tile_sum.p, st));
    GSP_HIP(hipMemsetAsync(sh.fill.p, 0, size_t(n) * 4, st));
    GSP_HIP(launch_scatter(sh.out_dst.p, int64_t(n) * fanout, fanout, 0, sh.off.p, sh.fill.p,
                           sh.csr_src.p, st));
    GSP_HIP(hipMemsetAsync(sh.deg.p, 0, size_t(n) * 4, st));
    return GSP_OK;
}

// What differs between the engines' JOINREP sends.
struct JoinForm {
    bool shared_csr;        // column tiles sharing shard 0's CSR: only local[0] sends and scatters
    bool count_all;         // every shard counts sent / dropped (else shard 0 of the job alone)
    size_t dig_words;       // digest words per tick (slots * fields)
    int sent, dropped;      // the digest's field indices
    size_t payload_bytes;   // node 0's row / view, the JOINREP payload
};

// The JOINREPs node 0 sends at tick t to the nodes that start at t + 1 (join_kernels.hpp):
// deg of the receivers (next tick's CSR) and the digest's sent / dropped of tick t; the row
// layout also broadcasts node 0's row of tick t to the other shards (the JOINREP payload).
template <class E>
int join_sends(E *s, int32_t t, const JoinForm &f) {
    const int64_t cnt = s->plan.count(t + 1);
    if (!s->joins || cnt == 0) return GSP_OK;
    for (auto &sh : s->local) {
        if (f.shared_csr && &sh != &s->local[0]) continue;   // one CSR (shard 0's deg)
        JoinSendArgs j{};
        j.joiners = sh.joiners.p + s->plan.first(t + 1);
        j.count = int32_t(cnt);
        j.tick = t;
        j.drop_pct = drop_at(s->p.policy, s->p.drop_pct, t);
        j.seed = s->p.seed;
        j.fail_tick = sh.fail_tick.p;
        j.lo = sh.row0;                   // every row where the shards are not row shards
        j.hi = sh.row0 + sh.rows;
        j.ok = sh.join_ok.p + s->plan.first(t + 1);
        j.deg = sh.deg.p;
        const bool counts = f.count_all || sh.g == 0;
        unsigned long long *dig = sh.dig.p + size_t(t) * f.dig_words;
        j.sent = counts ? dig + f.sent : nullptr;
        j.dropped = counts ? dig + f.dropped : nullptr;
        GSP_HIP(launch_join_send(j, s->st));
    }
    if (!s->rowmode || s->shards == 1) return GSP_OK;
    // node 0's row of tick t -> intro_buf of every other shard
    if (s->comm) {
        auto &sh = s->local[0];
        void *buf = sh.row0 == 0 ? static_cast<void *>(sh.table[t & 1].p) : static_cast<void *>(sh.intro_buf.p);
        GSP_NCCL(ncclBroadcast(buf, buf, f.payload_bytes, ncclUint8, 0, s->comm, s->st));
        s->perf.xgmi_bytes += sh.row0 == 0 ? double(f.payload_bytes) * double(s->shards - 1) : 0.0;
        return GSP_OK;
    }
    for (auto &sh : s->local)
        if (sh.row0 != 0) {
            GSP_HIP(hipMemcpyAsync(sh.intro_buf.p, s->local[0].table[t & 1].p, f.payload_bytes,
                                   hipMemcpyDeviceToDevice, s->st));
            s->perf.xgmi_bytes += double(f.payload_bytes);
        }
    return GSP_OK;
}

// the delivered JOINREPs of tick t into every local shard's receiver CSR (after the scan)
template <class E>
int join_scatter(E *s, int32_t t, bool shared_csr) {
    const int64_t cnt = s->plan.count(t);
    if (!s->joins || cnt == 0) return GSP_OK;
    for (auto &sh : s->local) {
        if (shared_csr && &sh != &s->local[0]) continue;
        GSP_HIP(launch_join_scatter(sh.joiners.p + s->plan.first(t), sh.join_ok.p + s->plan.first(t),
                                    int32_t(cnt), sh.row0, sh.rows, sh.off.p, sh.fill.p, sh.csr_src.p,
                                    s->rowmode ? sh.x.csr_slot.p : nullptr, s->st));
    }
    return GSP_OK;
}

// The capacity flag as last mirrored to the host (no synchronisation): a receiver sent more
// than max_segment messages at tick t sets the flag to t, and the tick kernels of t and every
// later tick return at once, so the job's state stays that of tick t - 1.  Every shard held by
// an engine reads one flag (shard 0's), so an in-process group stops as a whole; with a
// communicator the flag is exchanged each tick (columns: inside the picks all-reduce, and
// every rank holds the same receiver segments; rows: all-reduced ahead of the tick kernels, and
// again with the exchange counts), so all ranks stop at the same tick and report it from their
// own flag.  Full view: without a test's bound (GSP_TEST_MAX_SEGMENT) no segment overflows,
// segments past kMaxSegment are sorted in HBM.  Partial view, drain all (drain_bit set): a hub
// row past its HBM buffers (tick t | drain_bit) is found while tick t's rows run: rows already
// done hold tick t, the others are skipped, so the views after that error are undefined (the
// job stops all the same).
template <class E>
int mirrored_err(E *s, int32_t drain_bit) {
    for (size_t i = 0; i < s->local.size(); ++i) {
        const int32_t e = s->h_err[i];
        GSP_REQUIRE(!(e & kRowxErrBit), GSP_ERR_CAPACITY,
                    "row exchange at tick %d: a shard's rows or records passed the region capacity "
                    "or the size posted to RCCL; ticks after it did not run", e & ~kRowxErrBit);
        GSP_REQUIRE(!(e & drain_bit), GSP_ERR_CAPACITY,
                    "drain all at tick %d: a hub row's list passed its HBM buffers; the job stopped "
                    "there (the views of that tick are undefined)", e & ~drain_bit);
        GSP_REQUIRE(e == 0, GSP_ERR_CAPACITY,
                    "a receiver was sent more than %d messages at tick %d; ticks after it did not run",
                    s->max_segment, e);
    }
    return GSP_OK;
}

// every shard's flag -> h_err, stream-ordered (end of step: read by the next call, never
// waited on)
template <class E>
int mirror_err(E *s) {
    for (size_t i = 0; i < s->local.size(); ++i)
        GSP_HIP(hipMemcpyAsync(s->h_err + i, s->local[i].err.p, 4, hipMemcpyDeviceToHost, s->st));
    return GSP_OK;
}

template <class E>
int check_err(E *s, int32_t drain_bit) {
    if (int rc = mirror_err(s)) return rc;
    GSP_HIP(hipStreamSynchronize(s->st));
    return mirrored_err(s, drain_bit);
}

// the traffic ledger's timed passes into its kernel_ms (waits for their events)
inline int traffic_collect(EngineCore &c) {
    for (auto &e : c.traffic.pending) {
        float ms = 0.f;
        GSP_HIP(hipEventSynchronize(e.second));
        GSP_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        c.traffic.kernel_ms += ms;
        c.free_events.push_back(e.first);
        c.free_events.push_back(e.second);
    }
    c.traffic.pending.clear();
    return GSP_OK;
}

// the timed ticks into perf (waits for their events); row layout: the exchanges' byte counts
inline int collect_timing(EngineCore &c) {
    for (auto &t : c.pending) {
        float a = 0.f, b = 0.f;
        GSP_HIP(hipEventSynchronize(t.c));
        GSP_HIP(hipEventElapsedTime(&a, t.a, t.b));
        GSP_HIP(hipEventElapsedTime(&b, t.b, t.c));
        c.perf.csr_ms += a;
        c.perf.merge_ms += b;
        c.perf.merge_launches++;
        c.recycle(t);
    }
    c.pending.clear();
    for (auto &e : c.rumor.pending) {          // the trace launches of the timed ticks
        float ms = 0.f;
        GSP_HIP(hipEventSynchronize(e.second));
        GSP_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        c.rumor.kernel_ms += ms;
        c.free_events.push_back(e.first);
        c.free_events.push_back(e.second);
    }
    c.rumor.pending.clear();
    for (auto &e : c.detect.pending) {         // the folds of the timed ticks
        float ms = 0.f;
        GSP_HIP(hipEventSynchronize(e.second));
        GSP_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        c.detect.kernel_ms += ms;
        c.free_events.push_back(e.first);
        c.free_events.push_back(e.second);
    }
    c.detect.pending.clear();
    if (int rc = traffic_collect(c)) return rc;
    if (c.rowmode)
        if (int rc = rowx_collect(c.rowx, &c.perf.xgmi_bytes)) return rc;
    return GSP_OK;
}

// ---- C-ABI bodies (the engine has been synchronised; `fn` prefixes the messages) ----

template <class E>
auto holder(E &s, int32_t r) -> decltype(s.local.data()) {
    for (auto &sh : s.local)
        if (r >= sh.row0 && r < sh.row0 + sh.rows) return &sh;
    return nullptr;
}

template <class E>
int read_own_hb(E &s, const char *fn, int32_t r, int32_t *hb) {
    auto *sh = holder(s, r);
    GSP_REQUIRE(sh, GSP_ERR_INVALID, "%s: row %d is not held by this rank", fn, r);
    GSP_HIP(hipMemcpy(hb, sh->own_hb.p + (r - sh->row0), 4, hipMemcpyDeviceToHost));
    return GSP_OK;
}

// the message slots of the first `count` local shards' rows, in row order
template <class E>
int read_messages(E &s, size_t count, int32_t *dst, int64_t cap, int64_t *n) {
    int64_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        const int64_t slots = int64_t(s.local[i].rows) * s.p.fanout;
        if (dst && total < cap)
            GSP_HIP(hipMemcpy(dst + total, s.local[i].out_dst.p, size_t(std::min(cap - total, slots)) * 4,
                              hipMemcpyDeviceToHost));
        total += slots;
    }
    *n = total;
    return GSP_OK;
}

template <class E>
int drain_events(E &s, uint64_t *buf, int64_t cap, int64_t *n, int64_t *lost) {
    int64_t total = 0, dropped = 0;
    for (auto &sh : s.local) GSP_HIP(sh.ev.drain(buf, cap, &total, &dropped));
    *n = total;
    if (lost) *lost = dropped;
    return GSP_OK;
}

// f[k] += field k of tick t's digest, over its slots and the local shards
template <class E>
int digest_sum(E &s, int32_t t, int slots, int fields, unsigned long long *f) {
    std::vector<unsigned long long> h(size_t(slots) * size_t(fields));
    for (auto &sh : s.local) {
        GSP_HIP(hipMemcpy(h.data(), sh.dig.p + size_t(t) * h.size(), h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i) f[i % size_t(fields)] += h[i];
    }
    return GSP_OK;
}

// The census of the engine's current tick T (gossip.h, census_kernels.hpp), after the engine
// has synchronised and reported any pending capacity error.  `packed`: the engine's kernels
// count into census.counts (partial view) instead of listed / fresh.  launch(shard) adds that
// shard's share -- its rows, its columns -- to the zeroed arrays; with a communicator the
// arrays are then all-reduced on the engine's stream (SUM; MAX for max_hb), so every rank must
// make the call at the same tick.
template <class E, class Launch>
int census_run(E &s, bool packed, int32_t age_limit, uint32_t *listed,
               uint32_t *fresh, uint32_t *max_hb, uint8_t *state, gsp_census_info *info,
               Launch launch) {
    const size_t n = size_t(s.p.n);
    const int32_t T = s.tick;
    CensusBufs &c = s.census;
    if (!c.t1) {                       // first call (t1 is made last: a failed attempt starts over)
        GSP_HIP(c.max_hb.alloc(n));
        if (packed) GSP_HIP(c.counts.alloc(n));
        else {
            GSP_HIP(c.listed.alloc(n));
            GSP_HIP(c.fresh.alloc(n));
        }
        if (!c.t0) GSP_HIP(hipEventCreate(&c.t0));
        GSP_HIP(hipEventCreate(&c.t1));
    }
    c.h32.resize(packed ? n : 3 * n);
    c.h64.resize(packed ? n : 0);
    GSP_HIP(hipMemsetAsync(c.max_hb.p, 0, n * 4, s.st));
    if (packed) GSP_HIP(hipMemsetAsync(c.counts.p, 0, n * 8, s.st));
    else {
        GSP_HIP(hipMemsetAsync(c.listed.p, 0, n * 4, s.st));
        GSP_HIP(hipMemsetAsync(c.fresh.p, 0, n * 4, s.st));
    }
    if (s.timing) GSP_HIP(hipEventRecord(c.t0, s.st));
    for (auto &sh : s.local)
        if (int rc = launch(sh)) return rc;
    if (s.timing) GSP_HIP(hipEventRecord(c.t1, s.st));
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
        const uint8_t st = T < s.h_start[x] ? 0 : T <= s.h_fail[x] ? 1 : 2;
        entries += l;
        alive += st == 1;
        if (listed) listed[x] = l;
        if (fresh) fresh[x] = f;
        if (max_hb) max_hb[x] = h_hb[x];
        if (state) state[x] = st;
    }
    if (info) {
        float ms = 0.f;
        if (s.timing) GSP_HIP(hipEventElapsedTime(&ms, c.t0, c.t1));
        *info = gsp_census_info{T, s.p.n, age_limit, alive, entries, double(ms)};
    }
    return GSP_OK;
}

// The view audit of the engine's current tick T (gossip.h, audit_kernels.hpp), after the engine
// has synchronised and reported any pending capacity error.  `full`: the full view, whose kernel
// reads the fingerprint table.  The prologue writes the call's truth (alive bitmap, fp table);
// launch(shard) adds that shard's share -- its rows, its columns -- to the zeroed arrays; with a
// communicator the arrays are then all-reduced on the engine's stream (SUM for the counts and the
// wrapping print, MAX for age_max), so every rank must make the call at the same tick.  The
// observer's own fingerprint joins print in the readback loop.
template <class E, class Launch>
int audit_run(E &s, bool full, int32_t age_limit, uint32_t *size, uint32_t *dead, uint32_t *suspect,
              uint32_t *age_sum, uint8_t *age_max, uint64_t *print, uint8_t *state,
              gsp_audit_info *info, Launch launch) {
    const size_t n = size_t(s.p.n);
    const int32_t T = s.tick;
    AuditBufs &b = s.audit;
    if (!b.t1) {                       // first call (t1 is made last: a failed attempt starts over)
        GSP_HIP(b.arr.alloc(size_t(kAuditFields) * n));
        GSP_HIP(b.print.alloc(n));
        GSP_HIP(b.alive.alloc((n + 7) / 8));
        if (full) GSP_HIP(b.fp.alloc(n));
        if (!b.t0) GSP_HIP(hipEventCreate(&b.t0));
        GSP_HIP(hipEventCreate(&b.t1));
    }
    b.h32.resize(size_t(kAuditFields) * n);
    b.h64.resize(n);
    GSP_HIP(hipMemsetAsync(b.arr.p, 0, size_t(kAuditFields) * n * 4, s.st));
    GSP_HIP(hipMemsetAsync(b.print.p, 0, n * 8, s.st));
    if (s.timing) GSP_HIP(hipEventRecord(b.t0, s.st));
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
    if (s.timing) GSP_HIP(hipEventRecord(b.t1, s.st));
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
        const uint8_t st = T < s.h_start[r] ? 0 : T <= s.h_fail[r] ? 1 : 2;
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
        float ms = 0.f;
        if (s.timing) GSP_HIP(hipEventElapsedTime(&ms, b.t0, b.t1));
        *info = gsp_audit_info{T, s.p.n, age_limit, alive, entries, double(ms)};
    }
    return GSP_OK;
}

// The overlay reach of the engine's current tick T (gossip.h, reach_kernels.hpp), after the
// engine has synchronised and reported any pending capacity error: a level-synchronous BFS, one
// launch per local shard and level.  launch(shard, common, to) runs that shard's share of level
// common.cur -- its rows, its columns -- on the engine's stream; with a communicator hops is
// then all-reduced (MIN), so every rank must make the call at the same tick with the same
// arguments.  After each level reach_level counts the nodes just reached into a device word the
// host waits for: one host wait per level, and the loop ends at the first level that reaches
// nobody.  The count word is cumulative, so it is zeroed once per call.
template <class E, class Launch>
int reach_run(E &s, const char *fn, int32_t direction, int32_t age_limit, const int32_t *sources,
              int32_t n_sources, int32_t *hops, uint8_t *state, gsp_reach_info *info, Launch launch) {
    GSP_REQUIRE(direction == GSP_REACH_FROM || direction == GSP_REACH_TO, GSP_ERR_INVALID,
                "%s: direction=%d is neither GSP_REACH_FROM (0) nor GSP_REACH_TO (1)", fn, direction);
    GSP_REQUIRE(age_limit >= 1 && age_limit <= 32, GSP_ERR_INVALID, "%s: age_limit=%d outside [1,32]",
                fn, age_limit);
    GSP_REQUIRE(sources && n_sources > 0, GSP_ERR_INVALID, "%s: no sources (n_sources=%d)", fn, n_sources);
    for (int32_t i = 0; i < n_sources; ++i)
        GSP_REQUIRE(sources[i] >= 0 && sources[i] < s.p.n, GSP_ERR_INVALID,
                    "%s: sources[%d]=%d outside [0,%d)", fn, i, sources[i], s.p.n);
    const size_t n = size_t(s.p.n), words = reach_bitmap_words(s.p.n);
    const int32_t T = s.tick;
    ReachBufs &b = s.reach;
    if (!b.t1) {                       // first call (t1 is made last: a failed attempt starts over)
        GSP_HIP(b.hops.alloc(n));
        GSP_HIP(b.count.alloc(1));
        GSP_HIP(b.front.alloc(words));
        GSP_HIP(b.todo.alloc(words));
        if (!b.h_count) GSP_HIP(hipHostMalloc(reinterpret_cast<void **>(&b.h_count), 4));
        if (!b.t0) GSP_HIP(hipEventCreate(&b.t0));
        GSP_HIP(hipEventCreate(&b.t1));
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

    if (s.timing) GSP_HIP(hipEventRecord(b.t0, s.st));
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
    if (s.timing) GSP_HIP(hipEventRecord(b.t1, s.st));
    // unset is 0xFFFFFFFF: -1 as the caller's int32
    if (hops) GSP_HIP(hipMemcpyAsync(hops, b.hops.p, n * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    int32_t alive = 0;
    for (size_t x = 0; x < n; ++x) {
        const uint8_t st = T < s.h_start[x] ? 0 : T <= s.h_fail[x] ? 1 : 2;
        alive += st == 1;
        if (state) state[x] = st;
    }
    if (info) {
        float ms = 0.f;
        if (s.timing) GSP_HIP(hipEventElapsedTime(&ms, b.t0, b.t1));
        *info = gsp_reach_info{T, s.p.n, age_limit, direction, alive, int32_t(level0), int32_t(reached),
                               depth, levels, sum_hops, double(ms)};
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
int rumor_open(E &s, const char *fn, int32_t rumors) {
    RumorBufs &b = s.rumor;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a trace is already open (%d rumors)", fn, b.rumors);
    GSP_REQUIRE(rumors >= 1 && rumors <= kRumorMax, GSP_ERR_INVALID, "%s: rumors=%d outside [1,%d]", fn,
                rumors, kRumorMax);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1;
    GSP_HIP(b.know.alloc(2 * n));
    GSP_HIP(b.heard.alloc(size_t(rumors) * n));
    GSP_HIP(b.known.alloc(size_t(rumors) * span));
    if (s.rowmode && s.comm) GSP_HIP(b.red.alloc(n + span));
    GSP_HIP(hipMemsetAsync(b.know.p, 0, 2 * n * 4, s.st));
    GSP_HIP(hipMemsetAsync(b.heard.p, 0xFF, size_t(rumors) * n * 4, s.st));     // -1: not heard
    GSP_HIP(hipMemsetAsync(b.known.p, 0, size_t(rumors) * span * 4, s.st));
    b.seed_tick.assign(size_t(rumors), -1);
    b.seeded.assign(size_t(rumors), {});
    b.rumors = rumors;
    b.ticks_traced = 0;
    b.kernel_ms = 0.0;
    b.open = true;
    return GSP_OK;
}

template <class E>
int rumor_close(E &s, const char *fn) {
    RumorBufs &b = s.rumor;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no trace is open", fn);
    GSP_HIP(hipStreamSynchronize(s.st));           // no queued launch still uses the buffers
    for (auto &e : b.pending) {
        s.free_events.push_back(e.first);
        s.free_events.push_back(e.second);
    }
    b.pending.clear();
    b.release();
    return GSP_OK;
}

// The seed rule at the engine's tick T, stream-ordered.  The host keeps the distinct alive
// sources per rumor from its own copy of the schedule.
template <class E>
int rumor_seed(E &s, const char *fn, int32_t rumor, const int32_t *sources, int32_t n_sources) {
    RumorBufs &b = s.rumor;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no trace is open", fn);
    GSP_REQUIRE(rumor >= 0 && rumor < b.rumors, GSP_ERR_INVALID, "%s: rumor=%d outside [0,%d)", fn, rumor,
                b.rumors);
    GSP_REQUIRE(sources && n_sources > 0, GSP_ERR_INVALID, "%s: no sources (n_sources=%d)", fn, n_sources);
    for (int32_t i = 0; i < n_sources; ++i)
        GSP_REQUIRE(sources[i] >= 0 && sources[i] < s.p.n, GSP_ERR_INVALID,
                    "%s: sources[%d]=%d outside [0,%d)", fn, i, sources[i], s.p.n);
    const size_t n = size_t(s.p.n);
    const int32_t T = s.tick;
    GSP_HIP(b.src.alloc(size_t(n_sources)));
    GSP_HIP(hipMemcpyAsync(b.src.p, sources, size_t(n_sources) * 4, hipMemcpyHostToDevice, s.st));
    RumorSeedArgs a{};
    a.n = s.p.n;
    a.tick = T;
    a.rumor = rumor;
    a.lo = 0;
    a.hi = s.p.n;
    if (s.rowmode && s.comm) {                     // this rank records its own rows only
        a.lo = s.local.front().row0;
        a.hi = s.local.back().row0 + s.local.back().rows;
    }
    a.sources = b.src.p;
    a.n_sources = n_sources;
    a.fail_tick = s.local[0].fail_tick.p;
    a.start_tick = s.joins ? s.local[0].start_tick.p : nullptr;
    a.know = b.know.p + size_t(T & 1) * n;
    a.heard = b.heard.p + size_t(rumor) * n;
    a.known = b.known.p + size_t(rumor) * (size_t(s.p.max_ticks) + 1) + size_t(T);
    GSP_HIP(launch_rumor_seed(a, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));           // seeding is between steps: the caller's array
                                                   // and b.src are free again on return
    std::vector<int32_t> &set = b.seeded[size_t(rumor)];
    for (int32_t i = 0; i < n_sources; ++i) {
        const size_t x = size_t(sources[i]);
        if (s.h_start[x] <= T && T <= s.h_fail[x]) set.push_back(sources[i]);
    }
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
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing) {
        e0 = s->event();
        e1 = s->event();
        GSP_HIP(hipEventRecord(e0, s->st));
    }
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
    if (s->timing) {
        GSP_HIP(hipEventRecord(e1, s->st));
        b.pending.emplace_back(e0, e1);
    }
    ++b.ticks_traced;
    return GSP_OK;
}

// One rumor's result at the engine's tick T, after the engine has synchronised and reported any
// pending capacity error.
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
        const uint8_t st = T < s.h_start[x] ? 0 : T <= s.h_fail[x] ? 1 : 2;
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
                               b.ticks_traced, s.timing ? b.kernel_ms : 0.0};
    return GSP_OK;
}

// ---- the detection ledger (gossip.h "Detection ledger", detect_kernels.hpp) ----

// One fold, stream-ordered with no host wait: every local shard's ring into the ledger, then the
// shard's counters zeroed by a memset behind its launch.  Called where every writer of the tick
// has been queued on the engine's stream.
template <class E>
int detect_fold(E *s) {
    DetectBufs &b = s->detect;
    const size_t span = size_t(s->p.max_ticks) + 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing) {
        e0 = s->event();
        e1 = s->event();
        GSP_HIP(hipEventRecord(e0, s->st));
    }
    for (auto &sh : s->local) {
        DetectFoldArgs a{};
        a.ev = sh.ev.args();
        a.n = s->p.n;
        a.span = int32_t(span);
        a.crash = b.crash.p;
        a.arr = b.arr.p;
        a.by_tick = b.wide.p;
        a.tot = b.wide.p + span * 4;
        GSP_HIP(launch_detect_fold(a, b.form, s->st));
        GSP_HIP(hipMemsetAsync(sh.ev.count.p, 0, size_t(kEvStripes) * kEvCounterStride * 8, s->st));
    }
    if (s->timing) {
        GSP_HIP(hipEventRecord(e1, s->st));
        b.pending.emplace_back(e0, e1);
    }
    return GSP_OK;
}

template <class E>
int detect_open(E &s, const char *fn) {
    DetectBufs &b = s.detect;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a ledger is already open (since tick %d)", fn, b.open_tick);
    GSP_REQUIRE(s.p.events != 0 && (s.local[0].ev.kinds & GSP_EVENTS_REMOVE), GSP_ERR_INVALID,
                "%s: the engine does not record removes (params.events = %d; needs GSP_EVENTS_ALL or "
                "GSP_EVENTS_REMOVE)", fn, s.p.events);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1, wide = span * 4 + kDetTotals;
    GSP_HIP(b.crash.alloc(n));
    GSP_HIP(b.arr.alloc(size_t(kDetFields) * n));
    GSP_HIP(b.wide.alloc(wide));
    if (s.comm) {
        GSP_HIP(b.red.alloc(size_t(kDetFields) * n));
        GSP_HIP(b.red64.alloc(wide));
    }
    GSP_HIP(hipMemcpyAsync(b.crash.p, s.h_fail.data(), n * 4, hipMemcpyHostToDevice, s.st));
    GSP_HIP(hipMemsetAsync(b.arr.p, 0, size_t(kDetFields) * n * 4, s.st));
    for (int f : {int(kDetFirst), int(kDetFirstFalse)})                        // ~0: none
        GSP_HIP(hipMemsetAsync(b.arr.p + size_t(f) * n, 0xFF, n * 4, s.st));
    GSP_HIP(hipMemsetAsync(b.wide.p, 0, wide * 8, s.st));
    b.form = kDetectAggregated;
    if (const char *f = std::getenv("GSP_TEST_DETECT_FORM")) b.form = std::atoi(f) ? kDetectAggregated : kDetectPlain;
    b.open_tick = s.tick;
    b.ticks_folded = 0;
    b.kernel_ms = 0.0;
    b.open = true;
    if (int rc = detect_fold(&s)) {            // what the ring holds now: every record since the last drain
        b.open = false;
        return rc;
    }
    GSP_HIP(hipStreamSynchronize(s.st));       // open is between steps: the schedule's copy is done on return
    return GSP_OK;
}

template <class E>
int detect_close(E &s, const char *fn) {
    DetectBufs &b = s.detect;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no ledger is open", fn);
    GSP_HIP(hipStreamSynchronize(s.st));           // no queued launch still uses the buffers
    for (auto &e : b.pending) {
        s.free_events.push_back(e.first);
        s.free_events.push_back(e.second);
    }
    b.pending.clear();
    b.release();
    return GSP_OK;
}

// the fold of one stepped tick
template <class E>
int detect_step(E *s) {
    if (int rc = detect_fold(s)) return rc;
    ++s->detect.ticks_folded;
    return GSP_OK;
}

// The ledger at the engine's tick T, after the engine has synchronised and reported any pending
// capacity error.
template <class E>
int detect_get(E &s, const char *fn, int32_t *first_remove, int32_t *last_remove, uint32_t *removers,
               uint32_t *false_removes, int32_t *first_false, uint32_t *revivals, uint32_t *evicts,
               uint8_t *state, uint64_t *by_tick, int32_t by_tick_cap, gsp_detect_info *info) {
    DetectBufs &b = s.detect;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no ledger is open", fn);
    GSP_REQUIRE(by_tick_cap >= 0 || !by_tick, GSP_ERR_INVALID, "%s: by_tick_cap=%d", fn, by_tick_cap);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1, wide = span * 4 + kDetTotals;
    const int32_t T = s.tick;
    const uint32_t *d_arr = b.arr.p;
    const unsigned long long *d_wide = b.wide.p;
    if (s.comm) {
        auto reduce = [&](int f, int fields, ncclRedOp_t op) {
            return ncclAllReduce(b.arr.p + size_t(f) * n, b.red.p + size_t(f) * n, size_t(fields) * n,
                                 ncclUint32, op, s.comm, s.st);
        };
        GSP_NCCL(reduce(kDetFirst, 1, ncclMin));
        GSP_NCCL(reduce(kDetLast, 1, ncclMax));
        GSP_NCCL(reduce(kDetRemovers, 2, ncclSum));        // removers, false_removes
        GSP_NCCL(reduce(kDetFirstFalse, 1, ncclMin));
        GSP_NCCL(reduce(kDetRevivals, 2, ncclSum));        // revivals, evicts
        GSP_NCCL(ncclAllReduce(b.wide.p, b.red64.p, wide, ncclUint64, ncclSum, s.comm, s.st));
        d_arr = b.red.p;
        d_wide = b.red64.p;
    }
    b.h_arr.resize(size_t(kDetFields) * n);
    b.h_wide.resize(wide);
    GSP_HIP(hipMemcpyAsync(b.h_arr.data(), d_arr, b.h_arr.size() * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipMemcpyAsync(b.h_wide.data(), d_wide, wide * 8, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    const uint32_t *h = b.h_arr.data();
    for (size_t x = 0; x < n; ++x) {
        // first_*: ~0 is -1 as the caller's int32; last_remove holds t + 1
        if (first_remove) first_remove[x] = int32_t(h[size_t(kDetFirst) * n + x]);
        if (last_remove) last_remove[x] = int32_t(h[size_t(kDetLast) * n + x]) - 1;
        if (removers) removers[x] = h[size_t(kDetRemovers) * n + x];
        if (false_removes) false_removes[x] = h[size_t(kDetFalse) * n + x];
        if (first_false) first_false[x] = int32_t(h[size_t(kDetFirstFalse) * n + x]);
        if (revivals) revivals[x] = h[size_t(kDetRevivals) * n + x];
        if (evicts) evicts[x] = h[size_t(kDetEvicts) * n + x];
        if (state) state[x] = T < s.h_start[x] ? 0 : T <= s.h_fail[x] ? 1 : 2;
    }
    if (by_tick)
        for (int32_t t = 0; t < by_tick_cap && t <= T; ++t)
            for (int c = 0; c < 4; ++c) by_tick[size_t(t) * 4 + c] = b.h_wide[size_t(t) * 4 + c];
    if (info) {
        const unsigned long long *tot = b.h_wide.data() + span * 4;
        *info = gsp_detect_info{T, s.p.n, b.open_tick, int32_t(s.local[0].ev.kinds), b.ticks_folded, 0,
                                int64_t(tot[kDetRecords]), int64_t(tot[kDetLost]), int64_t(tot[kDetTrue]),
                                int64_t(tot[kDetFalseTot]), int64_t(tot[kDetJoins]),
                                int64_t(tot[kDetRevived]), int64_t(tot[kDetEvicted]),
                                s.timing ? b.kernel_ms : 0.0};
    }
    return GSP_OK;
}

// ---- the traffic ledger (gossip.h "Traffic ledger", traffic_kernels.hpp) ----
// Who computes what, as for the rumor trace: without row shards every engine holds the job's whole
// receiver CSR and every send slot in local[0] and runs all n rows from it, so ranks need no
// exchange; row shards write their own rows of the shared ledger, and across ranks a get
// all-reduces the buffers (SUM; MAX for the peaks) into staging.

template <class E>
int traffic_open(E &s, const char *fn, const int32_t *watch, int32_t n_watch, bool own_sizes) {
    TrafficBufs &b = s.traffic;
    GSP_REQUIRE(!b.open, GSP_ERR_INVALID, "%s: a ledger is already open (since tick %d)", fn, b.open_tick);
    GSP_REQUIRE(n_watch >= 0 && n_watch <= kTrMaxWatch && (watch || n_watch == 0), GSP_ERR_INVALID,
                "%s: n_watch=%d outside [0,%d], or no ids", fn, n_watch, kTrMaxWatch);
    const size_t n = size_t(s.p.n), span = size_t(s.p.max_ticks) + 1;
    std::vector<int32_t> slot(n, -1);
    for (int32_t w = 0; w < n_watch; ++w) {
        GSP_REQUIRE(watch[w] >= 0 && watch[w] < s.p.n, GSP_ERR_INVALID, "%s: watch[%d]=%d outside [0,%d)",
                    fn, w, watch[w], s.p.n);
        GSP_REQUIRE(slot[size_t(watch[w])] < 0, GSP_ERR_INVALID, "%s: watch[%d]=%d is listed twice", fn, w,
                    watch[w]);
        slot[size_t(watch[w])] = w;
    }
    const TrafficLayout L{n, span};
    const size_t words = size_t(kTrFields) * n + std::max<size_t>(1, size_t(n_watch)) * span * 2;
    GSP_HIP(b.arr.alloc(words));
    GSP_HIP(b.wide.alloc(L.total()));
    GSP_HIP(b.watch_slot.alloc(n));
    if (own_sizes) GSP_HIP(b.psize.alloc(n));
    if (s.rowmode && s.comm) {
        GSP_HIP(b.red.alloc(words));
        GSP_HIP(b.red64.alloc(L.total()));
    }
    GSP_HIP(hipMemsetAsync(b.arr.p, 0, words * 4, s.st));
    GSP_HIP(hipMemsetAsync(b.wide.p, 0, L.total() * 8, s.st));
    GSP_HIP(hipMemcpyAsync(b.watch_slot.p, slot.data(), n * 4, hipMemcpyHostToDevice, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));       // open is between steps: the map's copy is done on return
    b.form = kTrafficFromSlots;
    if (const char *f = std::getenv("GSP_TEST_TRAFFIC_FORM")) b.form = std::atoi(f) ? kTrafficFromCsr : kTrafficFromSlots;
    b.open_tick = s.tick;
    b.ticks_counted = 0;
    b.n_watch = n_watch;
    b.sent_done = -1;
    b.kernel_ms = 0.0;
    b.open = true;
    return GSP_OK;
}

template <class E>
int traffic_close(E &s, const char *fn) {
    TrafficBufs &b = s.traffic;
    GSP_REQUIRE(b.open, GSP_ERR_INVALID, "%s: no ledger is open", fn);
    GSP_HIP(hipStreamSynchronize(s.st));           // no queued launch still uses the buffers
    for (auto &e : b.pending) {
        s.free_events.push_back(e.first);
        s.free_events.push_back(e.second);
    }
    b.pending.clear();
    b.release();
    return GSP_OK;
}

// a timed span of ledger launches on the engine's stream
template <class E, class Body>
int traffic_timed(E *s, Body body) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s->timing) {
        e0 = s->event();
        e1 = s->event();
        GSP_HIP(hipEventRecord(e0, s->st));
    }
    if (int rc = body()) return rc;
    if (s->timing) {
        GSP_HIP(hipEventRecord(e1, s->st));
        s->traffic.pending.emplace_back(e0, e1);
    }
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
    return traffic_timed(s, [&]() -> int {
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
            a.arr = b.arr.p;
            a.wide = b.wide.p;
            a.watch_slot = b.watch_slot.p;
            a.watch = b.arr.p + size_t(kTrFields) * n;
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
    return traffic_timed(s, [&]() -> int {
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
            a.arr = b.arr.p;
            a.wide = b.wide.p;
            a.watch_slot = b.watch_slot.p;
            a.watch = b.arr.p + size_t(kTrFields) * n;
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

// The ledger at the engine's tick T, after the engine has synchronised and reported any pending
// capacity error.
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
    const size_t words = size_t(kTrFields) * n + std::max<size_t>(1, size_t(b.n_watch)) * span * 2;
    if (b.form == kTrafficFromCsr && T > b.open_tick && b.sent_done != T) {
        if (int rc = traffic_send_pass(&s, T)) return rc;      // the last tick's sends are in no CSR yet
        b.sent_done = T;
    }
    const uint32_t *d_arr = b.arr.p;
    const unsigned long long *d_wide = b.wide.p;
    if (s.rowmode && s.comm) {
        GSP_NCCL(ncclAllReduce(b.arr.p, b.red.p, words, ncclUint32, ncclSum, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(b.wide.p, b.red64.p, L.added(), ncclUint64, ncclSum, s.comm, s.st));
        GSP_NCCL(ncclAllReduce(b.wide.p + L.peak(), b.red64.p + L.peak(), L.total() - L.added(), ncclUint64,
                               ncclMax, s.comm, s.st));
        d_arr = b.red.p;
        d_wide = b.red64.p;
    }
    b.h_arr.resize(words);
    b.h_wide.resize(L.total());
    GSP_HIP(hipMemcpyAsync(b.h_arr.data(), d_arr, words * 4, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipMemcpyAsync(b.h_wide.data(), d_wide, L.total() * 8, hipMemcpyDeviceToHost, s.st));
    GSP_HIP(hipStreamSynchronize(s.st));
    if (int rc = traffic_collect(s)) return rc;                // a fold queued by this get
    const uint32_t *h = b.h_arr.data();
    const unsigned long long *w = b.h_wide.data();
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
        if (state) state[x] = T < s.h_start[x] ? 0 : T <= s.h_fail[x] ? 1 : 2;
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
                                 s.timing ? b.kernel_ms : 0.0};
    return GSP_OK;
}

}  // namespace gsp
