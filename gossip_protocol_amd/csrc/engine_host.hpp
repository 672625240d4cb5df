// gossip_protocol_amd/csrc/engine_host.hpp -- the host engine core shared by the two scale-mode
// engines (scale_engine.cpp: full view, pview_engine.cpp: partial view).
//
// Both engines are an EngineCore plus their own parameters `p` and shards `local` (a ShardCore
// plus their own tables each); the function templates below take the engine type E and read
// only those members.  Here: the stream, the timing-event pool, the failure / join schedule,
// the communicator, the capacity flag and its host mirror, the single-shard CSR build, the
// JOINREP sends, the call into the row exchange (rowx_host.hpp), and the C-ABI bodies that are
// the same code.
// Tables, tick arguments, kernels launched and test knobs stay with each engine.  The six
// read-only probes (census ... traffic ledger) are a layer on top of this core: probes_host.hpp,
// which the engines include and whose ProbeCore they derive from.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "event_ring.hpp"
#include "join_kernels.hpp"
#include "policy.hpp"
#include "rowx_host.hpp"
#include "scale_kernels.hpp"

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
        release_all(own_hb, fail_tick, out_dst, deg, off, fill, csr_src, err, tile_sum, start_tick, joiners,
                    join_ok, ping, dig, ev, x);
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

}  // namespace gsp
