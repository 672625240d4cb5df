// gossip_protocol_amd/csrc/scale_engine.cpp -- host side of the SCALE engine (C ABI).
//
// One GPU (fused): one tick = four stream-ordered launches, no host synchronisation:
//   exclusive_scan(deg) -> off   receiver CSR offsets from last tick's destination counts
//   scatter(out_dst)   -> csr    sender ids per receiver (order fixed later by the kernel)
//   memset(deg)                  re-armed for this tick's sends
//   scale_tick_kernel            merge + ops + events + send, one workgroup per row
// Column shards (G > 1): shard g owns columns [g*W, (g+1)*W) of EVERY row, so the merge is
// entirely local; the only exchange per tick is
//   all-gather of the per-row member counts of every slice     (n * 4 B per shard)
//   all-reduce MAX of the resolved peer choices                (n * fanout * 4 B)
// over RCCL (one process per GPU) or, for a group of shards inside one process, device
// copies on the group's stream (used to test the sharded path on one GPU).
//
// The skeleton shared with the partial-view engine is engine_host.hpp: stream, event pool and
// timing, failure / join schedule, communicator, capacity flag, common shard buffers, the
// single-shard CSR build, JOINREP sends, the call into the row exchange and the C-ABI bodies
// that are the same code; on top of it probes_host.hpp, the host side of the six probes.  Here:
// the tables and column / slice state, the tick arguments, the count / pick exchanges, the sweep
// and the long-row table.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "philox.hpp"
#include "probes_host.hpp"

namespace {

struct Shard : gsp::ShardCore {
    int32_t col0 = 0;
    gsp::DevBuf<uint16_t> table[2];
    gsp::DevBuf<int32_t> cnt_total[2], cnt_slice, cnt_all, picks,
        long_list,                 // [2][1 + rows] by tick parity: rows with k > kMaxSegment
                                   // (a CSR owner's: shard 0 of a shared group, else each)
        mid_list,                  // sub-slab sweep: the same for kSweepMaxSeg < k <= kMaxSegment
        cnt_sub;                   // sub-slab sweep: [local tiles][stride / W][n] on shard 0 of a
                                   // shared group, else [stride / W][n] on each shard
    gsp::DevBuf<uint16_t> intro_buf;   // row layout, shards != 0: node 0's row of the last tick
    gsp::DevBuf<uint8_t> bitmap;

    void release() {
        for (int b = 0; b < 2; ++b) { table[b].release(); cnt_total[b].release(); }
        for (auto *b : {&cnt_slice, &cnt_all, &picks, &long_list, &mid_list, &cnt_sub}) b->release();
        intro_buf.release();
        bitmap.release();
        ShardCore::release();
    }
};

}  // namespace

struct gsp_scale : gsp::ProbeCore {
    gsp_scale_params p{};
    bool sliced = false;       // column layout (G > 1)
    bool shared = false;       // column layout, every shard in this process on one device (an
                               // in-process group): the shards share shard 0's CSR, counts,
                               // picks and sends, so the tick has no exchange at all -- G
                               // column tiles of one GPU's job (DESIGN.md "Column tiles")
    int32_t max_segment = INT32_MAX;     // segments past kMaxSegment take the HBM sort
    int64_t width = 0;         // n rounded up to 2048 * G
    int64_t stride = 0;        // columns per shard
    int policy = 5;            // bit 0 nt own row, bit 1 nt sender rows, bit 2 pipelined loads
    int merge = 1;             // 1 packed 16-bit merge, 0 per-entry form
    int32_t lds_pad = 0;       // GSP_TEST_SCALE_LDS_PAD: extra LDS per tick-kernel workgroup
    int32_t sweep = 0;         // sub-slab width of the tile sweep (scale_sweep_kernel), 0: off;
                               // fixed at create (sweep_width below, GSP_TEST_SCALE_SWEEP)
    int32_t sweep_seg = gsp::kSweepMaxSeg;   // the sweep defers rows with more messages
    std::vector<Shard> local;  // shards held by this engine (1, or G for an in-process group)
    gsp::DevBuf<gsp::ScaleTickArgs> long_tpl;   // [local][2]: every tile's args by tick parity
                                                // (scale_sweep_kernel, scale_long_kernel)
    std::vector<gsp::ScaleTickArgs> sweep_tiles;   // the tick's host-side args of every local tile
                                                   // (launch_scale_sweep's checks, the count launches)

    gsp::ScaleTickArgs args(Shard &sh, int32_t t) const {
        gsp::ScaleTickArgs a{};
        a.prev = sh.table[(t + 1) & 1].p;
        a.cur = sh.table[t & 1].p;
        a.remote = rowmode ? reinterpret_cast<const uint16_t *>(sh.x.recv_rows.p) : nullptr;
        a.stride = stride;
        a.n = p.n;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        a.tick = t;
        a.tremove = p.tremove;
        a.fanout = p.fanout;
        a.h0 = p.h0;
        a.nt_own = policy & 1;
        a.nt_src = (policy >> 1) & 1;
        a.pipe = (policy >> 2) & 1;
        a.lds_pad = lds_pad;
        a.tfail = p.tfail;
        a.swim = p.swim;
        a.count_rounds = rowmode || sh.g == 0;
        a.seed = p.seed;
        a.fail_tick = sh.fail_tick.p;
        a.start_tick = joins ? sh.start_tick.p : nullptr;
        a.drop_pct = gsp::drop_at(p.policy, p.drop_pct, t);
        a.drop_prev = gsp::drop_at(p.policy, p.drop_pct, t - 1);
        // node 0's row of tick t - 1 (the JOINREP payload): the local row 0, or the copy the
        // row layout's shard 0 broadcast
        a.intro = (rowmode && sh.row0 != 0) ? sh.intro_buf.p : sh.table[(t + 1) & 1].p;
        a.intro_list = p.policy.intro_list;
        const Shard &o = owner(sh);    // shared: shard 0 (its CSR, counts, picks and bitmaps)
        // shared: cnt_all[tick parity][G][n], so this tick's slice counts never overwrite the
        // tick-(t - 1) counts another shard's JOINREP still reads
        const size_t gn = size_t(shards) * size_t(p.n);
        a.intro_cnt = sliced ? o.cnt_all.p + (shared ? size_t((t + 1) & 1) * gn : 0) : nullptr;
        a.shards = shards;
        a.shard = sh.g;
        a.own_hb = sh.own_hb.p;
        a.cnt_prev = o.cnt_total[(t + 1) & 1].p;
        a.cnt_cur = shared ? o.cnt_all.p + size_t(t & 1) * gn + size_t(sh.g) * size_t(p.n)
                  : sliced ? sh.cnt_slice.p : sh.cnt_total[t & 1].p;
        a.off = o.off.p;
        a.csr_src = o.csr_src.p;
        a.csr_slot = rowmode ? sh.x.csr_slot.p : nullptr;
        a.out_dst = sh.out_dst.p;
        a.deg = sh.deg.p;
        a.ping = o.ping.p;
        a.bitmap = o.bitmap.p + (shared ? size_t(sh.g - rank) * size_t(p.n) * size_t(stride / 8) : 0);
        a.dig = sh.dig.p + size_t(t) * gsp::kDigSlots * gsp::kDigFields;
        a.err = local[0].err.p;        // one flag for every shard held here
        a.max_segment = max_segment;
        a.ev = sh.ev.args();
        // the rows this tile's CSR defers (k > kMaxSegment): appended by the CSR's owner only
        a.long_list = owns_csr(sh) ? long_list(sh, t) : nullptr;
        a.appends = owns_csr(sh) ? 1 : 0;       // the tile table keeps this where it fills the lists in
        if (sweep && merge == 1) {
            a.sweep = sweep;
            a.sweep_seg = sweep_seg;
            const size_t per = size_t(stride / sweep) * size_t(p.n);
            a.cnt_sub = o.cnt_sub.p + (shared ? size_t(sh.g - rank) * per : 0);
            a.mid_list = owns_csr(sh) ? mid_list(sh, t) : nullptr;
        }
        return a;
    }

    // the shard whose receiver CSR a shard reads (shared column tiles: shard 0's)
    const Shard &owner(const Shard &sh) const { return shared ? local[0] : sh; }
    bool owns_csr(const Shard &sh) const { return &sh == &owner(sh); }
    int32_t *long_list(const Shard &sh, int32_t t) const {
        const Shard &o = owner(sh);
        return o.long_list.p + size_t(t & 1) * size_t(1 + o.rows);
    }

    int32_t *mid_list(const Shard &sh, int32_t t) const {
        const Shard &o = owner(sh);
        return o.mid_list.p ? o.mid_list.p + size_t(t & 1) * size_t(1 + o.rows) : nullptr;
    }

    gsp::ScaleResolveArgs resolve_args(Shard &sh, int32_t t) const {
        gsp::ScaleResolveArgs r{};
        r.n = p.n;
        r.fanout = p.fanout;
        r.tick = t;
        r.shard = sh.g;
        r.shards = shards;
        r.count_rounds = sh.g == 0;
        r.stride = stride;
        r.seed = p.seed;
        r.fail_tick = sh.fail_tick.p;
        r.start_tick = joins ? sh.start_tick.p : nullptr;
        r.drop_pct = gsp::drop_at(p.policy, p.drop_pct, t);
        r.cnt_all = shared ? local[0].cnt_all.p + size_t(t & 1) * size_t(shards) * size_t(p.n) : sh.cnt_all.p;
        r.cnt_total = sh.cnt_total[t & 1].p;
        r.bitmap = sh.bitmap.p;
        r.picks = sh.picks.p;
        r.tiled = shared ? 1 : 0;       // one launch resolves the ranks of every local shard
        r.tile_lo = rank;
        r.tile_cnt = int32_t(local.size());
        r.tile_bytes = int64_t(p.n) * (stride / 8);
        r.swim = p.swim;
        r.ping = sh.ping.p;
        r.out_dst = sh.out_dst.p;
        r.deg = sh.deg.p;
        r.dig = sh.dig.p + size_t(t) * gsp::kDigSlots * gsp::kDigFields;
        return r;
    }
};

namespace {

int validate_scale_params(const gsp_scale_params *p) {
    GSP_REQUIRE(p, GSP_ERR_INVALID, "scale params NULL");
    GSP_REQUIRE(p->n >= 2 && p->n <= (1 << 21), GSP_ERR_INVALID, "n=%d outside [2, 2^21]", p->n);
    return gsp::validate_common(*p);
}

int shard_alloc(gsp_scale *s, Shard &sh) {
    const int32_t n = s->p.n;
    const size_t rows = size_t(sh.rows);
    const size_t tab = rows * size_t(s->stride);
    hipStream_t st = s->st;
    // tests / A/B (GSP_TEST_SCALE_CONTIG=1): the tables in physically contiguous memory
    const char *contig = std::getenv("GSP_TEST_SCALE_CONTIG");
    for (int b = 0; b < 2; ++b) {
        if (contig && std::atoi(contig)) GSP_HIP(sh.table[b].alloc_contiguous(tab));
        else GSP_HIP(sh.table[b].alloc(tab));
        GSP_HIP(sh.cnt_total[b].alloc(size_t(n)));
        GSP_HIP(hipMemsetAsync(sh.cnt_total[b].p, 0, size_t(n) * 4, st));
    }
    if (s->owns_csr(sh)) {
        GSP_HIP(sh.long_list.alloc(2 * (rows + 1)));
        GSP_HIP(hipMemsetAsync(sh.long_list.p, 0, 2 * (rows + 1) * 4, st));
        if (s->sweep) {
            GSP_HIP(sh.mid_list.alloc(2 * (rows + 1)));
            GSP_HIP(hipMemsetAsync(sh.mid_list.p, 0, 2 * (rows + 1) * 4, st));
        }
    }
    if (s->sweep && s->owns_csr(sh))
        GSP_HIP(sh.cnt_sub.alloc(size_t(s->stride / s->sweep) * size_t(n) * (s->shared ? s->local.size() : 1)));
    if (s->sliced && s->owns_csr(sh)) {
        GSP_HIP(sh.cnt_slice.alloc(size_t(n)));
        GSP_HIP(sh.cnt_all.alloc(size_t(n) * s->shards * (s->shared ? 2 : 1)));
        // + 1: the capacity flag rides the all-reduce MAX of the picks (exchange_picks)
        GSP_HIP(sh.picks.alloc(size_t(n) * (s->p.fanout + (s->p.swim > 0 ? 1 : 0)) + 1));
        // shared: every local shard's bitmap, one region each (the resolve reads them all)
        GSP_HIP(sh.bitmap.alloc(size_t(n) * size_t(s->stride / 8) * (s->shared ? s->local.size() : 1)));
    }
    if (s->rowmode)
        GSP_HIP(sh.x.alloc(s->shards, s->pair_cap, s->msg_cap, int32_t(s->stride / 4), false,
                           s->comm != nullptr, int64_t(n) * s->p.fanout, st));
    if (s->joins) {
        // a late joiner's row is read (empty) at its start tick from either buffer, and the
        // init kernel skips the rows that have not started
        for (int b = 0; b < 2; ++b) GSP_HIP(hipMemsetAsync(sh.table[b].p, 0, tab * sizeof(uint16_t), st));
        if (s->rowmode && sh.row0 != 0) GSP_HIP(sh.intro_buf.alloc(size_t(s->stride)));
    }
    return gsp::shard_alloc_core(*s, sh, size_t(s->p.max_ticks + 1) * gsp::kDigSlots * gsp::kDigFields);
}

// all-gather of every shard's per-row slice counts into every shard's cnt_all[G][n]
int exchange_counts(gsp_scale *s, int32_t t) {
    const size_t n = size_t(s->p.n);
    if (s->shared) {                      // the local shards wrote shard 0's cnt_all directly
        if (!s->comm) return GSP_OK;
        // in place: this rank's block of local-shard rows -> every rank's cnt_all[t & 1]
        const size_t L = s->local.size();
        int32_t *all = s->local[0].cnt_all.p + size_t(t & 1) * size_t(s->shards) * n;
        GSP_NCCL(ncclAllGather(all + size_t(s->rank) * n, all, L * n, ncclInt32, s->comm, s->st));
        return GSP_OK;
    }
    if (s->comm) {
        Shard &sh = s->local[0];
        GSP_NCCL(ncclAllGather(sh.cnt_slice.p, sh.cnt_all.p, n, ncclInt32, s->comm, s->st));
        return GSP_OK;
    }
    for (Shard &dst : s->local)
        for (Shard &src : s->local)
            GSP_HIP(hipMemcpyAsync(dst.cnt_all.p + size_t(src.g) * n, src.cnt_slice.p, n * 4,
                                   hipMemcpyDeviceToDevice, s->st));
    return GSP_OK;
}

// all-reduce MAX of the resolved picks (each pick is resolved by exactly one shard)
int exchange_picks(gsp_scale *s) {
    const size_t cnt = size_t(s->p.n) * (s->p.fanout + (s->p.swim > 0 ? 1 : 0));
    if (s->comm) {
        // the capacity flag (0, or the tick that overflowed) rides along in slot cnt, so every
        // rank's next tick kernels stop together and every rank's sync reports it
        Shard &sh = s->local[0];
        GSP_HIP(hipMemcpyAsync(sh.picks.p + cnt, sh.err.p, 4, hipMemcpyDeviceToDevice, s->st));
        GSP_NCCL(ncclAllReduce(sh.picks.p, sh.picks.p, cnt + 1, ncclInt32, ncclMax, s->comm, s->st));
        GSP_HIP(hipMemcpyAsync(sh.err.p, sh.picks.p + cnt, 4, hipMemcpyDeviceToDevice, s->st));
        return GSP_OK;
    }
    Shard &root = s->local[0];
    for (size_t i = 1; i < s->local.size(); ++i)
        GSP_HIP(gsp::launch_max_into(root.picks.p, s->local[i].picks.p, int64_t(cnt), s->st));
    for (size_t i = 1; i < s->local.size(); ++i)
        GSP_HIP(hipMemcpyAsync(s->local[i].picks.p, root.picks.p, cnt * 4, hipMemcpyDeviceToDevice,
                               s->st));
    return GSP_OK;
}

// message generation for tick t (columns: after the slices are merged)
int resolve_sends(gsp_scale *s, int32_t t) {
    const double G = double(s->shards), n = double(s->p.n);
    if (s->shared) {                     // one resolve over every local shard's ranks, one finalize
        if (s->comm) {                   // ... between the ranks' count and pick collectives
            const double W = G / double(s->local.size());
            s->perf.xgmi_bytes += (W - 1.0) * (n * 4.0 * double(s->local.size()) +
                                               2.0 * n * (s->p.fanout + (s->p.swim > 0 ? 1 : 0)) * 4.0 / W);
            if (int rc = exchange_counts(s, t)) return rc;
        }
        GSP_HIP(gsp::launch_scale_resolve(s->resolve_args(s->local[0], t), s->st));
        if (s->comm)
            if (int rc = exchange_picks(s)) return rc;
        GSP_HIP(gsp::launch_scale_finalize(s->resolve_args(s->local[0], t), s->st));
        return GSP_OK;
    }
    // egress per shard of ring collectives: all-gather (G-1)/G of G*n*4 B, all-reduce
    // 2 (G-1)/G of n*f*4 B
    s->perf.xgmi_bytes += double(s->local.size()) * (G - 1.0) *
                          (n * 4.0 + 2.0 * n * (s->p.fanout + (s->p.swim > 0 ? 1 : 0)) * 4.0 / G);
    if (int rc = exchange_counts(s, t)) return rc;
    for (Shard &sh : s->local) GSP_HIP(gsp::launch_scale_resolve(s->resolve_args(sh, t), s->st));
    if (int rc = exchange_picks(s)) return rc;
    for (Shard &sh : s->local) GSP_HIP(gsp::launch_scale_finalize(s->resolve_args(sh, t), s->st));
    return GSP_OK;
}

// Row layout: every shard's member counts of tick t (cnt_total[t & 1], own rows only) reach
// every shard -- the merges digest of tick t + 1 reads them for remote senders.
int exchange_row_counts(gsp_scale *s, int32_t t) {
    if (s->comm) {
        Shard &sh = s->local[0];
        int32_t *cnt = sh.cnt_total[t & 1].p;
        GSP_NCCL(ncclGroupStart());
        for (int32_t g = 0; g < s->shards; ++g) {
            const int32_t r0 = gsp::rowx_row0(g, s->p.n, s->shards);
            const int32_t nr = gsp::rowx_row0(g + 1, s->p.n, s->shards) - r0;
            GSP_NCCL(ncclBroadcast(cnt + r0, cnt + r0, size_t(nr), ncclInt32, g, s->comm, s->st));
        }
        GSP_NCCL(ncclGroupEnd());
        s->perf.xgmi_bytes += double(sh.rows) * 4.0 * double(s->shards - 1);
        return GSP_OK;
    }
    for (Shard &src : s->local)
        for (Shard &dst : s->local) {
            if (&src == &dst) continue;
            GSP_HIP(hipMemcpyAsync(dst.cnt_total[t & 1].p + src.row0, src.cnt_total[t & 1].p + src.row0,
                                   size_t(src.rows) * 4, hipMemcpyDeviceToDevice, s->st));
            s->perf.xgmi_bytes += double(src.rows) * 4.0;
        }
    return GSP_OK;
}

// JOINREPs (engine_host.hpp): one CSR for shared column tiles; per-row digest counters are
// shard 0's outside the row layout; the payload is node 0's row
gsp::JoinForm join_form(const gsp_scale *s) {
    return {s->shared, s->rowmode, size_t(gsp::kDigSlots) * gsp::kDigFields, gsp::kDigSent,
            gsp::kDigDropped, size_t(s->stride) * sizeof(uint16_t)};
}

// The tile table of scale_sweep_kernel and scale_long_kernel: each tile's args at both tick
// parities (digest base at tick 0, every tile reading its CSR owner's deferred-row lists;
// `appends` keeps saying which tile fills them in).  The kernels patch only tick, drop_pct,
// drop_prev and the digest offset per tick (tile_args, scale_row.hpp); every other field is
// read from here, so the table is rebuilt whenever a field it copies can change after create
// (gsp_scale_set_cache_policy: nt_own / nt_src / pipe; gsp_scale_set_merge: the sweep fields).
// An args field that changes per tick must join ScaleTickVals and tile_args instead.
int upload_long_tpl(gsp_scale *s) {
    std::vector<gsp::ScaleTickArgs> tpl;
    for (Shard &sh : s->local)
        for (int32_t par = 0; par < 2; ++par) {
            gsp::ScaleTickArgs x = s->args(sh, 2 + par);
            x.dig = sh.dig.p;
            x.long_list = s->long_list(sh, par);
            x.mid_list = s->mid_list(sh, par);
            tpl.push_back(x);
        }
    if (!s->long_tpl.p) GSP_HIP(s->long_tpl.alloc(tpl.size()));
    GSP_HIP(hipStreamSynchronize(s->st));          // no queued launch still reads the old table
    GSP_HIP(hipMemcpy(s->long_tpl.p, tpl.data(), tpl.size() * sizeof(gsp::ScaleTickArgs),
                      hipMemcpyHostToDevice));
    return GSP_OK;
}

// The sub-slab width of the tile sweep, or 0 for the workgroup-per-row kernel.  The sweep takes
// the slice form of the plain protocol only (no TFAIL, SWIM, join schedule or test bound on the
// segments), and by default only where a sub-slab of both tables, 2 * rows * W * 2 B, stays
// resident in the 256 MiB Infinity Cache with margin (DESIGN.md "Column tiles").
// GSP_TEST_SCALE_SWEEP=0|512 (tests, A/B) overrides the default and the residency rule (any
// other width selects the workgroup-per-row kernel); 512:K also lowers the messages a row may
// have before it is deferred to K (tests: the plain protocol makes no row with more than
// kSweepMaxSeg).
int32_t sweep_width(gsp_scale &s) {
    if (!s.sliced || s.p.tfail > 0 || s.p.swim > 0 || s.joins || s.max_segment != INT32_MAX) return 0;
    int32_t w = gsp::kSweepWidth;
    if (int64_t(s.p.n) * w * 4 > (int64_t(160) << 20)) w = 0;
    if (const char *e = std::getenv("GSP_TEST_SCALE_SWEEP")) {
        w = std::atoi(e);
        if (const char *c = std::strchr(e, ':'))
            s.sweep_seg = std::max(1, std::min<int32_t>(gsp::kSweepMaxSeg, std::atoi(c + 1)));
    }
    if (w != gsp::kSweepWidth) w = 0;
    return w;
}

int scale_build(const gsp_scale_params *p, int device, int32_t shards, int32_t rank,
                int32_t local_shards, const void *nccl_id, int32_t layout, gsp_scale **out) {
    GSP_REQUIRE(out, GSP_ERR_INVALID, "gsp_scale: out is NULL");
    *out = nullptr;
    if (int rc = validate_scale_params(p)) return rc;
    GSP_REQUIRE(shards >= 1 && shards <= 64 && rank >= 0 && rank + local_shards <= shards,
                GSP_ERR_INVALID, "gsp_scale: shards=%d rank=%d", shards, rank);
    std::unique_ptr<gsp_scale> s(new gsp_scale);
    s->p = *p;
    if (int rc = gsp::engine_begin(*s, "gsp_scale", device, shards, rank)) return rc;
    GSP_REQUIRE(layout == GSP_SHARD_COLUMNS || layout == GSP_SHARD_ROWS, GSP_ERR_INVALID,
                "gsp_scale: layout %d", layout);
    GSP_REQUIRE(shards <= p->n, GSP_ERR_INVALID, "gsp_scale: %d shards for %d nodes", shards, p->n);
    // a communicator always runs the sharded protocol (with one rank it exercises RCCL alone)
    const bool sharded = shards > 1 || nccl_id != nullptr;
    s->sliced = sharded && layout == GSP_SHARD_COLUMNS;
    // shared: every shard of this engine shares shard 0's CSR / counts / picks / sends -- an
    // in-process group (all shards here), or the column tiles of one rank (a communicator over
    // shards / local_shards ranks, each holding local_shards consecutive shards)
    s->shared = s->sliced && local_shards > 1 && (nccl_id != nullptr || local_shards == shards);
    GSP_REQUIRE(nccl_id == nullptr || local_shards == 1 ||
                    (layout == GSP_SHARD_COLUMNS && shards % local_shards == 0 && rank % local_shards == 0),
                GSP_ERR_INVALID, "gsp_scale: %d local tiles of %d column shards at shard %d", local_shards,
                shards, rank);
    if (const char *sx = std::getenv("GSP_TEST_SCALE_SHARED")) s->shared = s->shared && std::atoi(sx) != 0;
    s->rowmode = sharded && layout == GSP_SHARD_ROWS;
    const int64_t unit = int64_t(gsp::kChunk) * (s->sliced ? shards : 1);
    s->width = (int64_t(p->n) + unit - 1) / unit * unit;
    s->stride = s->width / (s->sliced ? shards : 1);
    if (s->rowmode) {
        // a sender row goes to a shard at most once: rows_max pairs always fit; large rows get
        // the expected share 1 - (1 - 1/G)^f with margin (a tick beyond it fails loudly)
        int32_t rows_max = 0;
        for (int32_t g = 0; g < shards; ++g)
            rows_max = std::max(rows_max, gsp::rowx_row0(g + 1, p->n, shards) - gsp::rowx_row0(g, p->n, shards));
        const double share = 1.0 - std::pow(1.0 - 1.0 / shards, double(p->fanout));
        s->pair_cap = std::min<int64_t>(rows_max, int64_t(rows_max * share * 1.1) + 1024);
        s->msg_cap = std::min<int64_t>(int64_t(rows_max) * p->fanout,
                                       int64_t(double(rows_max) * p->fanout / shards * 1.25) + 4096);
    }
    if (const char *pol = std::getenv("GSP_TEST_SCALE_POLICY")) s->policy = std::atoi(pol) & 7;
    if (const char *pad = std::getenv("GSP_TEST_SCALE_LDS_PAD")) s->lds_pad = std::max(0, std::min(65536, std::atoi(pad)));
    if (const char *m = std::getenv("GSP_TEST_SCALE_MERGE")) s->merge = std::atoi(m) ? 1 : 0;
    if (!s->sliced) {
        // the fused kernel keeps the row's presence bitmap (and the event stage) in LDS next
        // to 8.3 KB of statics
        GSP_REQUIRE(gsp::scale_lds_bytes(s->stride, false, p->events != 0) <= 48 * 1024, GSP_ERR_CAPACITY,
                    "row bitmap of %lld B%s exceeds the LDS budget (one-GPU full view n <= 393216, "
                    "327680 with events)", (long long)(s->stride / 8), p->events ? " + event stage" : "");
    }
    if (const char *ms = std::getenv("GSP_TEST_MAX_SEGMENT"))   // tests only: force overflows
        s->max_segment = std::max(1, std::atoi(ms));
    s->sweep = sweep_width(*s);
    if (int rc = gsp::engine_open(*s, local_shards, nccl_id, shards / local_shards, rank / local_shards))
        return rc;
    s->local.resize(size_t(local_shards));
    for (int32_t i = 0; i < local_shards; ++i) {
        Shard &sh = s->local[size_t(i)];
        sh.g = rank + i;
        sh.col0 = s->sliced ? int32_t(int64_t(sh.g) * s->stride) : 0;
        sh.row0 = s->rowmode ? gsp::rowx_row0(sh.g, p->n, shards) : 0;
        sh.rows = s->rowmode ? gsp::rowx_row0(sh.g + 1, p->n, shards) - sh.row0 : p->n;
        if (int rc = shard_alloc(s.get(), sh)) return rc;
    }
    if (int rc = upload_long_tpl(s.get())) return rc;
    for (Shard &sh : s->local) GSP_HIP(gsp::launch_scale_init(s->args(sh, 0), s->sliced, s->st));
    if (s->sliced)
        if (int rc = resolve_sends(s.get(), 0)) return rc;
    if (s->rowmode)
        if (int rc = exchange_row_counts(s.get(), 0)) return rc;
    if (int rc = gsp::join_sends(s.get(), 0, join_form(s.get()))) return rc;
    GSP_HIP(hipStreamSynchronize(s->st));
    *out = s.release();
    return GSP_OK;
}

}  // namespace

extern "C" {

int gsp_scale_create(const gsp_scale_params *p, int device, gsp_scale **out) {
    return scale_build(p, device, 1, 0, 1, nullptr, GSP_SHARD_COLUMNS, out);
}

int gsp_scale_create_group(const gsp_scale_params *p, int device, int32_t shards, gsp_scale **out) {
    return scale_build(p, device, shards, 0, shards, nullptr, GSP_SHARD_COLUMNS, out);
}

int gsp_scale_create_group_layout(const gsp_scale_params *p, int device, int32_t shards,
                                  int32_t layout, gsp_scale **out) {
    return scale_build(p, device, shards, 0, shards, nullptr, layout, out);
}

int gsp_scale_create_rank_layout(const gsp_scale_params *p, int device, int32_t rank,
                                 int32_t world, const void *nccl_id, int32_t layout, gsp_scale **out) {
    GSP_REQUIRE(nccl_id || world == 1, GSP_ERR_INVALID, "gsp_scale_create_rank_layout: NULL nccl id");
    return scale_build(p, device, world, rank, 1, nccl_id, layout, out);
}

int gsp_scale_create_rank_tiled(const gsp_scale_params *p, int device, int32_t rank, int32_t world,
                                int32_t tiles, const void *nccl_id, gsp_scale **out) {
    GSP_REQUIRE(nccl_id, GSP_ERR_INVALID, "gsp_scale_create_rank_tiled: NULL nccl id");
    GSP_REQUIRE(tiles >= 1 && world >= 1 && int64_t(world) * tiles <= 64, GSP_ERR_INVALID,
                "gsp_scale_create_rank_tiled: world=%d tiles=%d", world, tiles);
    return scale_build(p, device, world * tiles, rank * tiles, tiles, nccl_id, GSP_SHARD_COLUMNS, out);
}

int gsp_scale_nccl_id(void *out, size_t cap) {
    GSP_REQUIRE(out && cap >= sizeof(ncclUniqueId), GSP_ERR_INVALID,
                "gsp_scale_nccl_id: need %zu bytes", sizeof(ncclUniqueId));
    ncclUniqueId id;
    GSP_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out, &id, sizeof id);
    return GSP_OK;
}

int gsp_scale_create_rank(const gsp_scale_params *p, int device, int32_t rank, int32_t world,
                          const void *nccl_id, gsp_scale **out) {
    GSP_REQUIRE(nccl_id || world == 1, GSP_ERR_INVALID, "gsp_scale_create_rank: NULL nccl id");
    return scale_build(p, device, world, rank, 1, nccl_id, GSP_SHARD_COLUMNS, out);
}

int gsp_scale_destroy(gsp_scale *s) {
    if (!s) return GSP_OK;
    (void)hipSetDevice(s->device);
    if (s->st) (void)hipStreamSynchronize(s->st);
    for (Shard &sh : s->local) sh.release();
    s->long_tpl.release();
    gsp::engine_close(*s);     // the probes' state, then the core (probes_host.hpp)
    delete s;
    return GSP_OK;
}

int gsp_scale_step(gsp_scale *s, int32_t ticks) {
    GSP_REQUIRE(s && ticks >= 0, GSP_ERR_INVALID, "gsp_scale_step: bad argument");
    GSP_REQUIRE(s->tick + ticks <= s->p.max_ticks, GSP_ERR_RANGE,
                "gsp_scale_step: tick %d beyond max_ticks %d", s->tick + ticks, s->p.max_ticks);
    GSP_HIP(hipSetDevice(s->device));
    // an earlier call's ticks overflowed: one process stops here at once; ranks of a
    // communicator do not (the async mirror lands at different times on different ranks, and a
    // rank that returned would leave the others in a collective) -- their kernels already run
    // no row, the row exchange returns the error on every rank at the same tick, and sync
    // reports it
    if (!s->comm)
        if (int rc = gsp::mirrored_err(s, 0)) return rc;
    for (int32_t i = 0; i < ticks; ++i) {
        const int32_t t = s->tick + 1;
        gsp_scale::Timed tm{};
        if (s->timing) {
            tm = {s->event(), s->event(), s->event()};
            GSP_HIP(hipEventRecord(tm.a, s->st));
        }
        if (s->rowmode) {
            if (int rc = gsp::exchange_rows(s, t - 1, int32_t(s->stride / 4), false)) return rc;
            // ranks (row shards): a segment past a test's bound stops every rank's tick t, not
            // only the holder's -- the flag is checked ahead of the tick kernel and all-reduced
            // (ADVICE r03); unbounded otherwise (long segments are sorted in HBM)
            if (s->comm && s->max_segment < INT32_MAX) {
                Shard &sh = s->local[0];
                GSP_HIP(gsp::launch_segment_check(sh.off.p, sh.rows, s->max_segment, sh.err.p, t, s->st));
                GSP_NCCL(ncclAllReduce(sh.err.p, sh.err.p, 1, ncclInt32, ncclMax, s->comm, s->st));
            }
        } else {
            for (Shard &sh : s->local) {
                if (!s->owns_csr(sh)) continue;   // one CSR for every shard
                if (int rc = gsp::csr_build(sh, s->p.n, s->p.fanout, s->st)) return rc;
            }
        }
        if (int rc = gsp::join_scatter(s, t, s->shared)) return rc;
        if (s->rumor.open)       // the CSR of t is complete; the tick kernels may sort it in place
            if (int rc = gsp::rumor_step(s, t, [](Shard &, gsp::RumorTickArgs &) {})) return rc;
        if (s->traffic.open)     // payload sizes: the counts the tick kernels add to merges
            if (int rc = gsp::traffic_step_recv(s, t, [] { return GSP_OK; }, [&](Shard &sh, gsp::TrafficRecvArgs &a) {
                    a.psize = s->owner(sh).cnt_total[(t + 1) & 1].p;
                })) return rc;
        if (s->timing) GSP_HIP(hipEventRecord(tm.b, s->st));
        if (s->sweep && s->merge == 1) {
            // the sub-slab sweep: every local tile in one launch (the kernel reads each tile's
            // args from the tile table), then its per-sub-slab member counts -> cnt_cur
            std::vector<gsp::ScaleTickArgs> &tiles = s->sweep_tiles;   // reused: no allocation per tick
            tiles.clear();
            for (Shard &sh : s->local) tiles.push_back(s->args(sh, t));
            GSP_HIP(gsp::launch_scale_sweep(tiles.data(), int32_t(tiles.size()), s->long_tpl.p, s->st));
            if (s->shared) GSP_HIP(gsp::launch_sweep_counts(tiles[0], int32_t(tiles.size()), s->st));
            else for (const gsp::ScaleTickArgs &a : tiles) GSP_HIP(gsp::launch_sweep_counts(a, 1, s->st));
        } else {
            for (Shard &sh : s->local)
                GSP_HIP(gsp::launch_scale_tick(s->args(sh, t), s->sliced, s->merge, s->st));
        }
        // the rows the launches above deferred (usually none: one short launch per tick); the
        // tiles of a shared CSR, or a single tile, have one pair of lists
        GSP_HIP(gsp::launch_scale_long(s->args(s->local[0], t), s->long_tpl.p, int32_t(s->local.size()),
                                       s->sliced, s->shared || s->local.size() == 1, s->st));
        if (s->timing) {
            GSP_HIP(hipEventRecord(tm.c, s->st));
            s->pending.push_back(tm);
        }
        if (s->detect.open)      // every writer of the tick's records is queued: fold, empty the ring
            if (int rc = gsp::detect_step(s)) return rc;
        if (s->sliced)
            if (int rc = resolve_sends(s, t)) return rc;
        if (s->rowmode)
            if (int rc = exchange_row_counts(s, t)) return rc;
        if (int rc = gsp::join_sends(s, t, join_form(s))) return rc;
        if (s->traffic.open)     // the tick's send slots and JOINREP flags are final
            if (int rc = gsp::traffic_step_send(s, t)) return rc;
        s->tick = t;
        s->perf.ticks++;
    }
    return gsp::mirror_err(s);
}

int gsp_scale_sync(gsp_scale *s) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_sync: NULL");
    GSP_HIP(hipSetDevice(s->device));
    GSP_HIP(hipStreamSynchronize(s->st));
    if (int rc = gsp::collect_timing(*s)) return rc;       // the probes' spans too (probes_host.hpp)
    return gsp::check_err(s, 0);       // 0: the full view sets no drain-all bit
}

int gsp_scale_tick(gsp_scale *s, int32_t *tick) {
    GSP_REQUIRE(s && tick, GSP_ERR_INVALID, "gsp_scale_tick: NULL");
    *tick = s->tick;
    return GSP_OK;
}

// Digest of this engine's shards.  Per-column quantities (joins, removes, hash) are summed
// over the shards held here; per-row quantities are counted by shard 0 only.  In the
// one-process-per-GPU case the job's digest is the sum of every rank's digest.
int gsp_scale_digest_get(gsp_scale *s, int32_t t, gsp_scale_digest *out) {
    GSP_REQUIRE(s && out, GSP_ERR_INVALID, "gsp_scale_digest_get: NULL");
    GSP_REQUIRE(t >= 0 && t <= s->tick, GSP_ERR_INVALID, "gsp_scale_digest_get: tick %d", t);
    if (int rc = gsp_scale_sync(s)) return rc;
    unsigned long long f[gsp::kDigFields] = {0};
    if (int rc = gsp::digest_sum(*s, t, gsp::kDigSlots, gsp::kDigFields, f)) return rc;
    out->tick = t;
    out->node_rounds = int64_t(f[gsp::kDigRounds]);
    out->merges = int64_t(f[gsp::kDigMerges]);
    out->sent = int64_t(f[gsp::kDigSent]);
    out->dropped = int64_t(f[gsp::kDigDropped]);
    out->delivered = int64_t(f[gsp::kDigDelivered]);
    out->joins = int64_t(f[gsp::kDigJoins]);
    out->removes = int64_t(f[gsp::kDigRemoves]);
    out->event_hash = f[gsp::kDigHash];
    return GSP_OK;
}

// Row r of the current table as seen by this engine: every column held by its shards
// (the whole row on one GPU or in an in-process group; zeros outside this rank's slice).
int gsp_scale_row(gsp_scale *s, int32_t r, uint16_t *buf, int32_t cap) {
    GSP_REQUIRE(s && buf && r >= 0 && r < s->p.n, GSP_ERR_INVALID, "gsp_scale_row: row %d", r);
    GSP_REQUIRE(cap >= s->p.n, GSP_ERR_INVALID, "gsp_scale_row: cap %d < n %d", cap, s->p.n);
    if (int rc = gsp_scale_sync(s)) return rc;
    std::memset(buf, 0, size_t(s->p.n) * 2);
    // a crashed row stops at its fail tick: read the buffer of the last tick it ran
    const int32_t last = std::min(s->tick, s->h_fail[size_t(r)]);
    if (s->rowmode) {
        Shard *sh = gsp::holder(*s, r);
        GSP_REQUIRE(sh, GSP_ERR_INVALID, "gsp_scale_row: row %d is not held by this rank", r);
        GSP_HIP(hipMemcpy(buf, sh->table[last & 1].p + size_t(r - sh->row0) * size_t(s->stride),
                          size_t(s->p.n) * 2, hipMemcpyDeviceToHost));
        return GSP_OK;
    }
    for (Shard &sh : s->local) {
        const int64_t c0 = sh.col0;
        const int64_t cnt = std::min<int64_t>(s->stride, int64_t(s->p.n) - c0);
        if (cnt <= 0) continue;
        const uint16_t *src = sh.table[last & 1].p + size_t(r) * size_t(s->stride);
        GSP_HIP(hipMemcpy(buf + c0, src, size_t(cnt) * 2, hipMemcpyDeviceToHost));
    }
    return GSP_OK;
}

int gsp_scale_own_hb(gsp_scale *s, int32_t r, int32_t *hb) {
    GSP_REQUIRE(s && hb && r >= 0 && r < s->p.n, GSP_ERR_INVALID, "gsp_scale_own_hb: bad row");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::read_own_hb(*s, "gsp_scale_own_hb", r, hb);
}

int gsp_scale_messages(gsp_scale *s, int32_t *dst, int64_t cap, int64_t *n) {
    GSP_REQUIRE(s && n, GSP_ERR_INVALID, "gsp_scale_messages: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    // row layout: the slots of the rows held here; else every local shard holds all n rows and
    // local[0]'s out_dst is the job's n * fanout slots
    return gsp::read_messages(*s, s->rowmode ? s->local.size() : 1, dst, cap, n);
}

int gsp_scale_perf_get(gsp_scale *s, gsp_scale_perf *out) {
    GSP_REQUIRE(s && out, GSP_ERR_INVALID, "gsp_scale_perf_get: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    gsp_scale_digest d{};
    if (s->tick > 0)
        if (int rc = gsp_scale_digest_get(s, s->tick, &d)) return rc;
    // algorithmic HBM bytes of the tick kernel(s) of this engine at the last tick: every
    // processed row reads its own row and writes it back (2 * stride * 2 B per shard), reads
    // one sender row per delivered message (stride * 2 B) and its CSR entry (4 B)
    const double rows = double(2 * d.node_rounds + d.delivered);
    s->perf.bytes_per_tick = (rows * double(s->stride) * 2.0 + double(d.delivered) * 4.0) *
                             double(s->sliced ? s->local.size() : 1);
    *out = s->perf;
    return GSP_OK;
}

int gsp_scale_set_timing(gsp_scale *s, int32_t on) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_set_timing: NULL");
    s->timing = on != 0;
    return GSP_OK;
}

int gsp_scale_set_cache_policy(gsp_scale *s, int32_t policy) {
    GSP_REQUIRE(s && policy >= 0 && policy <= 7, GSP_ERR_INVALID,
                "gsp_scale_set_cache_policy: policy %d", policy);
    s->policy = policy;
    return upload_long_tpl(s);
}

int gsp_scale_set_merge(gsp_scale *s, int32_t packed) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_set_merge: NULL");
    s->merge = packed ? 1 : 0;
    return upload_long_tpl(s);         // the table copies the sweep fields args() sets for merge 1
}

int gsp_scale_sweep(gsp_scale *s, int32_t *width, int32_t *seg) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_sweep: NULL");
    if (width) *width = s->merge == 1 ? s->sweep : 0;
    if (seg) *seg = s->sweep_seg;
    return GSP_OK;
}

int gsp_scale_layout(gsp_scale *s, int32_t *shards, int32_t *rank, int64_t *stride) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_layout: NULL");
    if (shards) *shards = s->shards;
    if (rank) *rank = s->rank;
    if (stride) *stride = s->stride;
    return GSP_OK;
}

int gsp_scale_drain_events(gsp_scale *s, uint64_t *buf, int64_t cap, int64_t *n, int64_t *lost) {
    GSP_REQUIRE(s && n && cap >= 0 && (buf || cap == 0), GSP_ERR_INVALID, "gsp_scale_drain_events: bad argument");
    GSP_REQUIRE(s->p.events, GSP_ERR_INVALID, "gsp_scale_drain_events: the engine records no events "
                "(gsp_scale_params.events = 0)");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::drain_events(*s, buf, cap, n, lost);
}

// The probes (probes_host.hpp).  A snapshot or a get syncs the engine and runs the shared body;
// open, seed and close are the shared body alone.

// Census of the current tick (census_run): every local shard adds its rows x columns -- the fused
// table, a column tile from col0, a row shard from row0.
int gsp_scale_census(gsp_scale *s, int32_t age_limit, uint32_t *listed, uint32_t *fresh,
                     uint32_t *max_hb, uint8_t *state, gsp_census_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_census: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::census_run(*s, "gsp_scale_census", false, age_limit, listed, fresh, max_hb, state, info,
                           [&](Shard &sh) -> int {
        gsp::CensusScaleArgs a{};
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.n = s->p.n;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        a.tick = s->tick;
        a.age_limit = age_limit;
        a.fail_tick = sh.fail_tick.p;
        a.start_tick = s->joins ? sh.start_tick.p : nullptr;
        a.listed = s->census.listed.p;
        a.fresh = s->census.fresh.p;
        a.max_hb = s->census.max_hb.p;
        GSP_HIP(gsp::launch_census_scale(a, s->st));
        return GSP_OK;
    });
}

// View audit of the current tick (audit_run): every local shard adds its rows x columns -- the
// fused table, a column tile from col0, a row shard from row0.
int gsp_scale_audit(gsp_scale *s, int32_t age_limit, uint32_t *size, uint32_t *dead,
                    uint32_t *suspect, uint32_t *age_sum, uint8_t *age_max, uint64_t *print,
                    uint8_t *state, gsp_audit_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_audit: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::audit_run(*s, "gsp_scale_audit", true, age_limit, size, dead, suspect, age_sum, age_max,
                          print, state, info, [&](Shard &sh) -> int {
        gsp::AuditScaleArgs a{};
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.n = s->p.n;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        a.tick = s->tick;
        a.age_limit = age_limit;
        a.fail_tick = sh.fail_tick.p;
        a.start_tick = s->joins ? sh.start_tick.p : nullptr;
        a.alive = s->audit.alive.p;
        a.fp = s->audit.fp.p;
        a.arr = s->audit.arr.p;
        a.print = s->audit.print.p;
        GSP_HIP(gsp::launch_audit_scale(a, s->st));
        return GSP_OK;
    });
}

// Overlay reach of the current tick (reach_run): per level every local shard runs its rows x
// columns -- the fused table, a column tile from col0, a row shard from row0.
int gsp_scale_reach(gsp_scale *s, int32_t direction, int32_t age_limit, const int32_t *sources,
                    int32_t n_sources, int32_t *hops, uint8_t *state, gsp_reach_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_reach: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::reach_run(*s, "gsp_scale_reach", direction, age_limit, sources, n_sources, hops, state, info,
                          [&](Shard &sh, const gsp::ReachCommon &c, bool to) -> int {
        gsp::ReachScaleArgs a{};
        a.c = c;
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        GSP_HIP(gsp::launch_reach_scale(a, to, s->st));
        return GSP_OK;
    });
}

// Multi-source reach of the current tick (reach_multi_run): the same shares as gsp_scale_reach.
int gsp_scale_reach_multi(gsp_scale *s, int32_t direction, int32_t age_limit, const int32_t *sources,
                          int32_t n_sources, uint64_t *seen, int32_t *hops, int32_t *reached, int32_t *ecc,
                          int64_t *sum_hops, uint32_t *level_sizes, int32_t level_cap, uint8_t *state,
                          gsp_reach_multi_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_reach_multi: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::reach_multi_run(*s, "gsp_scale_reach_multi", direction, age_limit, sources, n_sources, seen,
                                hops, reached, ecc, sum_hops, level_sizes, level_cap, state, info,
                                [&](Shard &sh, const gsp::ReachMultiCommon &c, bool to) -> int {
        gsp::ReachMultiScaleArgs a{};
        a.c = c;
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        GSP_HIP(gsp::launch_reach_multi_scale(a, to, s->st));
        return GSP_OK;
    });
}

// Overlay clustering of the current tick (cluster_run): per phase every local shard runs its rows
// x columns -- the fused table, a column tile from col0, a row shard from row0.
int gsp_scale_cluster(gsp_scale *s, int32_t age_limit, const int32_t *observers, int32_t n_observers,
                      uint64_t *member, uint32_t *degree, uint64_t *links, uint32_t *mutual, uint8_t *state,
                      gsp_cluster_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_cluster: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::cluster_run(*s, "gsp_scale_cluster", age_limit, observers, n_observers, member, degree, links,
                            mutual, state, info, [&](Shard &sh, const gsp::ClusterCommon &c, int phase) -> int {
        gsp::ClusterScaleArgs a{};
        a.c = c;
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        GSP_HIP(gsp::launch_cluster_scale(a, phase, s->st));
        return GSP_OK;
    });
}

// Overlay components of the current tick (components_run): per sweep every local shard runs its
// rows x columns -- the fused table, a column tile from col0, a row shard from row0.
int gsp_scale_components(gsp_scale *s, int32_t kind, int32_t age_limit, int32_t max_sweeps, int32_t *label,
                         uint8_t *state, gsp_components_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_components: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::components_run(*s, "gsp_scale_components", kind, age_limit, max_sweeps, label, state, info,
                               [&](Shard &sh, const gsp::CompCommon &c) -> int {
        gsp::CompScaleArgs a{};
        a.c = c;
        a.table = sh.table[s->tick & 1].p;
        a.stride = s->stride;
        a.col0 = sh.col0;
        a.row0 = sh.row0;
        a.rows = sh.rows;
        GSP_HIP(gsp::launch_components_scale(a, s->st));
        return GSP_OK;
    });
}

// Rumor trace (rumor_*): every entry of a receiver's segment is heard.
int gsp_scale_rumor_open(gsp_scale *s, int32_t rumors) {
    return gsp::rumor_open(s, "gsp_scale_rumor_open", rumors);
}

int gsp_scale_rumor_seed(gsp_scale *s, int32_t rumor, const int32_t *sources, int32_t n_sources) {
    return gsp::rumor_seed(s, "gsp_scale_rumor_seed", rumor, sources, n_sources);
}

int gsp_scale_rumor_get(gsp_scale *s, int32_t rumor, int32_t *heard, uint8_t *state, int32_t *known,
                        int32_t known_cap, gsp_rumor_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_rumor_get: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::rumor_get(*s, "gsp_scale_rumor_get", rumor, heard, state, known, known_cap, info);
}

int gsp_scale_rumor_close(gsp_scale *s) {
    return gsp::probe_close(s, "gsp_scale_rumor_close", &gsp::ProbeCore::rumor, "trace");
}

// Detection ledger (detect_*): every local shard's ring folds into one ledger.
int gsp_scale_detect_open(gsp_scale *s) {
    return gsp::detect_open(s, "gsp_scale_detect_open");
}

int gsp_scale_detect_get(gsp_scale *s, int32_t *first_remove, int32_t *last_remove, uint32_t *removers,
                         uint32_t *false_removes, int32_t *first_false, uint32_t *revivals,
                         uint32_t *evicts, uint8_t *state, uint64_t *by_tick, int32_t by_tick_cap,
                         gsp_detect_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_detect_get: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::detect_get(*s, "gsp_scale_detect_get", first_remove, last_remove, removers, false_removes,
                           first_false, revivals, evicts, state, by_tick, by_tick_cap, info);
}

int gsp_scale_detect_close(gsp_scale *s) {
    return gsp::probe_close(s, "gsp_scale_detect_close", &gsp::ProbeCore::detect, "ledger");
}

// Traffic ledger (traffic_*): a GOSSIP carries its sender's member count.
int gsp_scale_traffic_open(gsp_scale *s, const int32_t *watch, int32_t n_watch) {
    return gsp::traffic_open(s, "gsp_scale_traffic_open", watch, n_watch, false);
}

int gsp_scale_traffic_get(gsp_scale *s, uint32_t *sent, uint32_t *recv, uint32_t *merged, uint32_t *lost,
                          uint64_t *entries_in, uint32_t *peak_recv, int32_t *peak_tick, uint8_t *state,
                          uint64_t *by_tick, uint64_t *fanin, uint32_t *watch, int32_t tick_cap,
                          gsp_traffic_info *info) {
    GSP_REQUIRE(s, GSP_ERR_INVALID, "gsp_scale_traffic_get: NULL");
    if (int rc = gsp_scale_sync(s)) return rc;
    return gsp::traffic_get(*s, "gsp_scale_traffic_get", sent, recv, merged, lost, entries_in, peak_recv,
                            peak_tick, state, by_tick, fanin, watch, tick_cap, info);
}

int gsp_scale_traffic_close(gsp_scale *s) {
    return gsp::probe_close(s, "gsp_scale_traffic_close", &gsp::ProbeCore::traffic, "ledger");
}

int gsp_scale_hip_stream(gsp_scale *s, void **stream) {
    GSP_REQUIRE(s && stream, GSP_ERR_INVALID, "gsp_scale_hip_stream: NULL");
    *stream = reinterpret_cast<void *>(s->st);
    return GSP_OK;
}

}  // extern "C"
