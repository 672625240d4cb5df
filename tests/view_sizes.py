"""Partial-view workloads at view sizes off the powers of two, and their CPU-oracle record.

The partial-view kernels depend on V in more places than on any other parameter.  The drain
kernels (csrc/pview_drain.hip) build every list as runs of Vp = pow2(V) tuples, so off a power of
two each run ends in padding that the merge, the fold and the hub kernel's chunk sizing step over;
pv_drain_class sends every long row of a view below 8 slots to the hub kernel, whose merge is then
d_merge_runs, not the windowed form (V = 7, 8 and 9 are three paths); d_own gives a lane two slots
when V passes the 192 lanes of a class-0 row (V = 192 / 193).  The bounded-inbox kernels pad every
source to 256 slots and cut "down to V"; a packed wire row of the row exchange is (4V + 73) / 8
words with its 33 group bounds at 2V, more than one group non-empty only when a view holds ids on
both sides of 65,536; census and reach index the table as i / view.

The workloads (tremove 6, 10 % drops, random failures at tick 4, a seed per V):
  drain_v*    inbox 0, fanout 8: V = 3 .. 255 (n = 1,500 and 14 ticks up to V = 65, 600 and 10 above)
  bounded_v*  inbox 7, fanout 3, n = 1,500; bounded_v9_k1_f16: inbox 1, fanout 16
  burst_v*    inbox 0, every node starts by tick 1 knowing only node 0: node 0 is a hub row
  ext_v*      inbox 0 with TFAIL, SWIM, the JOINREP's introducer list and a drop window
  ids64k_v9   n = 66,000: views with ids on both sides of 65,536

reference(name, evict_order) runs PviewOracle once per process and keeps what the comparisons
read: every tick's digest and per-receiver message counts k (the gossip messages and JOINREPs
queued before the step), at the check ticks the message list and a sample of rows (all rows at the
last tick of the small workloads), optionally every tick's events and the census and reach(0) of
the last tick.  Nothing in the record comes from an engine.  tests/test_view_sizes_cpu.py proves
from the record that each workload reaches what it is named for; tests/test_view_sizes_gpu.py
compares the engine with the record bit for bit.
"""
import functools
import time

import numpy as np

from tests import param_edges as pe
from tests.oracle_binding import PviewOracle, make_policy as oracle_policy

DRAIN_VIEWS = (3, 7, 8, 9, 17, 33, 65, 129, 192, 193, 255)
BOUNDED_VIEWS = (3, 7, 9, 33, 65, 129, 193, 255)
BURST_VIEWS = (7, 8, 9, 193)
EXT_VIEWS = (7, 9, 193)
CENSUS_VIEWS = (7, 193)                       # drain sweep: census and reach at the last tick
EVENT_VIEWS = (7, 9, 193)                     # drain sweep: every tick's events kept
CENSUS_LIMITS = (None, 32)


def _kw(V, **more):
    return dict(dict(view=V, tremove=6, drop_pct=10, seed=7100 + V, **pe._random(4, 40000)), **more)


WORKLOADS = {}
for _V in DRAIN_VIEWS:
    WORKLOADS["drain_v%d" % _V] = dict(
        n=1500 if _V <= 65 else 600, ticks=14 if _V <= 65 else 10, kw=_kw(_V, inbox=0, fanout=8),
        events=_V in EVENT_VIEWS, census=_V in CENSUS_VIEWS)
for _V in BOUNDED_VIEWS:
    WORKLOADS["bounded_v%d" % _V] = dict(n=1500, ticks=14, kw=_kw(_V, inbox=7, fanout=3, seed=7200 + _V))
WORKLOADS["bounded_v9_k1_f16"] = dict(n=1500, ticks=14, kw=_kw(9, inbox=1, fanout=16, seed=7250))
for _V in BURST_VIEWS:
    WORKLOADS["burst_v%d" % _V] = dict(n=900, ticks=8, kw=_kw(_V, inbox=0, fanout=3, seed=7300 + _V),
                                       policy=dict(step_rate=0.002, intro_list=0))
for _V in EXT_VIEWS:
    WORKLOADS["ext_v%d" % _V] = dict(
        n=900, ticks=14, kw=_kw(_V, inbox=0, fanout=6, tfail=3, swim=2, seed=7400 + _V), events=True,
        policy=dict(step_rate=0.02, intro_list=4, drop_window=(3, 12)))
# rows are compared on a sample: every 50th row and rows whose view straddles 65,536
WORKLOADS["ids64k_v9"] = dict(n=66000, ticks=6, kw=_kw(9, inbox=7, fanout=3, seed=7509),
                              checks=(4, 6), sample_step=50)

SPLIT = 65536                                 # the row exchange groups ids by id >> 16


def names(prefix, views):
    return ["%s_v%d" % (prefix, v) for v in views]


# ---- pv_drain_need / pv_drain_class (csrc/pview_kernels.hpp), restated ---------------------------
LDS_MAX, STAGE, HUB = 16384, 64, 4


def drain_need(k, V):
    vp = 1 << max(V - 1, 0).bit_length()
    return vp * (1 + k) + (k + vp - 1) // vp * vp


def drain_class(k, V, lds=LDS_MAX, wide=0):
    need = drain_need(k, V)
    if V < 8 or k > STAGE or need > lds:
        return HUB
    for c, cap in ((0, 3072), (1, 4096), (2, 8192)):
        if wide <= c and need <= cap:
            return c
    return 3 if need <= LDS_MAX else HUB


def check_ticks(w):
    return sorted(w["checks"]) if "checks" in w else pe.check_ticks(w)


def straddles(ids):
    return len(ids) > 0 and ids[0] < SPLIT <= ids[-1]           # a row's ids ascend


@functools.lru_cache(maxsize=None)
def reference(name, evict_order=0):
    """The oracle's record of workload `name` (one run per process and eviction order)."""
    w = WORKLOADS[name]
    n, ticks, kw = w["n"], w["ticks"], dict(w["kw"], evict_order=evict_order)
    orc = PviewOracle(n, policy=oracle_policy(**w["policy"]) if w.get("policy") else None, **kw)
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    start = np.array([orc.start_tick(r) for r in range(n)])
    rng = np.random.default_rng(kw["seed"] + n)
    checks = check_ticks(w)
    ref = {"name": name, "w": w, "kw": kw, "pview": True, "fail": fail, "start": start,
           "digest": [None], "k": [None], "live": [None], "joinreps": 0, "messages": {},
           "sample": {}, "snap": {}, "straddle": {}, "events": [None], "census": {}, "reach": {},
           "seconds": 0.0}
    for t in range(0, ticks + 1):
        if t:
            _, dst = orc.messages()                             # sent at t - 1, merged at t
            jr = orc.joinreps()
            live = (fail >= t) & (start <= t)
            ref["k"].append((np.bincount(dst, minlength=n) + np.bincount(jr, minlength=n)).astype(np.int32))
            ref["live"].append(live)
            ref["joinreps"] += int(live[jr].sum())
            t0 = time.perf_counter()
            ref["digest"].append(orc.step())
            ref["seconds"] += time.perf_counter() - t0
            if w.get("events"):
                k, r, x = orc.events()
                ref["events"].append(sorted(zip(k.tolist(), r.tolist(), x.tolist())))
        if t in checks:
            src, dst = orc.messages()
            ref["messages"][t] = sorted(zip(src.tolist(), dst.tolist()))
            if "sample_step" in w:
                rows = list(range(0, n, w["sample_step"]))
                ref["straddle"][t] = [r for r in rows if straddles(orc.row(r)[0])]
                more = [r for r in range(n) if straddles(orc.row(r)[0])][:60]
                ref["sample"][t] = sorted(set(rows) | set(more) | {n - 1})
            else:
                ref["sample"][t] = list(range(n)) if t == ticks else pe._sample(rng, n)
            ref["snap"][t] = pe._snapshot(orc, ref["sample"][t], fail, True)
        if t == ticks and w.get("census"):
            ref["census"][t] = pe._pview_census(orc, n, t, CENSUS_LIMITS, kw)
            ref["reach"][t] = pe._reach(orc, n, t, CENSUS_LIMITS, kw, True)
    orc.close()
    return ref


def long_rows(ref, t, live_only=False):
    """The receivers sent more than 7 messages for tick t: (rows, their k)."""
    k = ref["k"][t]
    rows = np.nonzero((k > 7) & (ref["live"][t] if live_only else True))[0]
    return rows, k[rows]


def classes_reached(ref, lds=LDS_MAX, wide=0, live_only=True):
    """{class: (rows, messages)} over every tick, of the long rows (the live ones: those that merge)."""
    V = ref["kw"]["view"]
    out = {}
    for t in range(1, ref["w"]["ticks"] + 1):
        for k in long_rows(ref, t, live_only)[1].tolist():
            c = drain_class(k, V, lds, wide)
            rows, msgs = out.get(c, (0, 0))
            out[c] = (rows + 1, msgs + k)
    return out


def total(ref, field):
    return sum(d[field] for d in ref["digest"][1:])
