"""Workloads at the ends of the scale engines' parameter ranges, and their CPU-oracle record.

Both engines pack an entry as hb << 5 | ts mod 32 in 16 bits; validate_common
(csrc/engine_host.hpp) admits tremove 1..31, tfail 1..tremove-1, h0 1..2046 with
h0 + max_ticks <= 2047, fanout 1..16, drop_pct 0..100, swim 0..8, view 1..256, inbox 0..7,
n >= 2, and census / reach take age_limit 1..32.  Each workload below sits on one of those ends;
tests/test_param_edges_cpu.py proves from the record that it reaches the edge it is named for,
tests/test_param_edges_gpu.py compares the engines with the record bit for bit.

reference(name) runs the oracle (ScaleOracle / PviewOracle, plain ints and absolute timestamps)
once per process and keeps what the comparisons read: every tick's digest, and at the check
ticks the message list and a sample of rows (all rows at the last tick), optionally every tick's
events and row lengths, and the expected census and reach at the listed ticks.  Nothing in the
record comes from an engine.
"""
import functools
import time

import numpy as np

from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.test_census_gpu import _reduce, _states

ALIVE = ro.ALIVE
DIRS = (("from", ro.FROM), ("to", ro.TO))
EDGE_LIMITS = (1, 2, 16, 30, 31, 32, None)      # None: the engine's default age limit


def _random(tick, ppm):
    return dict(fail_mode=1, fail_tick=tick, fail_ppm=ppm)      # FAIL_RANDOM


_HB_TOP = dict(h0=2040, fanout=8, tremove=5, drop_pct=10, seed=5, **_random(2, 30000))
_TR31 = dict(tremove=31, drop_pct=10, seed=6, **_random(3, 30000))

# Full view.  kw: the keywords ScaleEngine and ScaleOracle share; every: rows and messages are
# compared at the ticks that are a multiple of it; lens: keep every tick's row lengths; events:
# keep every tick's event list; census: ticks and age limits of the expected census (and reach).
FULL = {
    # the sender bump ((old >> 5) + 1) << 5 at the last heartbeat the 11 bits hold
    "hb_2047": dict(n=1100, ticks=1, kw=dict(h0=2046, fanout=8, tremove=20),
                    census=dict(at=(1,), limits=(None, 32), reach=False)),
    "hb_top": dict(n=1100, ticks=7, kw=_HB_TOP,
                   census=dict(at=(7,), limits=(None, 32), reach=False)),
    "hb_top_swim": dict(n=1100, ticks=7, kw=dict(_HB_TOP, seed=6, drop_pct=0, tfail=3, swim=2)),
    # heartbeats cross 1023 -> 1024: bit 15 of the packed entry turns on
    "hb_cross": dict(n=1100, ticks=27, kw=dict(h0=1020, tremove=9, seed=5, **_random(2, 30000))),
    # two mod-32 wraps of the stored timestamp, ages up to 30
    "tr31": dict(n=1100, ticks=70, kw=_TR31, events=True,
                 census=dict(at=(20, 33, 36), limits=EDGE_LIMITS, reach=True)),
    "tr31_tf30": dict(n=1100, ticks=70, kw=dict(_TR31, tfail=30, swim=2)),
    # tr - 1 = 0: an entry not refreshed in its own tick is removed
    "tr1": dict(n=1100, ticks=12, kw=dict(tremove=1, seed=7), lens=True),
    "tr2_tf1_sw8": dict(n=1100, ticks=20, kw=dict(tremove=2, tfail=1, swim=8, fanout=8, seed=6,
                                                  **_random(3, 30000))),
    "f16": dict(n=1100, ticks=30, kw=dict(fanout=16, tremove=5, drop_pct=20, seed=4,
                                          **_random(3, 30000))),
    # fanout > n - 1, and a lane vector that is partly padding
    "tiny_n2": dict(n=2, ticks=20, kw=dict(fanout=1, tremove=3)),
    "tiny_n9": dict(n=9, ticks=20, kw=dict(fanout=16, tremove=3)),
    "drop100": dict(n=520, ticks=12, kw=dict(drop_pct=100, tremove=5, seed=4),
                    census=dict(at=(12,), limits=(None, 32), reach=False)),
}

_PV = dict(view=32, fanout=3, inbox=7, seed=4128, **_random(2, 50000))
_PV_DRAIN = dict(view=64, fanout=8, inbox=0, seed=4128, **_random(2, 50000))

# Partial view (kw has "view").  The eviction key is age << 11 | (2047 - hb): heartbeats near
# 2047 put the histogram at its lowest bins, tremove = 31 the age at its largest.
PVIEW = {
    "pv_hb_top": dict(n=2048, ticks=7, kw=dict(_PV, h0=2040, tremove=5),
                      census=dict(at=(7,), limits=(None, 32), reach=False)),
    "pv_hb_top_drain": dict(n=1000, ticks=17, kw=dict(_PV_DRAIN, h0=2030, tremove=9)),
    "pv_hb_2046": dict(n=2048, ticks=1, kw=dict(_PV, h0=2046, tremove=5)),
    "pv_tr31_sw8": dict(n=2048, ticks=70, kw=dict(_PV, tremove=31, tfail=30, swim=8),
                        census=dict(at=(20, 33, 36), limits=EDGE_LIMITS, reach=True)),
    # n = 1000 took 4.1 - 5.0 s of oracle steps, against the 5 s bound of the CPU module; 700: 2.8 s
    "pv_tr31_drain": dict(n=700, ticks=70, kw=dict(_PV_DRAIN, fanout=3, tremove=31)),
    "pv_tr2": dict(n=2048, ticks=30, kw=dict(_PV, tremove=2), lens=True),
    "pv_tr1": dict(n=2048, ticks=10, kw=dict(_PV, tremove=1), lens=True),
    "pv_v1": dict(n=2048, ticks=20, kw=dict(_PV, view=1, tremove=5)),
    "pv_v2_f16_k1": dict(n=2048, ticks=20, kw=dict(_PV, view=2, fanout=16, inbox=1, tremove=5)),
    # view almost the population, hub-size inboxes: the oracle's cost grows fast with n (1500:
    # 16 s, 600: 4.6 - 6.0 s, 400: 2.6 s of oracle steps)
    "pv_v256_f16_drain": dict(n=400, ticks=12, kw=dict(_PV, view=256, fanout=16, inbox=0,
                                                       tremove=5)),
    "pv_n2": dict(n=2, ticks=10, kw=dict(view=1, fanout=1, inbox=1, tremove=3)),
    "pv_drop100": dict(n=2048, ticks=10, kw=dict(view=32, drop_pct=100, tremove=5, seed=4128)),
    # the privatised census past kCensusCut = 4096 ids: 4,608 x 128 slots are more than two
    # passes of its grid of 2 x CUs x 1,024 lanes at 256 CUs (census only, never a row run)
    "pv_census_big": dict(n=4608, ticks=6, kw=dict(_PV, view=128, tremove=9),
                          census=dict(at=(0, 6), limits=(3, 32, None), reach=False)),
}

WORKLOADS = dict(FULL, **PVIEW)


def is_pview(name):
    return "view" in WORKLOADS[name]["kw"]


def limit(lim, kw):
    """The age limit a census() / reach() call with lim (None: no argument) runs with."""
    return lim if lim is not None else (kw.get("tfail") or kw.get("tremove", 20))


def check_ticks(w):
    """The ticks whose messages and sampled rows are compared."""
    every, ticks, ftick = w.get("every", 5), w["ticks"], w["kw"].get("fail_tick", 10)
    return sorted({0} | {t for t in range(1, ticks + 1) if t % every == 0 or t in (1, ftick + 1, ticks)})


class Snapshot:
    """What _compare_state / _cmp_rows read of an oracle, frozen at one tick: row(r) of the
    recorded rows, own_hb(r) and fail_tick(r)."""

    def __init__(self, rows, own, fail):
        self.rows, self.own, self.fail = rows, own, fail

    def row(self, r):
        return self.rows[r]

    def own_hb(self, r):
        return self.own[r]

    def fail_tick(self, r):
        return int(self.fail[r])


def _snapshot(orc, rows, fail, pview):
    # full view: n values per row and all n rows at the last tick, so hb (< 2048) and ts as int16
    small = (lambda v: v) if pview else (lambda v: (v[0], v[1].astype(np.int16), v[2].astype(np.int16)))
    return Snapshot({r: small(orc.row(r)) for r in rows}, {r: orc.own_hb(r) for r in rows}, fail)


def _sample(rng, n):
    return sorted(set(rng.integers(0, n, 24).tolist()) | {0, n - 1})


def _full_census(orc, n, t, limits, kw):
    rows = [orc.row(r) for r in range(n)]
    pres = np.stack([x[0] for x in rows]).astype(bool)
    hb = np.stack([x[1] for x in rows])
    ts = np.stack([x[2] for x in rows])
    return _reduce(n, t, _states(orc, n, t), pres, hb, ts, limits, kw)


def _pview_census(orc, n, t, limits, kw):
    """The bincount form of tests/test_census_gpu.py over the alive rows' entries."""
    state = _states(orc, n, t)
    live = state == ALIVE
    rows = [orc.row(r) for r in range(n)]
    ids, hb, ts = (np.concatenate([rows[r][k] for r in range(n) if live[r]] + [np.zeros(0, np.int32)])
                   for k in range(3))
    assert ((ids >= 0) & (ids < n)).all()
    age = (t - ts) & 31
    max_hb = np.zeros(n, np.uint32)
    np.maximum.at(max_hb, ids, hb.astype(np.uint32))
    lims = sorted({limit(l, kw) for l in limits})
    return {"state": state, "live": live, "max_hb": max_hb,
            "listed": np.bincount(ids, minlength=n).astype(np.uint32),
            "fresh": {l: np.bincount(ids[age < l], minlength=n).astype(np.uint32) for l in lims},
            "lens": np.array([len(x[0]) for x in rows])}


def _reach(orc, n, t, limits, kw, pview):
    """{(age limit, direction): (hops, info)} of reach(0, direction, limit) at tick t."""
    state = ro.states(orc, n, t)
    edges = ro.edges_at(orc, n, state, pview)
    out = {}
    for lim in sorted({limit(l, kw) for l in limits}):
        for _, d in DIRS:
            out[(lim, d)] = ro.expected(n, t, state, ro.graph(n, t, edges, lim, d), lim, d, [0])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's record of workload `name` (one run per process)."""
    w = WORKLOADS[name]
    pview = is_pview(name)
    n, ticks, kw = w["n"], w["ticks"], w["kw"]
    orc = (PviewOracle if pview else ScaleOracle)(n, **kw)
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    rng = np.random.default_rng(kw.get("seed", 0) + n)
    checks = check_ticks(w)
    cen = w.get("census", dict(at=(), limits=(), reach=False))
    ref = {"name": name, "w": w, "pview": pview, "fail": fail, "digest": [None], "messages": {},
           "sample": {}, "snap": {}, "events": [None], "lens": {}, "census": {}, "reach": {},
           "seconds": 0.0}
    for t in range(0, ticks + 1):
        if t:
            t0 = time.perf_counter()
            ref["digest"].append(orc.step())
            ref["seconds"] += time.perf_counter() - t0
            if w.get("events"):
                k, r, x = orc.events()
                ref["events"].append(sorted(zip(k.tolist(), r.tolist(), x.tolist())))
        if t in checks:
            src, dst = orc.messages()
            ref["messages"][t] = sorted(zip(src.tolist(), dst.tolist()))
            ref["sample"][t] = list(range(n)) if t == ticks else _sample(rng, n)
            ref["snap"][t] = _snapshot(orc, ref["sample"][t], fail, pview)
        if w.get("lens"):
            if pview:
                ref["lens"][t] = np.array([len(orc.row(r)[0]) for r in range(n)])
            else:
                ref["lens"][t] = np.array([int(orc.row(r)[0].sum()) for r in range(n)])
        if t in cen["at"]:
            ref["census"][t] = (_pview_census if pview else _full_census)(orc, n, t, cen["limits"], kw)
            if cen["reach"]:
                ref["reach"][t] = _reach(orc, n, t, cen["limits"], kw, pview)
    orc.close()
    return ref


def final_entries(ref):
    """(hb, age) of every entry the rows hold at the last tick."""
    t = ref["w"]["ticks"]
    hb, age = [], []
    for r, row in ref["snap"][t].rows.items():
        keep = slice(None) if ref["pview"] else row[0].astype(bool)
        hb.append(row[1][keep])
        age.append(t - row[2][keep])
    return np.concatenate(hb), np.concatenate(age)


def total(ref, field):
    return sum(d[field] for d in ref["digest"][1:])
