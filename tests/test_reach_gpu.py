"""Overlay reach (gsp_scale_reach / gsp_pview_reach) against the CPU oracle.

The expected hops are always a numpy BFS (tests/reach_oracle.py) over the oracle's rows
(ScaleOracle.row / PviewOracle.row) between the nodes alive at T -- fail_tick(r) >= T and
start_tick(r) <= T -- never the engine's own row().  Every oracle workload runs once per module
and its BFS results are kept; the cases that share a workload share that record.  The workloads
are the census tests', restated.  The engine is stepped one tick at a time; at the listed ticks
every combination of direction, age limit (32, 3 and the default) and source set (node 0, a
high id, and a set with a duplicate, a node the schedule crashes and two it never does) is
compared: hops array for array, state, and every info field.  A repeated call returns identical
arrays, and at the end every tick's digest still equals the oracle's, so reach disturbed nothing.

What the inputs exercise is asserted from the oracle's record itself: graphs from 2 to 129
levels deep, live nodes that cannot be reached, stale entries in the crashed rows' own buffers,
ticks past the mod-32 wrap, joiners nobody lists yet and sources that are not alive.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

DIRS = (("from", ro.FROM), ("to", ro.TO))
LIMITS = (32, 3, None)
INFO = ("tick", "n", "age_limit", "direction", "alive", "sources", "reached", "depth", "levels",
        "sum_hops")

FULL = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes; T = 33, 40 lie past
    # the mod-32 wrap
    "main": dict(n=3000, ticks=40, at=(0, 1, 12, 20, 33, 40), high=2999, limits=LIMITS,
                 sets=("zero", "high", "multi"), pol=None,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): at T = 5 exactly the nodes >= 120 have not started
    "join": dict(n=600, ticks=35, at=(5, 20, 35), high=599, limits=LIMITS,
                 sets=("zero", "high", "multi"), pol=dict(step_rate=0.05, intro_list=8),
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
    # TFAIL + SWIM: a suspected member is not gossiped to, so age_limit defaults to tfail
    "variants": dict(n=1024, ticks=13, at=(13,), high=1023, limits=(None,), sets=("zero",), pol=None,
                     kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                             fail_ppm=20000, seed=3003, tfail=4, swim=2)),
}

PVIEW = {
    "A": dict(n=4096, ticks=40, at=(0, 1, 12, 25, 40), high=4000, limits=LIMITS,
              sets=("zero", "high", "multi"),
              kw=dict(view=32, fanout=3, inbox=7, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=4128)),
    "B": dict(n=1000, ticks=40, at=(12, 40), high=900, limits=LIMITS,
              sets=("zero", "high", "multi"),
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
}


def _limit(lim, kw):
    return lim if lim is not None else (kw.get("tfail") or kw["tremove"])


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    """One oracle run: the digests, the source sets, and per listed tick the state, the alive
    rows' in-degree and the expected (hops, info) of every case."""
    pview = kind == "pview"
    w = (PVIEW if pview else FULL)[name]
    n = w["n"]
    if pview:
        orc = PviewOracle(n, **w["kw"])
    else:
        orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    sets = ro.source_sets(orc, n, w["high"])
    ref = {"digest": [None], "sets": sets, "at": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t not in w["at"]:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        rec = {"state": state, "dead_entries": edges[3], "cases": {},
               "listed": np.bincount(edges[1], minlength=n)}
        for lim in sorted({_limit(l, w["kw"]) for l in w["limits"]}):
            for _, d in DIRS:
                adj = ro.graph(n, t, edges, lim, d)
                for s in w["sets"]:
                    rec["cases"][(lim, d, s)] = ro.expected(n, t, state, adj, lim, d, sets[s])
        ref["at"][t] = rec
    orc.close()
    return ref


def _check(got, want, tag):
    hops, info = want
    assert got.hops.dtype == np.int32 and got.tick == info["tick"], tag
    assert np.array_equal(got.hops, hops), "hops %s: %d differ" % (tag, int((got.hops != hops).sum()))
    for f in INFO:
        assert got.info[f] == info[f], "info.%s %s: %r != %r" % (f, tag, got.info[f], info[f])
    assert got.info["kernel_ms"] > 0, tag


def _run(eng, w, ref):
    """Step to the end, every case at the listed ticks, digests at the end."""
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        rec = ref["at"][t]
        for dname, d in DIRS:
            for l in w["limits"]:
                lim = _limit(l, w["kw"])
                for s in w["sets"]:
                    src = ref["sets"][s]
                    src = src[0] if len(src) == 1 else src          # an int or a sequence
                    got = eng.reach(src, dname) if l is None else eng.reach(src, dname, l)
                    tag = "tick %d %s age_limit %d sources %s" % (t, dname, lim, s)
                    assert np.array_equal(got.state, rec["state"]), "state " + tag
                    _check(got, rec["cases"][(lim, d, s)], tag)
            again = eng.reach(src, dname, lim)
            assert np.array_equal(again.hops, got.hops), "repeat hops " + tag
            assert np.array_equal(again.state, got.state), "repeat state " + tag
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the reach calls" % t


def _info(ref, t, lim, d, s):
    return ref["at"][t]["cases"][(lim, d, s)][1]


def test_full_view_inputs_exercise_the_paths():
    m = _reference("full", "main")
    for t, rec in m["at"].items():
        for (lim, d, s), (hops, info) in rec["cases"].items():
            assert info["reached"] == info["alive"], (t, lim, d, s)        # 2,948 of 2,948 later
            assert 1 <= info["depth"] <= 2, (t, lim, d, s)
            assert (hops[rec["state"] != ro.ALIVE] == -1).all()
    assert all(_info(m, t, 32, d, "zero")["levels"] == 2 for t in (0, 1) for d in (ro.FROM, ro.TO))
    assert _info(m, 12, 32, ro.FROM, "high")["levels"] == 3
    assert np.bincount(m["at"][12]["cases"][(3, ro.FROM, "zero")][0][m["at"][12]["state"] == ro.ALIVE]).size == 3
    assert _info(m, 40, 32, ro.FROM, "zero")["alive"] == 2948
    assert all(m["at"][t]["dead_entries"] > 0 for t in (12, 20, 33, 40))   # stale rows of the dead
    assert _info(m, 12, 32, ro.FROM, "multi")["sources"] == 2              # duplicate, crashed
    j = _reference("full", "join")
    assert _info(j, 5, 32, ro.FROM, "zero")["alive"] == 120
    assert _info(j, 5, 32, ro.FROM, "zero")["reached"] == 100              # 20 joiners unlisted
    assert _info(j, 5, 32, ro.TO, "zero")["reached"] == 120
    for t in (5, 20):                                                      # 599 has not started
        i = _info(j, t, 32, ro.FROM, "high")
        assert (i["sources"], i["reached"], i["depth"], i["levels"]) == (0, 0, -1, 0)
        assert (j["at"][t]["cases"][(32, ro.FROM, "high")][0] == -1).all()
    assert all(_info(j, 35, 32, d, "zero")["reached"] == 582 == _info(j, 35, 32, d, "zero")["alive"]
               for d in (ro.FROM, ro.TO))


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_reach_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _reference("full", "main"))


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_reach_join_schedule(layout):
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **layout,
                     **w["kw"]) as eng:
        _run(eng, w, _reference("full", "join"))


def test_full_view_reach_tfail_swim_default_age_limit():
    w = FULL["variants"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("full", "variants"))
        got = eng.reach(0)
        assert got.info["age_limit"] == 4 and got.info["direction"] == ro.FROM
        _check(got, _reference("full", "variants")["at"][13]["cases"][(4, ro.FROM, "zero")], "reach(0)")


def test_partial_view_inputs_exercise_the_paths():
    a = _reference("pview", "A")
    assert all(_info(a, 0, 32, d, "zero")["depth"] >= 100 for d in (ro.FROM, ro.TO))   # the lattice
    assert _info(a, 0, 32, ro.FROM, "zero")["levels"] == 129 and _info(a, 1, 32, ro.FROM, "zero")["levels"] == 66
    short = [(t, s) for t, rec in a["at"].items() for (lim, d, s), (_, i) in rec["cases"].items()
             if d == ro.TO and lim == 3 and i["sources"] and i["reached"] < i["alive"]]
    assert short, "no TO case with age limit 3 leaves a live node out"
    assert all(i["reached"] == i["alive"] for (lim, d, s), (_, i) in a["at"][25]["cases"].items()
               if d == ro.FROM)
    b = _reference("pview", "B")["at"][40]
    for d in (ro.FROM, ro.TO):
        i = b["cases"][(32, d, "zero")][1]
        assert 0 < i["reached"] < i["alive"], d
    orphans = (b["state"] == ro.ALIVE) & (b["listed"] == 0)
    orphans[0] = False                                                     # unless it is a source
    assert orphans.any(), "no live orphan"
    for lim in (32, 3, 9):
        assert (b["cases"][(lim, ro.FROM, "zero")][0][orphans] == -1).all()


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_reach_matches_oracle(group):
    w = PVIEW["A"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "A"))


def test_partial_view_reach_drain_all():
    w = PVIEW["B"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "B"))


@pytest.mark.parametrize("make", [lambda: ScaleEngine(64, max_ticks=2),
                                  lambda: PviewEngine(64, view=8, max_ticks=2)],
                         ids=["full", "pview"])
def test_reach_argument_errors(make):
    with make() as eng:
        for bad in (0, 33):
            with pytest.raises(GspError, match="age_limit"):
                eng.reach(0, "from", bad)
        with pytest.raises(GspError):
            eng.reach(0, 2)
        with pytest.raises(GspError):
            eng.reach([])
        for bad in (-1, 64):
            with pytest.raises(GspError):
                eng.reach(bad)
            with pytest.raises(GspError):
                eng.reach([0, bad], "to")
        assert eng.reach(0).info["reached"] >= 1         # the engine still answers
