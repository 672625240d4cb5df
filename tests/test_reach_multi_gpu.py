"""Multi-source reach (gsp_scale_reach_multi / gsp_pview_reach_multi) against the CPU oracle.

The expected arrays are always tests/reach_multi_oracle.py's stack of single-source numpy BFS over
the oracle's rows, never the engine's own row().  Every oracle workload runs once per module and
the cases that share a workload share its record.  The workloads are the reach tests', restated:
the smallest shapes that still reach every row form (a fused full view, 2,048-column tiles with a
ragged 952-column tile, three in-process row shards, a join schedule, a bounded and a drain-all
partial view).  At the listed ticks both directions of every (age limit, source set) are compared:
the hops matrix, seen, reached, ecc, sum_hops, level_sizes, state and every info field but
kernel_ms.  Source sets: `one` = [0]; `few` = five ids with a duplicate, a crashed node and the
highest id (not started under the join schedule); `sample` = the 64-id sample of
reach_multi_oracle.sample, which fills the high bits.  For `few` every row is also compared with
the engine's own reach() of that single source.  A repeated call is identical, and at the end
every tick's digest still equals the oracle's.

What the inputs exercise is asserted from the oracle's record itself, not from the engine.
"""
import ctypes
import functools

import numpy as np
import pytest

from gossip_protocol_amd import reach_multi
from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests import reach_multi_oracle as rm
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

DIRS = (("from", ro.FROM), ("to", ro.TO))
ARRAYS = ("hops", "seen", "reached", "ecc", "sum_hops", "level_sizes")

# at: tick -> the (age limit, source set) pairs compared there; None: the default (tremove)
FULL = {
    # T = 33 lies past the mod-32 wrap; limit 1 leaves only the entries refreshed at T
    "main": dict(n=3000, ticks=33, pol=None,
                 at={0: [(32, "one")], 12: [(1, "sample"), (32, "few")], 33: [(1, "sample"), (None, "few")]},
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): at T = 5 exactly the nodes >= 120 have not started
    "join": dict(n=600, ticks=20, pol=dict(step_rate=0.05, intro_list=8),
                 at={5: [(32, "sample"), (3, "few")], 20: [(32, "sample"), (1, "few")]},
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
}
PVIEW = {
    "A": dict(n=4096, ticks=12,
              at={0: [(32, "sample")], 1: [(32, "sample")], 12: [(3, "sample"), (32, "few"), (None, "one")]},
              kw=dict(view=32, fanout=3, inbox=7, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=4128)),
    "B": dict(n=1000, ticks=40, at={12: [(3, "few")], 40: [(3, "sample"), (32, "few")]},
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
}
SMALL_CAP = 5                                 # a level_cap below the depth of A at T = 0 (128)


def _limit(lim, kw):
    return lim if lim is not None else kw["tremove"]


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    """One oracle run: the digests, the source sets, and per listed tick the state and the
    expected() of every (age limit, direction, source set)."""
    pview = kind == "pview"
    w = (PVIEW if pview else FULL)[name]
    n = w["n"]
    if pview:
        orc = PviewOracle(n, **w["kw"])
    else:
        orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    sets = {"one": [0], "few": rm.few(orc, n), "sample": [int(v) for v in rm.sample(n)]}
    ref = {"digest": [None], "sets": sets, "at": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t not in w["at"]:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        rec = {"state": state, "cases": {}}
        for l, s in w["at"][t]:
            lim = _limit(l, w["kw"])
            for _, d in DIRS:
                adj = ro.graph(n, t, edges, lim, d)
                rec["cases"][(lim, d, s)] = rm.expected(n, t, state, adj, lim, d, sets[s])
        ref["at"][t] = rec
    orc.close()
    return ref


def _check(got, want, tag):
    assert got.tick == want["info"]["tick"], tag
    assert got.hops.dtype == np.int32 and got.seen.dtype == np.uint64, tag
    for a in ARRAYS:
        g, e = getattr(got, a), want[a]
        assert g.shape == e.shape, "%s %s: shape %s != %s" % (a, tag, g.shape, e.shape)
        assert np.array_equal(g, e), "%s %s: %d differ" % (a, tag, int((g != e).sum()))
    for f in rm.INFO:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])
    assert got.info["kernel_ms"] > 0, tag


def _check_rows_against_reach(eng, got, src, dname, lim, tag):
    """Row b of the multi-source result is the engine's own reach() of sources[b] alone."""
    for b, s in enumerate(src):
        one = eng.reach(int(s), dname, lim)
        assert np.array_equal(got.hops[b], one.hops), "%s: row %d is not reach(%d)" % (tag, b, s)
        live = one.info["sources"] == 1
        assert got.reached[b] == one.info["reached"] and got.ecc[b] == one.info["depth"], (tag, b)
        assert got.sum_hops[b] == one.info["sum_hops"], (tag, b)
        assert np.array_equal((got.seen >> np.uint64(b)) & np.uint64(1), one.hops >= 0), (tag, b)
        assert live or (got.reached[b] == 0 and got.ecc[b] == -1 and (got.hops[b] == -1).all()), (tag, b)


def _run(eng, w, ref):
    """Step to the end, every case at the listed ticks, digests at the end."""
    got = None
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        rec = ref["at"][t]
        for dname, d in DIRS:
            for l, s in w["at"][t]:
                lim, src = _limit(l, w["kw"]), ref["sets"][s]
                got = eng.reach_multi(src, dname) if l is None else eng.reach_multi(src, dname, l)
                tag = "tick %d %s age_limit %d sources %s" % (t, dname, lim, s)
                assert np.array_equal(got.state, rec["state"]), "state " + tag
                _check(got, rec["cases"][(lim, d, s)], tag)
                if s == "few":
                    _check_rows_against_reach(eng, got, src, dname, lim, tag)
            again = eng.reach_multi(src, dname, lim)
            for a in ARRAYS + ("state",):
                assert np.array_equal(getattr(again, a), getattr(got, a)), "repeat %s %s" % (a, tag)
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the reach_multi calls" % t


def _case(ref, t, lim, d, s):
    return ref["at"][t]["cases"][(lim, d, s)]


def _rows(seen_hops):
    """The number of different rows of a hops >= 0 matrix, the empty rows of sources that are
    not alive included."""
    return len({row.tobytes() for row in seen_hops >= 0})


def test_full_view_inputs_exercise_the_paths():
    m = _reference("full", "main")
    for t in (12, 33):                                   # 33: past the mod-32 wrap
        f, to = _case(m, t, 1, ro.FROM, "sample"), _case(m, t, 1, ro.TO, "sample")
        alone = (f["reached"] == 1) & (f["ecc"] == 0)
        assert alone.any() and (to["reached"][alone] >= 2800).all(), t     # only itself; 2,800+ reach it
        assert f["ecc"].max() == 3 and to["ecc"].max() == 3, t
        assert f["info"]["alive_sources"] < f["info"]["n_sources"] == 63, t
    assert len(set(m["sets"]["few"])) == 4 and m["at"][12]["state"][m["sets"]["few"][1]] == ro.CRASHED
    j = _reference("full", "join")
    assert _case(j, 5, 32, ro.FROM, "sample")["info"]["alive_sources"] == 63 - 50      # 50 not started
    assert j["at"][5]["state"][j["sets"]["few"][4]] == ro.NOT_STARTED
    assert (_case(j, 20, 32, ro.TO, "sample")["reached"] == 1).any()
    assert _rows(_case(j, 20, 32, ro.FROM, "sample")["hops"]) >= 3


def test_partial_view_inputs_exercise_the_paths():
    a = _reference("pview", "A")
    for d in (ro.FROM, ro.TO):
        e = _case(a, 0, 32, d, "sample")
        assert (e["reached"] == 4096).all() and (e["ecc"] == 128).all(), d         # the lattice
        assert e["info"]["depth"] > SMALL_CAP
        e = _case(a, 1, 32, d, "sample")
        assert e["ecc"].min() >= 64 and e["ecc"].max() <= 66, d
    f, to = _case(a, 12, 3, ro.FROM, "sample"), _case(a, 12, 3, ro.TO, "sample")
    assert ((f["reached"] == 1) & (to["reached"] >= 3830)).any()
    assert f["info"]["n_sources"] - f["info"]["alive_sources"] == 2
    assert rm.distinct_sets(f) >= 3
    b = _reference("pview", "B")
    f, to = _case(b, 40, 3, ro.FROM, "sample"), _case(b, 40, 3, ro.TO, "sample")
    assert _rows(f["hops"]) >= 10                       # 9 among the alive sources, and the empty row
    live = f["ecc"] >= 0
    assert f["reached"][live].min() == 1 and f["reached"][live].max() == 944
    assert set(rm.component_sizes(f, to).tolist()) == {0, 1, 811}
    assert f["info"]["n_sources"] - f["info"]["alive_sources"] == 3


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_reach_multi_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _reference("full", "main"))


def test_full_view_reach_multi_join_schedule():
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        _run(eng, w, _reference("full", "join"))


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_reach_multi_matches_oracle(group):
    w = PVIEW["A"]
    ref = _reference("pview", "A")
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        # a level_cap below the depth drops the deeper levels from level_sizes only
        for dname, d in DIRS:
            want = _case(ref, 0, 32, d, "sample")
            got = eng.reach_multi(ref["sets"]["sample"], dname, 32, level_cap=SMALL_CAP)
            assert got.level_sizes.shape == (63, SMALL_CAP)
            assert np.array_equal(got.level_sizes, want["level_sizes"][:, :SMALL_CAP]), dname
            for a in ("hops", "seen", "reached", "ecc", "sum_hops"):
                assert np.array_equal(getattr(got, a), want[a]), (a, dname)
        _run(eng, w, ref)


def test_partial_view_reach_multi_drain_all():
    w = PVIEW["B"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "B"))


def test_bowtie_and_summary_of_the_drain_all_overlay():
    """ReachMulti.summary() and bowtie() on engine results, against the oracle's stack."""
    w = PVIEW["B"]
    ref = _reference("pview", "B")
    src = ref["sets"]["sample"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        eng.step(40)
        frm, to = eng.reach_multi(src, "from", 3, hops=False), eng.reach_multi(src, "to", 3, hops=False)
    f, t = _case(ref, 40, 3, ro.FROM, "sample"), _case(ref, 40, 3, ro.TO, "sample")
    assert frm.hops is None and np.array_equal(frm.seen, f["seen"]) and np.array_equal(to.seen, t["seen"])
    s = frm.summary()
    assert s["distinct_sets"] == rm.distinct_sets(f) and s["alive_sources"] == 60
    assert s["diameter_bound"] == f["info"]["depth"] and (s["reached_min"], s["reached_max"]) == (1, 944)
    assert s["mean_hops"] == f["info"]["sum_hops"] / f["info"]["pairs"]
    bt = reach_multi.bowtie(frm, to)
    fh, th = f["hops"] >= 0, t["hops"] >= 0
    assert np.array_equal(bt["scc"], rm.component_sizes(f, t))
    assert np.array_equal(bt["downstream"], (fh & ~th).sum(axis=1))
    assert np.array_equal(bt["upstream"], (th & ~fh).sum(axis=1))
    assert np.array_equal(bt["scc"] + bt["downstream"] + bt["upstream"] + bt["neither"],
                          np.full(len(src), f["info"]["alive"]))
    core = np.nonzero(bt["scc"] == 811)[0]
    assert bt["same"][core[0], core[-1]] and not bt["same"][core[0], np.nonzero(bt["scc"] == 1)[0][0]]


@pytest.mark.parametrize("make", [lambda: ScaleEngine(64, max_ticks=2),
                                  lambda: PviewEngine(64, view=8, max_ticks=2)],
                         ids=["full", "pview"])
def test_reach_multi_arguments(make):
    with make() as eng:
        name = eng._abi + "_reach_multi"
        with pytest.raises(GspError, match=name + ": n_sources=0"):
            eng.reach_multi([])
        with pytest.raises(GspError, match=name + ": n_sources=65"):
            eng.reach_multi(list(range(64)) + [0])
        with pytest.raises(GspError, match=name + ": sources"):
            eng.reach_multi([0, 64])
        with pytest.raises(GspError, match=name + ": direction=2"):
            eng.reach_multi([0], 2)
        for bad in (0, 33):
            with pytest.raises(GspError, match=name + ": age_limit"):
                eng.reach_multi([0], "from", bad)
        # every output may be NULL
        fn, what = eng._probe("reach_multi")
        src = (ctypes.c_int32 * 2)(0, 63)
        assert fn(eng._h, 0, 9, src, 2, None, None, None, None, None, None, 0, None, None) == 0
        full = eng.reach_multi(list(range(64)), "to")                # all 64 bits
        assert full.info["alive_sources"] == 64 and (full.ecc >= 0).all()
        assert (full.seen[full.state == 1] != 0).all()


def test_reach_multi_beside_open_per_tick_probes():
    """A rumor trace, a detection ledger and a traffic ledger open on the engine: the multi-source
    result is the oracle's, and the digests are untouched."""
    w = FULL["join"]
    ref = _reference("full", "join")
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), events=True,
                     event_cap=1 << 20, **w["kw"]) as eng:
        eng.rumor_open(4)
        eng.rumor_seed(0, 0)
        eng.detect_open()
        eng.traffic_open([0, 7])
        _run(eng, w, ref)
        assert eng.rumor(0).info["ticks_traced"] == w["ticks"]
        assert eng.detect().info["ticks_folded"] == w["ticks"]
        assert eng.traffic().info["ticks_counted"] == w["ticks"]
