"""Overlay clustering (gsp_scale_cluster / gsp_pview_cluster) against the CPU oracle.

The expected arrays are always tests/cluster_oracle.py's numpy counts over the oracle's rows, never
the engine's own row().  Every oracle workload runs once per module and the cases that share a
workload share its record.  The workloads are the multi-source reach tests', restated: the
smallest shapes that still reach every row form and every ragged edge (a fused full view,
2,048-column tiles with a ragged 952-column tile, three in-process row shards, a join schedule, a
bounded and a drain-all partial view).  At the listed ticks every (age limit, observer set) is
compared exactly: member, degree, links, mutual, state and every info field but kernel_ms.
Observer sets: `one` = [0]; `edge` = cluster_oracle.edge of that tick and limit (an observer with
no neighbour, one with exactly one where there is one, the one with the most links, one that is
not alive, a duplicate, and n - 1, not started under the join schedule); `sample` = the 63
distinct ids of reach_multi_oracle.sample, which fills the high bits.  A repeated call is
identical, and at the end every tick's digest still equals the oracle's.

What the inputs exercise is asserted from the oracle's record itself, not from the engine.
"""
import ctypes
import functools

import numpy as np
import pytest

from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests import cluster_oracle as co
from tests import reach_multi_oracle as rm
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

# at: tick -> the (age limit, observer set) pairs compared there; None: the default (tremove)
FULL = {
    # T = 33 lies past the mod-32 wrap; limit 1 leaves only the entries refreshed at T
    "main": dict(n=3000, ticks=33, pol=None,
                 at={0: [(32, "one"), (32, "sample")],
                     12: [(1, "sample"), (1, "edge"), (32, "edge"), (None, "sample")],
                     33: [(1, "sample"), (1, "edge"), (None, "edge")]},
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): at T = 5 exactly the nodes >= 120 have not started
    "join": dict(n=600, ticks=20, pol=dict(step_rate=0.05, intro_list=8),
                 at={5: [(32, "sample"), (3, "edge")], 20: [(32, "sample"), (1, "edge"), (None, "one")]},
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
}
PVIEW = {
    "A": dict(n=4096, ticks=12,
              at={0: [(32, "sample")], 1: [(32, "sample")],
                  12: [(3, "sample"), (3, "edge"), (32, "edge"), (None, "one"), (None, "sample")]},
              kw=dict(view=32, fanout=3, inbox=7, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=4128)),
    # T = 40 lies past the mod-32 wrap
    "B": dict(n=1000, ticks=40, at={12: [(3, "edge")], 40: [(3, "sample"), (3, "edge"), (32, "edge"), (None, "sample")]},
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
}


def _limit(lim, kw):
    return lim if lim is not None else kw["tremove"]


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    """One oracle run: the digests and, per listed tick, the state and per age limit the counts
    of every node, the edge set and the expected() of every observer set."""
    pview = kind == "pview"
    w = (PVIEW if pview else FULL)[name]
    n = w["n"]
    if pview:
        orc = PviewOracle(n, **w["kw"])
    else:
        orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    fixed = {"one": [0], "sample": [int(v) for v in rm.sample(n)]}
    assert len(fixed["sample"]) == 63
    ref = {"digest": [None], "at": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t not in w["at"]:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        rec = {"state": state, "cases": {}, "sets": {}, "slots": {}, "counts": {}}
        for l, s in w["at"][t]:
            lim = _limit(l, w["kw"])
            if lim not in rec["counts"]:
                a = co.adjacency(n, ro.graph(n, t, edges, lim, ro.FROM))
                cnt = co.counts(a)
                rec["counts"][lim] = (a, cnt)
                rec["sets"][(lim, "edge")], rec["slots"][lim] = co.edge(n, state, cnt)
            a, cnt = rec["counts"][lim]
            obs = rec["sets"].setdefault((lim, s), fixed.get(s))
            rec["cases"][(lim, s)] = co.expected(n, t, state, a, cnt, lim, obs)
        for lim in rec["counts"]:
            rec["counts"][lim] = rec["counts"][lim][1]        # the matrices are no longer needed
        ref["at"][t] = rec
    orc.close()
    return ref


def _check(got, want, tag):
    assert got.tick == want["info"]["tick"], tag
    assert got.member.dtype == np.uint64 and got.links.dtype == np.uint64, tag
    assert got.degree.dtype == np.uint32 and got.mutual.dtype == np.uint32, tag
    for a in co.ARRAYS:
        g, e = getattr(got, a), want[a]
        assert g.shape == e.shape, "%s %s: shape %s != %s" % (a, tag, g.shape, e.shape)
        assert np.array_equal(g, e), "%s %s: %d differ" % (a, tag, int((g != e).sum()))
    for f in co.INFO:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])
    assert got.info["kernel_ms"] > 0, tag


def _run(eng, w, ref):
    """Step to the end, every case at the listed ticks, digests at the end."""
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        rec = ref["at"][t]
        for l, s in w["at"][t]:
            lim = _limit(l, w["kw"])
            obs = rec["sets"][(lim, s)]
            got = eng.cluster(obs) if l is None else eng.cluster(obs, l)
            tag = "tick %d age_limit %d observers %s" % (t, lim, s)
            assert np.array_equal(got.state, rec["state"]), "state " + tag
            _check(got, rec["cases"][(lim, s)], tag)
        again = eng.cluster(obs, lim)
        for a in co.ARRAYS + ("state",):
            assert np.array_equal(getattr(again, a), getattr(got, a)), "repeat %s %s" % (a, tag)
        assert {f: again.info[f] for f in co.INFO} == {f: got.info[f] for f in co.INFO}, "repeat info " + tag
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the cluster calls" % t


def _alive_counts(rec, lim):
    live = rec["state"] == ro.ALIVE
    degree, links, mutual = rec["counts"][lim]
    return degree[live], links[live], mutual[live]


def test_full_view_inputs_exercise_the_paths():
    m = _reference("full", "main")
    zero = m["at"][0]["cases"][(32, "sample")]
    assert (zero["degree"] == 2999).all() and (zero["links"] == 2999 * 2998).all()         # complete
    assert (zero["mutual"] == 2999).all() and zero["info"]["rows"] == 3000
    k, links, _ = _alive_counts(m["at"][12], 1)
    assert int((k == 0).sum()) == 143 and not (k == 1).any()
    assert m["at"][12]["slots"][1] == ["empty", "top", "dead", "again", "last"]            # no `single`
    clu, density, rec = co.mean_clustering(m["at"][12]["state"], m["at"][12]["counts"][1])
    assert 0.30 < clu < 0.35 and 0.24 < density < 0.28 and 0.23 < rec < 0.28               # a real graph
    assert co.mean_clustering(m["at"][12]["state"], m["at"][12]["counts"][32])[0] > 0.99   # nearly complete
    for t in (12, 33):                                   # 33: past the mod-32 wrap
        e = m["at"][t]["cases"][(1, "sample")]
        assert e["info"]["alive_observers"] < e["info"]["n_observers"] == 63, t
        live = e["degree"] > 0
        assert e["links"].min() == 0 and e["links"].max() > 100000 and len(set(e["links"][live].tolist())) > 40, t
        assert 0 < e["mutual"][live].min() < e["mutual"].max() < e["degree"].max(), t
        assert e["info"]["rows"] < e["info"]["alive"], t                                   # rows are skipped
        g = m["at"][t]["cases"][(1, "edge")]
        ids, slots = m["at"][t]["sets"][(1, "edge")], m["at"][t]["slots"][1]
        assert g["degree"][slots.index("empty")] == 0 and g["degree"][slots.index("dead")] == 0, t
        assert m["at"][t]["state"][ids[slots.index("dead")]] == ro.CRASHED, t
        assert g["links"][slots.index("top")] == g["links"][slots.index("again")] == links_max(m, t, 1), t
    j = _reference("full", "join")
    assert j["at"][5]["cases"][(32, "sample")]["info"]["alive_observers"] == 63 - 50       # 50 not started
    ids, slots = j["at"][5]["sets"][(3, "edge")], j["at"][5]["slots"][3]
    assert j["at"][5]["state"][ids[slots.index("last")]] == ro.NOT_STARTED
    assert j["at"][5]["cases"][(3, "edge")]["degree"][slots.index("last")] == 0


def links_max(ref, t, lim):
    return int(_alive_counts(ref["at"][t], lim)[1].max())


def test_partial_view_inputs_exercise_the_paths():
    a = _reference("pview", "A")
    zero = a["at"][0]["cases"][(32, "sample")]
    assert (zero["degree"] == 32).all() and not zero["links"].any() and not zero["mutual"].any()   # the lattice
    one = a["at"][1]["cases"][(32, "sample")]
    assert one["links"].min() > 300 and 0.6 < co.mean_clustering(a["at"][1]["state"], a["at"][1]["counts"][32])[0] < 0.7
    k, links, _ = _alive_counts(a["at"][12], 3)
    assert int((k == 0).sum()) == 49 and int((k == 1).sum()) == 21
    assert a["at"][12]["slots"][3] == ["empty", "single", "top", "dead", "again", "last"]
    clu, density, rec = co.mean_clustering(a["at"][12]["state"], a["at"][12]["counts"][3])
    assert 0.17 < clu < 0.19 and clu > 20 * density and 0.17 < rec < 0.19
    e = a["at"][12]["cases"][(3, "sample")]
    assert e["info"]["n_observers"] - e["info"]["alive_observers"] == 2
    live = e["degree"] > 0
    assert e["links"].max() > 100 and len(set(e["links"][live].tolist())) > 30
    assert e["mutual"][live].min() < e["mutual"].max()
    assert (np.bincount([bin(int(v)).count("1") for v in e["member"]])[2:] > 0).any()      # shared neighbours
    g = a["at"][12]["cases"][(3, "edge")]
    assert g["degree"].tolist()[:2] == [0, 1] and g["links"][2] == g["links"][4] == links_max(a, 12, 3)
    b = _reference("pview", "B")
    k, _, _ = _alive_counts(b["at"][40], 3)
    assert (k == 0).any() and (k == 1).any()
    assert b["at"][40]["slots"][3] == ["empty", "single", "top", "dead", "again", "last"]
    clu, density, rec = co.mean_clustering(b["at"][40]["state"], b["at"][40]["counts"][3])
    assert 0.34 < clu < 0.38 and 0.12 < rec < 0.16
    assert b["at"][40]["cases"][(3, "sample")]["info"]["n_observers"] - \
        b["at"][40]["cases"][(3, "sample")]["info"]["alive_observers"] == 3


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_cluster_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _reference("full", "main"))


def test_full_view_cluster_join_schedule():
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        _run(eng, w, _reference("full", "join"))


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_cluster_matches_oracle(group):
    w = PVIEW["A"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "A"))


def test_partial_view_cluster_drain_all():
    w = PVIEW["B"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "B"))


def test_summary_and_overlap_of_the_bounded_overlay():
    """Cluster.summary() and overlap() on an engine result, against the oracle's counts."""
    w = PVIEW["A"]
    ref = _reference("pview", "A")
    rec = ref["at"][12]
    obs = rec["sets"][(3, "sample")]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        eng.step(12)
        got = eng.cluster(obs, 3)
    want = rec["cases"][(3, "sample")]
    live = rec["state"][obs] == ro.ALIVE
    assert np.array_equal(got.live, live)
    k = want["degree"][live].astype(np.int64)
    s = got.summary()
    assert s["observers"] == 61 and s["alive"] == want["info"]["alive"]
    assert s["mean_degree"] == k.mean() and s["density"] == k.mean() / (want["info"]["alive"] - 1)
    assert s["transitivity"] == int(want["links"].sum()) / int((k * (k - 1)).sum())
    assert s["reciprocity"] == int(want["mutual"].sum()) / int(k.sum())
    big = k >= 2
    assert s["mean_clustering"] == float((want["links"][live][big] / (k[big] * (k[big] - 1))).mean())
    assert s["clustering_over_density"] > 15
    inter, jac = got.overlap()
    sets = [set(np.nonzero((want["member"] >> np.uint64(b)) & np.uint64(1))[0].tolist()) for b in range(63)]
    assert inter[3, 3] == len(sets[3]) and inter[3, 40] == len(sets[3] & sets[40])
    pairs = [(a, b) for a in range(63) for b in range(a + 1, 63) if live[a] and live[b] and sets[a] | sets[b]]
    assert abs(jac - np.mean([len(sets[a] & sets[b]) / len(sets[a] | sets[b]) for a, b in pairs])) < 1e-12


@pytest.mark.parametrize("make", [lambda: ScaleEngine(64, max_ticks=2),
                                  lambda: PviewEngine(64, view=8, max_ticks=2)],
                         ids=["full", "pview"])
def test_cluster_arguments(make):
    with make() as eng:
        name = eng._abi + "_cluster"
        with pytest.raises(GspError, match=name + ": n_observers=0"):
            eng.cluster([])
        with pytest.raises(GspError, match=name + ": n_observers=65"):
            eng.cluster(list(range(64)) + [0])
        with pytest.raises(GspError, match=name + ": observers"):
            eng.cluster([0, 64])
        with pytest.raises(GspError, match=name + ": observers"):
            eng.cluster([-1])
        for bad in (0, 33):
            with pytest.raises(GspError, match=name + ": age_limit"):
                eng.cluster([0], bad)
        # every output may be NULL
        fn, what = eng._probe("cluster")
        obs = (ctypes.c_int32 * 2)(0, 63)
        assert fn(eng._h, 9, obs, 2, None, None, None, None, None, None) == 0
        full = eng.cluster(list(range(64)))                          # all 64 bits
        assert full.info["alive_observers"] == 64 and full.info["n_observers"] == 64
        assert (full.degree > 0).all() and (full.member != 0).all() and full.info["rows"] == 64
        if eng._abi == "gsp_scale":                                  # tick 0: the complete graph
            assert (full.degree == 63).all() and (full.links == 63 * 62).all() and (full.mutual == 63).all()
            assert (full.member == [~np.uint64(1 << x) for x in range(64)]).all()


def test_cluster_beside_open_per_tick_probes():
    """A rumor trace, a detection ledger and a traffic ledger open on the engine: the clustering
    is the oracle's, and the digests are untouched."""
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
