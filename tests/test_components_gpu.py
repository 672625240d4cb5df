"""Overlay components (gsp_scale_components / gsp_pview_components) against the CPU oracle.

The expected labels are always tests/components_oracle.py's (a numpy min-label propagation and an
iterative Tarjan) over the oracle's rows, never the engine's own row().  Every oracle workload
runs once per module and the cases that share a workload share its record.  At the listed ticks
both kinds of every age limit are compared: label exactly, state, and every info field but
kernel_ms, sweeps and rounds.  A repeated call is identical, and at the end every tick's digest
still equals the oracle's.

The workloads: a 2,048-node view-8 lattice with a crashed block, whose early ticks fall into
hundreds of strong components with a condensation 194 components deep (one shard and three row
shards); its fanout-1 form, which falls into weak components too; the reach tests' drain-all
partial view (a giant component, pairs and singletons); a fanout-1 full view (fused, 2,048-column
tiles with a ragged tile, three row shards) at a fragmented tick, past the mod-32 wrap and at
tick 0; and the reach tests' join schedule, where the nodes not started get -1.

What the inputs exercise is asserted from the oracle's record itself, not from the engine.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd import components, reach_multi
from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_BLOCK, FAIL_RANDOM, ScaleEngine, make_policy
from tests import components_oracle as co
from tests import reach_multi_oracle as rm
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

KINDS = (("weak", co.WEAK), ("strong", co.STRONG))
LATTICE = dict(view=8, fanout=2, inbox=7, tremove=9, fail_mode=FAIL_BLOCK, fail_tick=0, fail_ppm=100000, seed=77)

# at: tick -> the age limits compared there (both kinds each)
FULL = {
    # T = 33 lies past the mod-32 wrap; limit 1 leaves only the entries refreshed at T
    "main": dict(n=3000, ticks=33, pol=None, at={0: [32], 10: [1], 33: [1]},
                 kw=dict(fanout=1, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000, seed=3003)),
    # FULL["join"] of the reach tests: node i starts at int(0.05 i)
    "join": dict(n=600, ticks=20, pol=dict(step_rate=0.05, intro_list=8), at={5: [32], 20: [1]},
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000, seed=600)),
}
PVIEW = {
    "block": dict(n=2048, ticks=5, at={2: [1], 3: [1, 32], 5: [1]}, kw=LATTICE),
    "fan1": dict(n=2048, ticks=8, at={1: [1], 8: [1]}, kw=dict(LATTICE, fanout=1, inbox=0)),
    # PVIEW["B"] of the reach tests
    "B": dict(n=1000, ticks=40, at={40: [3, 32]},
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
}
DEEP = ("pview", "block", 3, 1)               # the condensation of depth 194


@functools.lru_cache(maxsize=None)
def _reference(form, name):
    """One oracle run: the digests, the `few` source set, and per listed tick the state, the
    edges and the expected() of every (age limit, kind)."""
    pview = form == "pview"
    w = (PVIEW if pview else FULL)[name]
    n = w["n"]
    if pview:
        orc = PviewOracle(n, **w["kw"])
    else:
        orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    ref = {"digest": [None], "few": rm.few(orc, n), "at": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t not in w["at"]:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        rec = {"state": state, "edges": edges, "cases": {}}
        for lim in w["at"][t]:
            for _, k in KINDS:
                rec["cases"][(lim, k)] = co.expected(n, t, state, edges, lim, k)
        ref["at"][t] = rec
    orc.close()
    return ref


def _case(ref, t, lim, kind):
    return ref["at"][t]["cases"][(lim, kind)]


def _check(got, want, state, tag):
    assert got.tick == want["info"]["tick"] and got.label.dtype == np.int32, tag
    assert np.array_equal(got.state, state), "state " + tag
    assert np.array_equal(got.label, want["label"]), "label %s: %d differ" % (tag, int((got.label != want["label"]).sum()))
    for f in co.INFO:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])
    assert got.converged and got.info["kernel_ms"] > 0, tag
    assert 1 <= got.info["sweeps"] <= got.info["rounds"] <= components.DEFAULT_SWEEPS, tag


def _run(eng, w, ref):
    """Step to the end, both kinds of every age limit at the listed ticks, digests at the end."""
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        rec = ref["at"][t]
        for lim in w["at"][t]:
            for kname, k in KINDS:
                got = eng.components(kname, lim)
                tag = "tick %d %s age_limit %d" % (t, kname, lim)
                _check(got, rec["cases"][(lim, k)], rec["state"], tag)
                again = eng.components(kname, lim)
                assert np.array_equal(again.label, got.label) and np.array_equal(again.state, got.state), tag
                assert all(again.info[f] == got.info[f] for f in co.INFO), "repeat " + tag
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the components calls" % t


def _nontrivial(case):
    return int((case["sizes"] >= 2).sum())


def test_partial_view_inputs_exercise_the_paths():
    b = _reference("pview", "block")
    s, w = _case(b, 2, 1, co.STRONG), _case(b, 2, 1, co.WEAK)
    assert (s["info"]["components"], _nontrivial(s), s["info"]["largest"]) == (1114, 90, 99)
    assert (w["info"]["components"], _nontrivial(w)) == (31, 3)
    s = _case(b, 3, 1, co.STRONG)
    assert (s["info"]["components"], _nontrivial(s)) == (881, 99)
    rec = b["at"][3]
    assert co.depth(2048, 3, rec["edges"], 1, s["label"]) == 194         # deep for trimming and colouring
    assert _case(b, 5, 1, co.STRONG)["sizes"][:3].tolist() == [722, 444, 249]      # three side by side
    for k in (co.WEAK, co.STRONG):
        assert _case(b, 3, 32, k)["sizes"].tolist() == [1844]
    assert (rec["state"] == ro.CRASHED).sum() == 204                   # the crashed block: rows never read
    f = _reference("pview", "fan1")
    w, s = _case(f, 1, 1, co.WEAK), _case(f, 1, 1, co.STRONG)
    assert (w["info"]["components"], _nontrivial(w), w["info"]["largest"]) == (180, 109, 453)
    assert s["info"]["components"] == s["info"]["singletons"] == 1844
    w = _case(f, 8, 1, co.WEAK)
    assert w["info"]["components"] == 33 and w["sizes"][:3].tolist() == [826, 317, 247]
    p = _reference("pview", "B")
    s, w = _case(p, 40, 3, co.STRONG), _case(p, 40, 3, co.WEAK)
    assert s["sizes"].tolist() == [811, 2, 2] + [1] * 147 and w["sizes"].tolist() == [953, 2] + [1] * 7
    assert _case(p, 40, 32, co.STRONG)["sizes"].tolist() == [952, 2] + [1] * 8
    # a component's label is its smallest id: not every label is a small one
    assert _case(b, 2, 1, co.STRONG)["label"].max() > 2000


def test_full_view_inputs_exercise_the_paths():
    m = _reference("full", "main")
    w, s = _case(m, 10, 1, co.WEAK), _case(m, 10, 1, co.STRONG)
    assert (w["info"]["components"], _nontrivial(w)) == (28, 12)
    assert s["info"]["components"] == 2576 and s["sizes"][:5].tolist() == [352, 11, 10, 2, 2] and _nontrivial(s) == 5
    assert (m["at"][10]["state"] == ro.CRASHED).sum() == 52
    s = _case(m, 33, 1, co.STRONG)                                      # past the mod-32 wrap
    assert s["info"]["components"] > 1000 and s["info"]["largest"] > 1000
    assert _case(m, 33, 1, co.WEAK)["info"]["components"] == 1
    for k in (co.WEAK, co.STRONG):
        assert _case(m, 0, 32, k)["sizes"].tolist() == [3000]
    j = _reference("full", "join")
    s = _case(j, 5, 32, co.STRONG)
    assert s["sizes"].tolist() == [100] + [1] * 20
    assert (j["at"][5]["state"] == ro.NOT_STARTED).sum() == 480 and (s["label"][120:] == -1).all()
    assert _case(j, 20, 1, co.STRONG)["info"]["components"] > 100


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_block_crash_matches_oracle(group):
    w = PVIEW["block"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "block"))


def test_partial_view_fanout_one_matches_oracle():
    w = PVIEW["fan1"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "fan1"))


def test_partial_view_drain_all_and_the_other_probes():
    """PVIEW["B"], and on the same engine: strong.of(s) has the size bowtie() gives for s, weak.of(s)
    holds every node either reach direction marks, and every strong component lies in one weak
    one."""
    w = PVIEW["B"]
    ref = _reference("pview", "B")
    few = ref["few"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, ref)
        for lim in (3, 32):
            strong, weak = eng.components("strong", lim), eng.components("weak", lim)
            frm, to = eng.reach_multi(few, "from", lim, hops=False), eng.reach_multi(few, "to", lim, hops=False)
            scc = reach_multi.bowtie(frm, to)["scc"]
            fs, ts = frm.sets(), to.sets()
            for b, s in enumerate(few):
                assert strong.of(s).size == scc[b], (lim, s)
                assert np.array_equal(np.isin(np.arange(w["n"]), strong.of(s)), fs[b] & ts[b]), (lim, s)
                assert np.isin(np.nonzero(fs[b] | ts[b])[0], weak.of(s)).all(), (lim, s)
            labels, counts = components.nesting(strong, weak)
            assert labels.tolist() == sorted(set(weak.label[weak.label >= 0].tolist()))
            assert counts.sum() == strong.info["components"]
    assert ref["at"][40]["state"][few[1]] == ro.CRASHED and sorted(scc.tolist())[0] == 0


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _reference("full", "main"))


def test_full_view_join_schedule():
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        _run(eng, w, _reference("full", "join"))


def test_max_sweeps_caps_the_deep_case():
    form, name, t, lim = DEEP
    w = PVIEW[name]
    want = _case(_reference(form, name), t, lim, co.STRONG)
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        eng.step(t)
        capped = eng.components("strong", lim, max_sweeps=2)
        assert not capped.converged and capped.info["converged"] == 0 and capped.info["sweeps"] <= 2
        assert capped.info["components"] == 0 and capped.info["alive"] == want["info"]["alive"]
        with pytest.raises(ValueError, match="did not converge"):
            capped.summary()
        full = eng.components("strong", lim)                            # the default cap
        assert full.converged and np.array_equal(full.label, want["label"])
        assert full.info["sweeps"] > 2
        assert full.summary()["components"] == 881
        wk = eng.components("weak", lim, max_sweeps=1)
        assert not wk.converged and wk.info["sweeps"] == 1


@pytest.mark.parametrize("make", [lambda: ScaleEngine(64, max_ticks=2),
                                  lambda: PviewEngine(64, view=8, max_ticks=2)],
                         ids=["full", "pview"])
def test_components_arguments(make):
    with make() as eng:
        name = eng._abi + "_components"
        with pytest.raises(GspError, match=name + ": kind=2"):
            eng.components(2)
        for bad in (0, 33):
            with pytest.raises(GspError, match=name + ": age_limit"):
                eng.components("weak", bad)
        with pytest.raises(GspError, match=name + ": max_sweeps=-1"):
            eng.components("weak", 9, -1)
        fn, what = eng._probe("components")                             # every output may be NULL
        for kind in (0, 1):
            assert fn(eng._h, kind, 9, 0, None, None, None) == 0
        for kname, _ in KINDS:                                         # T = 0: one component
            got = eng.components(kname)
            assert got.info["age_limit"] == eng.params.tremove
            assert got.label.tolist() == [0] * 64 and got.info["components"] == 1 and got.info["largest"] == 64
            assert got.info["largest_label"] == 0 and got.info["singletons"] == 0 and got.converged


def test_components_beside_open_per_tick_probes():
    """A rumor trace, a detection ledger and a traffic ledger open on the engine: the labels are
    the oracle's, and the digests are untouched."""
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
