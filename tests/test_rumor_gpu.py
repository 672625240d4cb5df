"""Rumor trace (gsp_scale_rumor_* / gsp_pview_rumor_*) against the numpy rule over the CPU oracle.

The expected arrays come from tests/rumor_oracle.py, which reads only the oracle's messages(),
joinreps(), start_tick() and fail_tick() -- never engine output.  Every oracle workload runs once
per module; the cases that share one share its record.  A trace of four rumors is opened at tick
0 and seeded
  rumor 0  at node 0 at tick 0,
  rumor 1  at a high id at tick 0,
  rumor 2  mid-run, with a duplicate and a node the schedule has crashed among its sources,
  rumor 3  at a source that is not alive (a join schedule: the last joiner before it starts,
           seeded again once it has; otherwise a crashed node),
the engine is stepped one tick at a time, and at the listed ticks every rumor is compared: heard
array for array, known, state and every info field but kernel_ms (> 0).  A repeated get is
identical, and at the end every tick's digest equals the oracle's.

What the inputs exercise is asserted from the oracle's own record: a segment past 64 (the
wave-cooperative path), an inbox cut that withholds a new bit, a rumor carried by a JOINREP, a
live node left out and a rumor with no alive source.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests import rumor_oracle as ru
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

RUMORS = 4
INFO = ("tick", "n", "rumor", "seed_tick", "sources", "alive", "known", "known_alive", "last_heard",
        "ticks_traced")
JOIN = dict(step_rate=0.05, intro_list=8)

FULL = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes
    "main": dict(n=3000, ticks=40, at=(0, 1, 12, 25, 40), high=2999, mid=12, pol=None,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): 599 starts at tick 29
    "join": dict(n=600, ticks=35, at=(0, 5, 20, 35), high=599, mid=15, late=30, pol=JOIN,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
    # node i starts at int(0.01 i): 100 nodes per tick, whose JOINREP answers land on node 0
    "burst": dict(n=600, ticks=20, at=(1, 3, 8, 20), high=599, mid=12, late=8,
                  pol=dict(step_rate=0.01, intro_list=8),
                  kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                          seed=600)),
    # TFAIL + SWIM: probes carry nothing
    "variants": dict(n=1024, ticks=13, at=(6, 13), high=1023, mid=6, pol=None,
                     kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                             seed=3003, tfail=4, swim=2)),
}

_A = dict(view=32, fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=50000, seed=4128)
PVIEW = {
    "A7": dict(n=4096, ticks=40, at=(0, 1, 12, 25, 40), high=4000, mid=12, pol=None, kw=dict(inbox=7, **_A)),
    "A2": dict(n=4096, ticks=40, at=(12, 40), high=4000, mid=12, pol=None, kw=dict(inbox=2, **_A)),
    "A0": dict(n=4096, ticks=40, at=(12, 40), high=4000, mid=12, pol=None, kw=dict(inbox=0, **_A)),
    "B": dict(n=1000, ticks=40, at=(12, 40), high=900, mid=12, pol=None,
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
    # node i starts at int(0.02 i): 250 at tick 5, the last joiner 1199 at tick 23
    "join": dict(n=1200, ticks=40, at=(6, 20, 30, 40), high=250, high_at=6, mid=20, late=30,
                 pol=dict(step_rate=0.02, intro_list=8),
                 kw=dict(view=32, fanout=3, inbox=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10,
                         fail_ppm=30000, seed=77)),
}


def _oracle(kind, name):
    w = (PVIEW if kind == "pview" else FULL)[name]
    pol = oracle_policy(**w["pol"]) if w["pol"] else None
    return (PviewOracle if kind == "pview" else ScaleOracle)(w["n"], policy=pol, **w["kw"])


def _seeds(w, start, fail):
    """The seed plan of a workload, from the schedule alone."""
    n, mid = w["n"], w["mid"]
    dead = int(np.nonzero(fail < mid)[0][0])                  # crashed before `mid`
    ok = np.nonzero((start <= mid) & (fail >= w["ticks"]))[0]  # alive at `mid` and to the end
    a, b = int(ok[len(ok) // 3]), int(ok[2 * len(ok) // 3])
    plan = {0: [(0, [0])]}
    plan.setdefault(w.get("high_at", 0), []).append((1, [w["high"]]))
    plan.setdefault(mid, []).append((2, [a, dead, a, b]))
    if w["pol"]:                                              # n - 1 starts late: not alive at 0
        assert start[n - 1] > 0 and start[n - 1] <= w["late"] <= fail[n - 1]
        plan[0].append((3, [n - 1]))
        plan.setdefault(w["late"], []).append((3, [n - 1]))
    else:
        plan[mid].append((3, [dead]))
    return plan


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    w = (PVIEW if kind == "pview" else FULL)[name]
    orc = _oracle(kind, name)
    start, fail = ru.schedule(orc, w["n"])
    seeds = _seeds(w, start, fail)
    ref = ru.run(orc, w["n"], w["ticks"], w["kw"].get("inbox", 0), RUMORS, seeds, set(w["at"]))
    ref["seeds"] = seeds
    orc.close()
    return ref


def _compare(got, want, tag):
    heard, state, known, info = want
    assert got.heard.dtype == np.int32 and got.tick == info["tick"], tag
    assert np.array_equal(got.heard, heard), "heard %s: %d differ" % (tag, int((got.heard != heard).sum()))
    assert np.array_equal(got.known, known), "known %s: %s != %s" % (tag, got.known.tolist(), known.tolist())
    assert np.array_equal(got.state, state), "state " + tag
    for f in INFO:
        assert got.info[f] == info[f], "info.%s %s: %r != %r" % (f, tag, got.info[f], info[f])


def _run(eng, w, ref, chunk=1):
    """Open at tick 0, seed by the plan, compare at the listed ticks, digests at the end."""
    eng.rumor_open(RUMORS)
    for t in range(0, w["ticks"] + 1, chunk):
        if t:
            eng.step(chunk)
        for rumor, sources in ref["seeds"].get(t, ()):
            eng.rumor_seed(rumor, sources[0] if len(sources) == 1 else sources)
        if t not in ref["at"]:
            continue
        for b in range(RUMORS):
            got = eng.rumor(b)
            _compare(got, ref["at"][t][b], "tick %d rumor %d" % (t, b))
            if t:
                assert got.info["kernel_ms"] > 0, (t, b)
        again = eng.rumor(RUMORS - 1)
        assert np.array_equal(again.heard, got.heard) and np.array_equal(again.known, got.known)
        assert np.array_equal(again.state, got.state)
        assert {f: again.info[f] for f in INFO} == {f: got.info[f] for f in INFO}
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d with a trace open" % t


def _final(ref, rumor):
    return ref["at"][max(ref["at"])][rumor]


def test_full_view_inputs_exercise_the_paths():
    m = _reference("full", "main")
    for b in (0, 1, 2):                                  # every live node hears, 9-11 ticks on
        heard, state, _, info = _final(m, b)
        assert info["known_alive"] == info["alive"] and info["sources"] == (2 if b == 2 else 1)
        late = heard[(state == ru.ALIVE)].max() - info["seed_tick"]
        assert 5 <= late <= 15, (b, late)
    assert _final(m, 3)[3]["sources"] == 0 and _final(m, 3)[3]["known"] == 0   # a crashed source
    assert m["trace"].longest <= 64
    j = _reference("full", "join")
    assert j["trace"].joinrep_carried > 100              # rumors ride the JOINREPs
    assert j["at"][20][3][3]["seed_tick"] == -1 and j["at"][20][3][3]["known"] == 0   # 599 not started
    assert _final(j, 3)[3]["seed_tick"] == 30 and _final(j, 3)[3]["sources"] == 1
    assert j["at"][20][1][3]["sources"] == 0             # 599 at tick 0: reaches nobody
    b = _reference("full", "burst")
    assert b["trace"].longest > 64, b["trace"].longest   # the wave-cooperative path
    assert b["trace"].joinrep_carried > 0
    v = _reference("full", "variants")
    assert _final(v, 0)[3]["known"] > 1


def test_partial_view_inputs_exercise_the_paths():
    a7, a2, a0 = (_reference("pview", k) for k in ("A7", "A2", "A0"))
    assert a7["trace"].longest > 64 and a7["trace"].cut_withheld > 0    # the cut matters
    assert a2["trace"].cut_withheld > a7["trace"].cut_withheld
    i = _final(a2, 0)[3]
    assert 0 < i["known_alive"] < i["alive"]             # live nodes left out at tick 40
    assert a0["trace"].cut_withheld == 0 and a0["trace"].longest > 64   # drain all, wave path
    assert _final(a0, 3)[3]["sources"] == 0
    j = _reference("pview", "join")
    assert j["trace"].longest > 64 and j["trace"].joinrep_carried > 0 and j["trace"].cut_withheld > 0
    i = _final(j, 1)[3]                                  # seeded at 250 at tick 6
    assert i["sources"] == 1 and 0 < i["known_alive"] < i["alive"]
    i = _final(j, 3)[3]                                  # the last joiner, at tick 30
    assert (i["seed_tick"], i["sources"], i["known"]) == (30, 1, 1)     # it never leaves that node
    assert j["at"][20][3][3]["sources"] == 0             # ... which had not started at tick 0


LAYOUTS = [dict(), dict(group=2), dict(group=3, layout="rows")]
LAYOUT_IDS = ["fused", "tiles2", "rows3"]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_full_view_rumor_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _reference("full", "main"))


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_full_view_rumor_join_schedule(layout):
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **layout,
                     **w["kw"]) as eng:
        _run(eng, w, _reference("full", "join"))


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2]], ids=["fused", "rows3"])
def test_full_view_rumor_join_burst(layout):
    w = FULL["burst"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **layout,
                     **w["kw"]) as eng:
        _run(eng, w, _reference("full", "burst"))


def test_full_view_rumor_tfail_swim():
    w = FULL["variants"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _reference("full", "variants"))


@pytest.mark.parametrize("name,group", [("A7", 1), ("A7", 3), ("A2", 1), ("A0", 1), ("B", 1)],
                         ids=["inbox7", "inbox7-rows3", "inbox2", "drain", "B-drain"])
def test_partial_view_rumor_matches_oracle(name, group):
    w = PVIEW[name]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, _reference("pview", name))


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_rumor_join_schedule(group):
    w = PVIEW["join"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, policy=make_policy(**w["pol"]),
                     **w["kw"]) as eng:
        _run(eng, w, _reference("pview", "join"))


def test_step_five_equals_five_steps():
    """step(5) between the listed ticks (all multiples of 5 here) gives the same trace."""
    w = dict(FULL["join"], at=(0, 5, 20, 35))
    ref = _reference("full", "join")
    assert all(t % 5 == 0 for t in ref["seeds"]) and all(t % 5 == 0 for t in ref["at"])
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        _run(eng, w, ref, chunk=5)


def test_thirty_two_rumors_are_independent():
    """Every bit of the word, each from its own source (the nodes alive at tick 5 are 0..119)."""
    w = FULL["join"]
    orc = _oracle("full", "join")
    seeds = {5: [(b, [3 * b + 1]) for b in range(32)]}
    ref = ru.run(orc, w["n"], w["ticks"], 0, 32, seeds, {5, 12, w["ticks"]})
    orc.close()
    heard = np.stack([s[0] for s in ref["at"][12]])
    assert len({h.tobytes() for h in heard}) == 32       # no two rumors travel alike
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        eng.rumor_open(32)
        for t in range(0, w["ticks"] + 1):
            if t:
                eng.step(1)
            for rumor, sources in seeds.get(t, ()):
                eng.rumor_seed(rumor, sources)
            if t in ref["at"]:
                for b in range(32):
                    _compare(eng.rumor(b), ref["at"][t][b], "tick %d rumor %d of 32" % (t, b))


def test_close_then_open_starts_empty():
    w = PVIEW["join"]
    ref = _reference("pview", "join")
    with PviewEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **w["kw"]) as eng:
        eng.rumor_open(2)
        with pytest.raises(GspError, match="already open"):
            eng.rumor_open(2)
        eng.rumor_seed(1, 0)
        eng.step(4)
        assert eng.rumor(1).info["known"] > 1
        eng.rumor_close()
        for call in (lambda: eng.rumor(0), lambda: eng.rumor_seed(0, 0), eng.rumor_close):
            with pytest.raises(GspError, match="no trace is open"):
                call()
        eng.step(2)                                      # untraced ticks
        eng.rumor_open(RUMORS)
        for b in range(RUMORS):
            r = eng.rumor(b)
            assert (r.heard == -1).all() and not r.known.any()
            assert (r.info["known"], r.info["seed_tick"], r.info["sources"], r.info["ticks_traced"],
                    r.info["tick"]) == (0, -1, 0, 0, 6)
        # the trace opened at tick 6 equals an oracle trace opened there
        orc = _oracle("pview", "join")
        tr = ru.Trace(w["n"], RUMORS, ref["start"], ref["fail"], w["kw"]["inbox"], opened_at=6)
        for t in range(1, 13):
            src, dst, joiners = orc.messages() + (orc.joinreps(),)
            orc.step()
            if t == 6:
                tr.seed(2, [0, 250])
                eng.rumor_seed(2, [0, 250])
            if t > 6:
                tr.tick(src, dst, joiners)
                eng.step(1)
        orc.close()
        _compare(eng.rumor(2), tr.snapshot(2), "reopened")
        for bad in (-1, RUMORS):
            with pytest.raises(GspError, match="rumor="):
                eng.rumor(bad)
        with pytest.raises(GspError):
            eng.rumor_seed(0, w["n"])
        for t in range(1, 13):
            assert eng.digest(t) == ref["digest"][t], t


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_untraced_engine_is_undisturbed(kind):
    """Two engines side by side, one with a trace: identical digests and rows."""
    w = (PVIEW if kind == "pview" else FULL)["join"]
    make = (lambda: PviewEngine(w["n"], max_ticks=20, policy=make_policy(**w["pol"]), **w["kw"])) \
        if kind == "pview" else \
        (lambda: ScaleEngine(w["n"], max_ticks=20, policy=make_policy(**w["pol"]), **w["kw"]))
    with make() as plain, make() as traced:
        traced.rumor_open(32)
        for b in range(32):
            traced.rumor_seed(b, [b, 0])
        for _ in range(4):
            plain.step(5)
            traced.step(5)
        assert traced.rumor(31).info["ticks_traced"] == 20
        for t in range(1, 21):
            assert plain.digest(t) == traced.digest(t), t
        for r in range(0, w["n"], 37):
            a, b = plain.row(r), traced.row(r)
            if kind == "pview":                          # (entries, length): the valid prefix
                assert a[1] == b[1], r
                a, b = a[0][:a[1]], b[0][:b[1]]
            assert np.array_equal(a, b), r


@pytest.mark.parametrize("bad", [0, 33])
def test_rumor_open_argument_errors(bad):
    with ScaleEngine(64, max_ticks=2) as eng:
        with pytest.raises(GspError, match="rumors="):
            eng.rumor_open(bad)
        eng.rumor_open(32)                               # the engine still answers
        eng.rumor_seed(31, 63)
        assert eng.rumor(31).info["known"] == 1
