"""The membership census (gsp_scale_census / gsp_pview_census) against the CPU oracle.

The expected arrays are always numpy over the oracle's rows (ScaleOracle.row / PviewOracle.row)
of the rows alive at T -- fail_tick(r) >= T and start_tick(r) <= T -- never the engine's own
row().  Every oracle workload runs once per module; the cases that share it share its record.
The engine is stepped one tick at a time, the census taken at the listed ticks (each repeated
once: identical arrays), and at the end every tick's digest still equals the oracle's, so the
census disturbed nothing.

What the inputs exercise is asserted from the oracle's record itself: crashed members still
listed at one census and gone at a later one, stale entries in the crashed rows' own buffers (a
kernel that counted dead rows or read the other buffer would differ), fresh < listed, ticks past
the mod-32 wrap of the stored timestamp, rows shorter than the view, an empty live row, an
orphan and a hub.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd.census import ALIVE, CRASHED, NOT_STARTED
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

LIMITS = (3, 9, 32)

FULL = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes; T = 33, 40 lie past
    # the mod-32 wrap
    "main": dict(n=3000, ticks=40, at=(0, 1, 12, 13, 20, 33, 40), limits=LIMITS, pol=None,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): at T = 5 exactly the nodes >= 120 have not started
    "join": dict(n=600, ticks=35, at=(5, 20, 35), limits=LIMITS,
                 pol=dict(step_rate=0.05, intro_list=8),
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
    # TFAIL + SWIM change nothing in what is counted; age_limit defaults to tfail
    "variants": dict(n=1024, ticks=13, at=(12, 13), limits=(None,), pol=None,
                     kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                             fail_ppm=20000, seed=3003, tfail=4, swim=2)),
}

PVIEW = {
    "A": dict(n=4096, ticks=40, at=(0, 1, 12, 13, 25, 40), limits=LIMITS,
              kw=dict(view=32, fanout=3, inbox=7, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=4128)),
    "B": dict(n=1000, ticks=40, at=(12, 13, 40), limits=LIMITS,
              kw=dict(view=64, fanout=3, inbox=0, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2,
                      fail_ppm=50000, seed=1064)),
}


def _limit(lim, kw):
    return lim if lim is not None else (kw.get("tfail") or kw["tremove"])


def _states(orc, n, t):
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    start = np.array([orc.start_tick(r) for r in range(n)])
    return np.where(start > t, NOT_STARTED, np.where(fail >= t, ALIVE, CRASHED)).astype(np.uint8)


def _reduce(n, t, state, pres, hb, ts, limits, kw):
    """The census of tick t from the matrices [row][member] of the oracle's rows."""
    live = state == ALIVE
    p = pres & live[:, None]
    age = (t - ts) & 31
    out = {"state": state, "listed": p.sum(0).astype(np.uint32),
           "max_hb": np.where(p, hb, 0).max(0).astype(np.uint32),
           "fresh": {_limit(l, kw): (p & (age < _limit(l, kw))).sum(0).astype(np.uint32) for l in limits},
           # what the rows that are not alive still hold of crashed members
           "dead_entries": int(pres[~live][:, state == CRASHED].sum()),
           "lens": pres.sum(1), "live": live}
    return out


@functools.lru_cache(maxsize=None)
def _full_reference(name):
    w = FULL[name]
    n = w["n"]
    orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    ref = {"digest": [None], "census": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t in w["at"]:
            rows = [orc.row(r) for r in range(n)]
            pres = np.stack([x[0] for x in rows]).astype(bool)
            hb = np.stack([x[1] for x in rows])
            ts = np.stack([x[2] for x in rows])
            ref["census"][t] = _reduce(n, t, _states(orc, n, t), pres, hb, ts, w["limits"], w["kw"])
    orc.close()
    return ref


@functools.lru_cache(maxsize=None)
def _pview_reference(name):
    w = PVIEW[name]
    n = w["n"]
    orc = PviewOracle(n, **w["kw"])
    ref = {"digest": [None], "census": {}}
    for t in range(0, w["ticks"] + 1):
        if t:
            ref["digest"].append(orc.step())
        if t in w["at"]:
            state = _states(orc, n, t)
            live = state == ALIVE
            rows = [orc.row(r) for r in range(n)]
            ids, hb, ts = (np.concatenate([rows[r][k] for r in range(n) if live[r]]) for k in range(3))
            assert ((ids >= 0) & (ids < n)).all()
            age = (t - ts) & 31
            max_hb = np.zeros(n, np.uint32)
            np.maximum.at(max_hb, ids, hb.astype(np.uint32))
            ref["census"][t] = {
                "state": state, "live": live, "max_hb": max_hb,
                "listed": np.bincount(ids, minlength=n).astype(np.uint32),
                "fresh": {l: np.bincount(ids[age < l], minlength=n).astype(np.uint32) for l in w["limits"]},
                "lens": np.array([len(x[0]) for x in rows])}
    orc.close()
    return ref


def _undetected(c):
    return int(((c["state"] == CRASHED) & (c["listed"] > 0)).sum())


def _run(eng, w, ref):
    """Step to the end, census at the listed ticks, digests at the end."""
    n = w["n"]
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        want = ref["census"][t]
        for lim in w["limits"]:
            got = eng.census() if lim is None else eng.census(lim)
            lim = _limit(lim, w["kw"])
            tag = "tick %d age_limit %d" % (t, lim)
            assert got.tick == t and got.info["age_limit"] == lim and got.info["n"] == n, tag
            assert np.array_equal(got.state, want["state"]), "state " + tag
            assert np.array_equal(got.listed, want["listed"]), "listed " + tag
            assert np.array_equal(got.fresh, want["fresh"][lim]), "fresh " + tag
            assert np.array_equal(got.max_hb, want["max_hb"]), "max_hb " + tag
            assert got.info["alive"] == int((want["state"] == ALIVE).sum()), tag
            assert got.info["entries"] == int(want["listed"].sum(dtype=np.int64)), tag
            assert got.info["kernel_ms"] > 0, tag
        again = eng.census(lim)
        for f in ("state", "listed", "fresh", "max_hb"):
            assert np.array_equal(getattr(again, f), getattr(got, f)), "repeat %s %s" % (f, tag)
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the census" % t


def test_full_view_inputs_exercise_the_paths():
    c = _full_reference("main")["census"]
    crashed = int((c[40]["state"] == CRASHED).sum())
    assert crashed > 0 and _undetected(c[12]) > 0
    assert 0 < _undetected(c[20]) < crashed and _undetected(c[40]) == 0
    assert all(c[t]["dead_entries"] > 0 for t in (12, 13, 20, 33, 40))
    assert (c[12]["fresh"][3] < c[12]["listed"]).all()
    j = _full_reference("join")["census"]
    assert np.array_equal(np.nonzero(j[5]["state"] == NOT_STARTED)[0], np.arange(120, 600))
    assert (j[5]["listed"][120:] == 0).all() and (j[35]["state"] == CRASHED).any()


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_census_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, _full_reference("main"))


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_census_join_schedule(layout):
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **layout,
                     **w["kw"]) as eng:
        _run(eng, w, _full_reference("join"))


def test_full_view_census_tfail_swim_default_age_limit():
    w = FULL["variants"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _full_reference("variants"))
        assert eng.census().info["age_limit"] == 4


def test_census_age_limit_out_of_range():
    from gossip_protocol_amd._lib import GspError
    with ScaleEngine(64, max_ticks=2) as eng:
        for bad in (0, 33, -1):
            with pytest.raises(GspError, match="age_limit"):
                eng.census(bad)
    with PviewEngine(64, view=8, max_ticks=2) as eng:
        with pytest.raises(GspError, match="age_limit"):
            eng.census(0)


def test_partial_view_inputs_exercise_the_paths():
    a = _pview_reference("A")["census"]
    assert _undetected(a[12]) > 0 and _undetected(a[40]) == 0
    assert any((c["lens"][c["live"]] < 32).any() for c in a.values()), "no short row"
    assert int(a[40]["listed"].max()) > int((a[40]["state"] == ALIVE).sum()) / 4, "no hub"
    b = _pview_reference("B")["census"][40]
    assert ((b["state"] == ALIVE) & (b["listed"] == 0)).any(), "no live orphan"
    assert (b["lens"][b["live"]] == 0).any(), "no empty live row"


# form: GSP_TEST_PV_CENSUS, 0 the plain kernel, 1 the LDS-privatised one, None the default
@pytest.mark.parametrize("group,form", [(1, "0"), (1, "1"), (3, None), (3, "1")],
                         ids=["one_plain", "one_lds", "rows3", "rows3_lds"])
def test_partial_view_census_matches_oracle(group, form, monkeypatch):
    if form is not None:
        monkeypatch.setenv("GSP_TEST_PV_CENSUS", form)
    w = PVIEW["A"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, _pview_reference("A"))


@pytest.mark.parametrize("form", ["0", "1"], ids=["plain", "lds"])
def test_partial_view_census_drain_all(form, monkeypatch):
    monkeypatch.setenv("GSP_TEST_PV_CENSUS", form)
    w = PVIEW["B"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, _pview_reference("B"))
