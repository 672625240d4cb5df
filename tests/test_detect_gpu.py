"""Detection ledger (gsp_scale_detect_* / gsp_pview_detect_*) against the numpy rule over the CPU
oracle.

The expected arrays come from tests/detect_oracle.py, which reads only the oracle's events(),
start_tick() and fail_tick() -- never engine output.  Every oracle workload (the rumor tests'
FULL / PVIEW entries) runs once per module; the cases that share one share its record.  A ledger
is opened at tick 0, the engine is stepped one tick at a time, and at the listed ticks every array,
by_tick, state and every info field but kernel_ms (> 0) is compared; a repeated get is identical,
lost is 0 (the ring's stripes hold a tick), and at the end every tick's digest equals the
oracle's.  Both forms of the fold (plain global atomics, LDS-aggregated) run the same cases.

What the inputs reach is asserted from the oracle's own record: true removes, false removes,
revivals, evictions (partial view), and a member removed, revived and removed again.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, make_policy
from tests import detect_oracle as do
from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

pytestmark = pytest.mark.gpu

CAP = 1 << 20                    # a stripe (1/256) holds any tick of these workloads
FULL = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes
    "main": dict(n=3000, ticks=40, at=(0, 1, 12, 25, 40), pol=None, cap=CAP,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): 599 starts at tick 29
    "join": dict(n=600, ticks=35, at=(0, 5, 20, 35), pol=dict(step_rate=0.05, intro_list=8), cap=CAP,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
    # TFAIL + SWIM
    "variants": dict(n=1024, ticks=25, at=(6, 13, 25), pol=None, cap=CAP,
                     kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                             seed=3003, tfail=4, swim=2)),
}
_A = dict(view=32, fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=50000, seed=4128)
PVIEW = {
    "A7": dict(n=4096, ticks=40, at=(0, 1, 12, 25, 40), pol=None, cap=1 << 22, kw=dict(inbox=7, **_A)),
    "A0": dict(n=4096, ticks=40, at=(12, 40), pol=None, cap=1 << 22, kw=dict(inbox=0, **_A)),
    # node i starts at int(0.02 i): the last joiner 1199 at tick 23
    "join": dict(n=1200, ticks=40, at=(6, 20, 30, 40), pol=dict(step_rate=0.02, intro_list=8), cap=CAP,
                 kw=dict(view=32, fanout=3, inbox=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10,
                         fail_ppm=30000, seed=77)),
}


def _workload(kind, name):
    return (PVIEW if kind == "pview" else FULL)[name]


def _oracle(kind, name):
    w = _workload(kind, name)
    pol = oracle_policy(**w["pol"]) if w["pol"] else None
    return (PviewOracle if kind == "pview" else ScaleOracle)(w["n"], policy=pol, **w["kw"])


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    w = _workload(kind, name)
    orc = _oracle(kind, name)
    ref = do.run(orc, w["n"], w["ticks"], set(w["at"]) | set(range(0, w["ticks"] + 1, 5)),
                 keep_r=w["n"] < 4096)               # r: only where drained records are compared
    orc.close()
    return ref


def _engine(kind, name, events=True, cap=None, max_ticks=None, **layout):
    w = _workload(kind, name)
    pol = dict(policy=make_policy(**w["pol"])) if w["pol"] else {}
    cls = PviewEngine if kind == "pview" else ScaleEngine
    return cls(w["n"], max_ticks=max_ticks or w["ticks"], events=events, event_cap=cap or w["cap"],
               **pol, **layout, **w["kw"])


def _compare(got, want, tag, info=do.INFO):
    assert got.tick == want["info"]["tick"], tag
    for a in do.ARRAYS:
        g, e = getattr(got, a), want[a]
        assert g.dtype == e.dtype, (tag, a, g.dtype)
        assert np.array_equal(g, e), "%s %s: %d differ, first at %s" % (
            a, tag, int((g != e).sum()), np.nonzero(g != e)[0][:5].tolist())
    assert np.array_equal(got.state, want["state"]), "state " + tag
    assert got.by_tick.dtype == np.uint64 and got.by_tick.shape == want["by_tick"].shape, tag
    assert np.array_equal(got.by_tick, want["by_tick"]), "by_tick %s: ticks %s" % (
        tag, np.nonzero((got.by_tick != want["by_tick"]).any(axis=1))[0][:5].tolist())
    for f in info:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in do.ARRAYS + ("state", "by_tick")) \
        and {f: a.info[f] for f in do.INFO} == {f: b.info[f] for f in do.INFO}


def _run(eng, w, ref, chunk=1, at=None):
    """Open at tick 0, compare at the listed ticks, digests at the end."""
    eng.detect_open()
    for t in range(0, w["ticks"] + 1, chunk):
        if t:
            eng.step(chunk)
        if t not in (at or w["at"]):
            continue
        got = eng.detect()
        _compare(got, ref["at"][t], "tick %d" % t)
        assert got.info["lost"] == 0
        if t:
            assert got.info["kernel_ms"] > 0, t
        assert _same(eng.detect(), got), "a repeated get at tick %d" % t
    rec, lost = eng.drain_events()                       # the folds emptied the ring
    assert len(rec) == 0 and lost == 0
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d with a ledger open" % t


def _classes(ref, ticks):
    """From the oracle's record alone: the ledger's totals, and the members with a revival
    strictly between their first and their last true remove."""
    s = ref["ledger"].snapshot(ticks)
    again = np.zeros(len(ref["crash"]), bool)
    for t in range(1, ticks + 1):
        k, _, x = ref["events"][t]
        rv = x[(k == do.JOIN) & (t > ref["crash"][x])]
        again[rv[(s["first_remove"][rv] >= 0) & (s["first_remove"][rv] < t) & (t < s["last_remove"][rv])]] = True
    return s["info"], int(again.sum())


def test_full_view_inputs_reach_every_class():
    for name in FULL:
        info, again = _classes(_reference("full", name), FULL[name]["ticks"])
        assert info["true_removes"] > 0 and info["false_removes"] > 0 and info["revivals"] > 0, (name, info)
        assert info["evicts"] == 0
        assert again > 0, name                           # removed, revived and removed again


def test_partial_view_inputs_reach_every_class():
    for name in PVIEW:
        info, again = _classes(_reference("pview", name), PVIEW[name]["ticks"])
        assert info["true_removes"] > 0 and info["false_removes"] > 0 and info["revivals"] > 0, (name, info)
        assert info["evicts"] > 0, name
    assert _classes(_reference("pview", "join"), 40)[1] > 0      # removed, revived, removed again


LAYOUTS = [dict(), dict(group=2), dict(group=3, layout="rows")]
LAYOUT_IDS = ["fused", "tiles2", "rows3"]
FORMS = ["0", "1"]
FORM_IDS = ["plain", "lds"]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_full_view_detect_matches_oracle(layout, form, monkeypatch):
    monkeypatch.setenv("GSP_TEST_DETECT_FORM", form)
    with _engine("full", "main", **layout) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, FULL["main"], _reference("full", "main"))


@pytest.mark.parametrize("name,layout", [("join", 0), ("join", 2), ("variants", 0)],
                         ids=["join-fused", "join-rows3", "variants"])
def test_full_view_detect_join_and_variants(name, layout):
    with _engine("full", name, **LAYOUTS[layout]) as eng:
        _run(eng, FULL[name], _reference("full", name))


@pytest.mark.parametrize("name,group,form", [("A7", 1, "1"), ("A7", 1, "0"), ("A7", 3, "1"), ("A0", 1, "1"),
                                             ("join", 1, "1"), ("join", 1, "0")],
                         ids=["inbox7", "inbox7-plain", "inbox7-rows3", "drain", "join", "join-plain"])
def test_partial_view_detect_matches_oracle(name, group, form, monkeypatch):
    monkeypatch.setenv("GSP_TEST_DETECT_FORM", form)
    with _engine("pview", name, group=group) as eng:
        _run(eng, PVIEW[name], _reference("pview", name))


def test_step_five_equals_five_steps():
    ref = _reference("full", "main")
    with _engine("full", "main") as eng:
        _run(eng, FULL["main"], ref, chunk=5, at=(0, 5, 25, 40))


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_open_mid_run_covers_the_records_since_the_last_drain(kind):
    """Opened undrained at tick 5 the ledger equals the oracle's ticks 1..T; opened right after a
    drain at tick 12 it equals the ticks 13..T."""
    w = _workload(kind, "join")
    ref = _reference(kind, "join")
    T = 20
    with _engine(kind, "join") as eng:
        eng.step(5)
        eng.detect_open()
        want = do.ledger_over(ref, w["n"], w["ticks"], 1, 5)
        want.opened_at = 5
        _compare(eng.detect(), want.snapshot(5), "opened at 5")
        for t in range(6, T + 1):
            eng.step(1)
            k, _, x = ref["events"][t]
            want.fold(k, t, x)
        _compare(eng.detect(), want.snapshot(T), "opened at 5, tick %d" % T)
    with _engine(kind, "join") as eng:
        eng.step(12)
        rec, lost = eng.drain_events()
        assert len(rec) == sum(len(ref["events"][t][0]) for t in range(1, 13)) and lost == 0
        eng.detect_open()
        eng.step(T - 12)
        want = do.ledger_over(ref, w["n"], w["ticks"], 13, T)
        want.opened_at = 12
        got = eng.detect()
        _compare(got, want.snapshot(T), "opened after a drain at 12")
        assert not got.by_tick[:13].any()


def _sorted_records(ref, lo, hi):
    return np.sort(np.concatenate([do.pack(ref["events"][t][0], t, ref["events"][t][1], ref["events"][t][2])
                                   for t in range(lo, hi + 1)]))


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_close_then_reopen_starts_empty(kind):
    w = _workload(kind, "join")
    ref = _reference(kind, "join")
    with _engine(kind, "join") as eng:
        eng.detect_open()
        with pytest.raises(GspError, match="already open"):
            eng.detect_open()
        eng.step(10)
        assert eng.detect().info["records"] == sum(len(ref["events"][t][0]) for t in range(1, 11))
        eng.detect_close()
        for call in (eng.detect, eng.detect_close):
            with pytest.raises(GspError, match="no ledger is open"):
                call()
        eng.step(4)                                      # the ring fills and drains as before
        rec, lost = eng.drain_events()
        assert lost == 0 and np.array_equal(np.sort(rec), _sorted_records(ref, 11, 14))
        eng.step(2)                                      # ticks 15, 16: in the ring at the reopen
        eng.detect_open()
        want = do.ledger_over(ref, w["n"], w["ticks"], 15, 16)
        want.opened_at = 16
        _compare(eng.detect(), want.snapshot(16), "reopened at 16")
        eng.step(4)
        for t in range(17, 21):
            want.fold(ref["events"][t][0], t, ref["events"][t][2])
        _compare(eng.detect(), want.snapshot(20), "reopened, tick 20")
        eng.detect_close()
        eng.detect_open()                                # an empty ring: an empty ledger
        got = eng.detect()
        assert got.info["records"] == 0 and not got.by_tick.any()
        assert (got.first_remove == -1).all() and (got.last_remove == -1).all() and (got.first_false == -1).all()
        assert not (got.removers.any() or got.false_removes.any() or got.revivals.any() or got.evicts.any())
        for t in range(1, 21):
            assert eng.digest(t) == ref["digest"][t], t


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_ring_too_small_counts_lost(form, monkeypatch):
    """event_cap = 4096: 16 records per stripe.  What a full stripe refuses within a tick is lost,
    records + lost is every record made, and what was folded is a subset of the oracle's."""
    monkeypatch.setenv("GSP_TEST_DETECT_FORM", form)
    w, ref = FULL["main"], _reference("full", "main")
    want = ref["at"][40]
    with _engine("full", "main", cap=4096) as eng:
        eng.detect_open()
        for _ in range(w["ticks"]):
            eng.step(1)
        got = eng.detect()
    assert got.info["lost"] > 0
    assert got.info["records"] + got.info["lost"] == want["info"]["records"]
    for a in ("removers", "false_removes", "revivals", "evicts"):
        assert (getattr(got, a) <= want[a]).all(), a
    big = np.iinfo(np.int32).max
    for a in ("first_remove", "first_false"):
        g, e = getattr(got, a), want[a]
        assert (np.where(g < 0, big, g) >= np.where(e < 0, big, e)).all(), a
    assert (got.last_remove <= want["last_remove"]).all()
    assert (got.by_tick <= want["by_tick"]).all()
    for f in ("true_removes", "false_removes", "joins", "revivals"):
        assert got.info[f] <= want["info"][f], f


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_summary_equals_the_host_drained_summary(kind):
    """Detect.summary()'s shared fields against bench.event_summary of a twin engine that never
    opens a ledger and drains once at the end."""
    import bench
    name = "main" if kind == "full" else "join"
    w = _workload(kind, name)
    with _engine(kind, name) as eng, _engine(kind, name, cap=1 << 23) as twin:
        eng.detect_open()
        eng.step(w["ticks"])
        twin.step(w["ticks"])
        got = eng.detect()
        host = bench.event_summary(twin, w["n"], w["ticks"], None, got.crash)
    assert host["lost"] == 0 and host["crashed_nodes_detected"] > 0
    s = got.summary()
    for f in ("crashed_nodes", "crashed_nodes_detected", "removes_per_detected_node", "removes_of_live_nodes",
              "first_detection_latency_ticks", "full_detection_latency_ticks", "lost"):
        assert s[f] == host[f], (f, s[f], host[f])
    assert got.info["records"] == host["records"] and got.info["joins"] == host["joins"]
    assert got.info["true_removes"] + got.info["false_removes"] == host["removes"]
    ref = _reference(kind, name)["at"][w["ticks"]]
    assert s["revivals"] == ref["info"]["revivals"] and s["revived_nodes"] == int((ref["revivals"] > 0).sum())
    assert s["falsely_removed_nodes"] == int((ref["false_removes"] > 0).sum())


def test_detect_argument_errors():
    with ScaleEngine(64, max_ticks=2) as eng:            # events off
        with pytest.raises(GspError, match="events"):
            eng.detect_open()
        for call in (eng.detect, eng.detect_close):
            with pytest.raises(GspError, match="no ledger is open"):
                call()
    with PviewEngine(256, view=32, max_ticks=2, events=_lib.EVENTS_JOIN | _lib.EVENTS_EVICT) as eng:
        with pytest.raises(GspError, match="gsp_pview_detect_open.*events"):
            eng.detect_open()
    with ScaleEngine(64, max_ticks=2, events=_lib.EVENTS_REMOVE) as eng:     # joins count 0
        eng.detect_open()
        with pytest.raises(GspError, match="already open"):
            eng.detect_open()
        eng.step(2)
        got = eng.detect()
        assert got.info["kinds"] == _lib.EVENTS_REMOVE and got.info["joins"] == 0
        assert got.info["ticks_folded"] == 2 and got.info["open_tick"] == 0


def test_removes_only_engine_counts_no_joins():
    """Kinds the engine does not record count 0: the oracle's ledger over the remove records."""
    w, ref = FULL["join"], _reference("full", "join")
    pol = make_policy(**w["pol"])
    with ScaleEngine(w["n"], max_ticks=w["ticks"], events=_lib.EVENTS_REMOVE, event_cap=CAP, policy=pol,
                     **w["kw"]) as eng:
        eng.detect_open()
        eng.step(w["ticks"])
        want = do.ledger_over(ref, w["n"], w["ticks"], 1, w["ticks"], kinds=_lib.EVENTS_REMOVE)
        _compare(eng.detect(), want.snapshot(w["ticks"]), "removes only")
