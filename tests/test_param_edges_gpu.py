"""Both scale engines at the ends of their parameter ranges, bit for bit against the CPU oracle.

The workloads are tests/param_edges.py's: heartbeats up to 2047 (bit 15 of the packed entry
set), tremove 1, 2 and 31 with tfail = tremove - 1, fanout 16, drop_pct 100, swim 8, views of 1,
2 and 256 entries, inbox 0 and 1, n = 2 and 9, and census / reach age limits 1..32 on tremove =
31 workloads whose rows hold ages up to 30.  tests/test_param_edges_cpu.py proves from the
oracle's record that each workload reaches the edge it is named for.

Every comparison is against the oracle's record (ScaleOracle / PviewOracle: plain ints, absolute
timestamps), never the engine's own output: every tick's digest, at the check ticks the message
list and a sample of rows, at the last tick all rows (presence and hb exactly, ts mod 32).  The
scalar merge (set_merge(0)) and the packed v_pk_*_u16 merge must both equal the oracle at
hb = 2047, hb >= 2040 and tremove = 31: the check the comment on merge_word_packed
(csrc/scale_row.hpp) points to.
"""
import functools
import subprocess
import sys

import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import ScaleEngine
from tests import param_edges as pe
from tests.test_pview_gpu import _cmp_rows
from tests.test_scale_gpu import _compare_state

pytestmark = pytest.mark.gpu

LAYOUTS = {
    # name: (engine keywords, set_merge argument or None)
    "fused": (dict(), 1),
    "fused_scalar": (dict(), 0),
    "columns2": (dict(group=2), 1),
    "rows3": (dict(group=3, layout="rows"), 1),
}
FULL_RUNS = [(name, "fused") for name in pe.FULL] + \
    [(name, lay) for lay in ("columns2", "rows3") for name in ("hb_top", "tr31", "tr1")] + \
    [(name, "fused_scalar") for name in ("hb_2047", "hb_top", "hb_cross", "tr31", "tr1")]
PVIEW_RUNS = [(name, 1) for name in pe.PVIEW if name != "pv_census_big"] + \
    [("pv_hb_top", 3), ("pv_tr31_sw8", 3)]
INFO = ("tick", "n", "age_limit", "direction", "alive", "sources", "reached", "depth", "levels",
        "sum_hops")


def _messages(eng):
    m = eng.messages()
    s, f = np.nonzero(m >= 0)
    return sorted(zip(s.tolist(), m[s, f].tolist()))


def _events(eng, t):
    rec, lost = eng.drain_events()
    k, tk, r, x = _lib.split_events(rec)
    assert lost == 0 and np.all(tk == t), "events of tick %d: %d lost" % (t, lost)
    return sorted(zip(k.tolist(), r.tolist(), x.tolist()))


def _run_full(name, layout, events=False):
    ref = pe.reference(name)
    w, (lay, merge) = ref["w"], LAYOUTS[layout]
    n, ticks = w["n"], w["ticks"]
    with ScaleEngine(n, max_ticks=ticks, events=events, **lay, **w["kw"]) as eng:
        eng.set_merge(merge)
        assert _messages(eng) == ref["messages"][0], "messages of tick 0"
        if events:
            eng.drain_events()
        for t in range(1, ticks + 1):
            eng.step(1)
            got, want = eng.digest(t), ref["digest"][t]
            assert got == want, "tick %d digest\n got %s\nwant %s" % (t, got, want)
            if events:
                assert _events(eng, t) == ref["events"][t], "events tick %d" % t
            if t in ref["snap"]:
                assert _messages(eng) == ref["messages"][t], "messages tick %d" % t
                _compare_state(eng, ref["snap"][t], n, ref["sample"][t])     # every row at the end
        assert ref["sample"][ticks] == list(range(n))


@pytest.mark.parametrize("name,layout", FULL_RUNS, ids=["%s-%s" % c for c in FULL_RUNS])
def test_full_view_edge_matches_oracle(name, layout):
    _run_full(name, layout)


def test_full_view_tr31_event_stream_matches_oracle():
    """tremove = 31 with the event stream on: every tick's drained records are the oracle's
    joins and removes of that tick, none lost, across two wraps of the stored timestamp."""
    _run_full("tr31", "fused", events=True)


@pytest.mark.parametrize("name,group", PVIEW_RUNS, ids=["%s-g%d" % c for c in PVIEW_RUNS])
def test_partial_view_edge_matches_oracle(name, group):
    ref = pe.reference(name)
    w = ref["w"]
    n, ticks = w["n"], w["ticks"]
    with PviewEngine(n, max_ticks=ticks, group=group, **w["kw"]) as eng:
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
                got, want = eng.digest(t), ref["digest"][t]
                assert got == want, "tick %d digest\n got %s\nwant %s" % (t, got, want)
            eng._tick = t
            if t in ref["snap"]:
                assert _messages(eng) == ref["messages"][t], "messages tick %d" % t
                _cmp_rows(eng, ref["snap"][t], ref["sample"][t])             # every row at the end
        assert ref["sample"][ticks] == list(range(n))


def _census_and_reach(eng, ref):
    """Step one tick at a time to the last listed tick; there, census() at every age limit and
    reach(0) in both directions at every age limit against the record, a repeated call returning
    identical arrays; at the end every tick's digest still equals the oracle's."""
    w = ref["w"]
    kw, cen, n = w["kw"], w["census"], w["n"]
    last = max(cen["at"])
    for t in range(0, last + 1):
        if t:
            eng.step(1)
        if t not in cen["at"]:
            continue
        want = ref["census"][t]
        for l in cen["limits"]:
            got = eng.census() if l is None else eng.census(l)
            lim = pe.limit(l, kw)
            tag = "tick %d age_limit %d" % (t, lim)
            assert got.tick == t and got.info["age_limit"] == lim and got.info["n"] == n, tag
            assert np.array_equal(got.state, want["state"]), "state " + tag
            assert np.array_equal(got.listed, want["listed"]), "listed " + tag
            assert np.array_equal(got.fresh, want["fresh"][lim]), "fresh %s: %d differ" % (
                tag, int((got.fresh != want["fresh"][lim]).sum()))
            assert np.array_equal(got.max_hb, want["max_hb"]), "max_hb " + tag
            assert got.info["alive"] == int((want["state"] == pe.ALIVE).sum()), tag
            assert got.info["entries"] == int(want["listed"].sum(dtype=np.int64)), tag
            again = eng.census(lim)
            for f in ("state", "listed", "fresh", "max_hb"):
                assert np.array_equal(getattr(again, f), getattr(got, f)), "repeat %s %s" % (f, tag)
        if not cen["reach"]:
            continue
        for dname, d in pe.DIRS:
            for l in cen["limits"]:
                got = eng.reach(0, dname) if l is None else eng.reach(0, dname, l)
                lim = pe.limit(l, kw)
                tag = "tick %d %s age_limit %d" % (t, dname, lim)
                hops, info = ref["reach"][t][(lim, d)]
                assert got.hops.dtype == np.int32 and got.tick == t, tag
                assert np.array_equal(got.state, want["state"]), "state " + tag
                assert np.array_equal(got.hops, hops), "hops %s: %d differ" % (
                    tag, int((got.hops != hops).sum()))
                for f in INFO:
                    assert got.info[f] == info[f], "info.%s %s: %r != %r" % (f, tag, got.info[f], info[f])
                again = eng.reach(0, dname, lim)
                assert np.array_equal(again.hops, got.hops), "repeat hops " + tag
                assert np.array_equal(again.state, got.state), "repeat state " + tag
    for t in range(1, last + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the census" % t
    return got


@pytest.mark.parametrize("layout", ["fused", "columns2"])
def test_full_view_census_and_reach_at_age_limits(layout):
    """tr31 at ticks 20, 33 and 36: live rows hold ages 0..30, so the limits 16, 30, 31 and 32
    give different `fresh` (the packed age < limit compare at its last values, and 32 past the
    five bits)."""
    ref = pe.reference("tr31")
    w = ref["w"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **LAYOUTS[layout][0], **w["kw"]) as eng:
        _census_and_reach(eng, ref)


def test_partial_view_census_and_reach_at_age_limits():
    ref = pe.reference("pv_tr31_sw8")
    w = ref["w"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _census_and_reach(eng, ref)


@pytest.mark.parametrize("name", ["hb_2047", "hb_top", "drop100", "pv_hb_top"])
def test_census_at_the_heartbeat_and_drop_ends(name):
    """max_hb at 2047 / >= 2040 (the heartbeat field's top), and an all-alive population that
    lists nobody (drop_pct = 100 past tremove): listed, fresh and max_hb all zero."""
    ref = pe.reference(name)
    w = ref["w"]
    make = PviewEngine if ref["pview"] else ScaleEngine
    with make(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        got = _census_and_reach(eng, ref)
    if name == "drop100":
        assert (got.state == pe.ALIVE).all()
        assert not got.listed.any() and not got.fresh.any() and not got.max_hb.any()
    elif name == "hb_2047":
        senders = {s for s, _ in ref["messages"][0]}
        assert int((got.max_hb == 2047).sum()) == len(senders) and got.max_hb.max() == 2047
    else:
        assert int(got.max_hb.max()) >= 2040


@functools.lru_cache(maxsize=None)
def _compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a fresh child: this
    process has the engine's HIP runtime loaded, and torch cannot open the device next to it."""
    out = subprocess.run(
        [sys.executable, "-c", "import torch; "
         "print('CUS', torch.cuda.get_device_properties(0).multi_processor_count)"],
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return int([l for l in out.stdout.splitlines() if l.startswith("CUS")][-1].split()[1])


@pytest.mark.parametrize("form", ["0", "1"], ids=["plain", "lds"])
def test_partial_view_census_past_the_lds_cut(form, monkeypatch):
    """n = 4,608 > kCensusCut = 4,096 ids and rows x view slots beyond two passes of the
    privatised kernel's grid (2 x CUs workgroups of 1,024 lanes): its global-atomic branch for
    ids >= 4,096 and the second trip of its grid-stride loop.  Both forms equal the oracle."""
    ref = pe.reference("pv_census_big")
    w = ref["w"]
    cus = _compute_units()
    assert w["n"] > 4096 and w["n"] * w["kw"]["view"] > 2 * cus * 1024, cus
    assert ref["census"][6]["listed"][4096:].any()
    monkeypatch.setenv("GSP_TEST_PV_CENSUS", form)
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _census_and_reach(eng, ref)
