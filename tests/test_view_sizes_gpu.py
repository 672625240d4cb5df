"""The partial-view engine at view sizes off the powers of two, bit for bit against the CPU oracle.

The workloads are tests/view_sizes.py's: drained views of 3 .. 255 slots (below 8: every long row
in the hub kernel with d_merge_runs; 8: Vp = V; 9, 17, 33, 65, 129: runs of Vp tuples that end in
padding; 192 / 193: the two sides of d_own's per = V > NT ? 2 : 1 in the 192-lane class), the same
sizes with a bounded inbox, join bursts that make node 0 a hub row at V = 7, 8, 9 and 193 (at 193
merged in chunks, the list carried between them), the protocol extensions, and 66,000 nodes
with ids on both sides of 65,536 in one 9-slot view.  tests/test_view_sizes_cpu.py proves from
the oracle's record that each workload reaches what it is named for.

Every comparison is against the oracle's record (PviewOracle: plain ints, absolute timestamps),
never the engine's own output: every tick's digest (no overflow when drained), at the check ticks
the sorted message list and sampled rows, at the last tick every row (length, ids, hb, ts mod 32,
the buffer's tail empty, own_hb of live rows), rows_run(t) == n without a join schedule, and
after a drained run the rows and messages of every drain class (drain_stats) against the
classes pv_drain_class gives the record's message counts.
"""
import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd.pview import PviewEngine
from tests import view_sizes as vs
from tests.test_param_edges_gpu import INFO, _events, _messages
from tests.test_pview_gpu import _cmp_rows

pytestmark = pytest.mark.gpu

DRAIN = vs.names("drain", vs.DRAIN_VIEWS)
BOUNDED = vs.names("bounded", vs.BOUNDED_VIEWS) + ["bounded_v9_k1_f16"]
BURST = vs.names("burst", vs.BURST_VIEWS)
EXT = vs.names("ext", vs.EXT_VIEWS)


def _force(monkeypatch, cls):
    """The row class a case is named for: (LDS bound, wide) as pv_drain_class takes them."""
    monkeypatch.setenv("GSP_TEST_PV_COUNT_ROWS", "1")
    if cls in ("c1", "c2", "c3"):
        monkeypatch.setenv("GSP_TEST_PV_DRAIN_WIDE", cls[1:])
        return vs.LDS_MAX, int(cls[1:])
    if cls == "hub":
        monkeypatch.setenv("GSP_TEST_PV_DRAIN_LDS", "300")
        return 300, 0
    return vs.LDS_MAX, 0


def _check_drain_stats(eng, ref, lds, wide):
    """drain_stats() per class == the record's long rows by pv_drain_class.  The receipt kernel
    lists every row sent more than 7 messages (gossip and a JOINREP), whether or not it is alive
    or has started -- the drain kernels count such a row as run and leave it alone -- so the
    record's rows count by k alone, not by state."""
    V = ref["kw"]["view"]
    want = vs.classes_reached(ref, lds, wide, live_only=False)
    got = eng.drain_stats()
    rows = [want.get(c, (0, 0))[0] for c in range(5)]
    msgs = [want.get(c, (0, 0))[1] for c in range(5)]
    assert got["rows"] == rows, "rows per class: got %s want %s" % (got["rows"], rows)
    assert got["messages"] == msgs, "messages per class: got %s want %s" % (got["messages"], msgs)
    live = vs.classes_reached(ref, lds, wide, live_only=True)
    assert sum(r for r, _ in live.values()) > 0, "no live long row"
    if V < 8:
        assert set(live) == {vs.HUB}
    elif lds < vs.LDS_MAX:
        assert vs.HUB in live and got["rows"][vs.HUB] > 0
    else:
        assert wide in live and got["rows"][wide] > 0, "class %d ran no live row" % wide


def _run(name, monkeypatch, cls="c0", group=1, events=False, evict_order=0, stats=True):
    ref = vs.reference(name, evict_order)
    w, kw = ref["w"], dict(ref["kw"])
    n, ticks, drained = w["n"], w["ticks"], ref["kw"]["inbox"] == 0
    lds, wide = _force(monkeypatch, cls)
    if w.get("policy"):
        kw["policy"] = _lib.make_policy(**w["policy"])
    with PviewEngine(n, max_ticks=ticks, group=group, events=events, **kw) as eng:
        if events:
            eng.drain_events()
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
                got, want = eng.digest(t), ref["digest"][t]
                assert got == want, "tick %d digest\n got %s\nwant %s" % (t, got, want)
                if drained:
                    assert got["overflow"] == 0
                if not w.get("policy"):
                    assert eng.rows_run(t) == n, "tick %d: %d rows run" % (t, eng.rows_run(t))
                if events:
                    assert _events(eng, t) == ref["events"][t], "events tick %d" % t
            eng._tick = t
            if t in ref["snap"]:
                assert _messages(eng) == ref["messages"][t], "messages tick %d" % t
                _cmp_rows(eng, ref["snap"][t], ref["sample"][t])
        if "sample_step" not in w:
            assert ref["sample"][ticks] == list(range(n))             # every row at the end
        if drained and stats:
            _check_drain_stats(eng, ref, lds, wide)


SIZED = DRAIN + BOUNDED + BURST + EXT + ["ids64k_v9"]


@pytest.mark.parametrize("name", SIZED)
def test_view_size_matches_oracle(name, monkeypatch):
    """Every workload as sized, one shard."""
    _run(name, monkeypatch)


FORCED = [("drain_v%d" % V, cls) for V in (8, 9, 33, 193) for cls in ("c1", "c2", "c3")] + \
    [("drain_v33", "hub"), ("drain_v193", "hub")]


@pytest.mark.parametrize("name,cls", FORCED, ids=["%s-%s" % c for c in FORCED])
def test_drain_sweep_in_forced_classes(name, cls, monkeypatch):
    """The 256-, 512- and 1024-lane LDS classes (E = 16 tuples per lane over runs of Vp = 8, 16,
    64 and 256) and the hub kernel's windowed merge.  At V = 8 and 9 a row's need stays under
    the 258-tuple floor of GSP_TEST_PV_DRAIN_LDS unless k is about 27 or more: the join bursts
    are the hub cases of those two views."""
    _run(name, monkeypatch, cls=cls)


EVENTS = [(name, e) for name in vs.names("drain", vs.EVENT_VIEWS) + EXT for e in (0, 1)]


@pytest.mark.parametrize("name,evict_order", EVENTS, ids=["%s-e%d" % c for c in EVENTS])
def test_view_size_event_stream(name, evict_order, monkeypatch):
    """Events on, both eviction orders: every tick's drained join / remove / evict records are
    the oracle's, none lost."""
    _run(name, monkeypatch, events=True, evict_order=evict_order)


SHARDS = vs.names("drain", (7, 9, 193)) + ["bounded_v9", "bounded_v255", "ext_v9", "ids64k_v9"]


@pytest.mark.parametrize("name", SHARDS)
def test_view_size_row_shards(name, monkeypatch):
    """Three row shards in one process: the senders' views cross as packed wire rows of
    (4V + 73) / 8 words, an odd V among them, and at 66,000 nodes with two non-empty id groups."""
    _run(name, monkeypatch, group=3)


ONE_KERNEL = ["drain_v9", "drain_v193", "bounded_v9", "bounded_v193"]


@pytest.mark.parametrize("name", ONE_KERNEL)
def test_view_size_one_kernel_form(name, monkeypatch):
    """GSP_TEST_PV_SPLIT=0: every short row in the one 256-lane tick kernel (the engine keeps no
    class sizes on the host in this form, so drain_stats is not read)."""
    monkeypatch.setenv("GSP_TEST_PV_SPLIT", "0")
    _run(name, monkeypatch, stats=False)


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("V", vs.CENSUS_VIEWS)
def test_view_size_census_and_reach(V, group):
    """census() at the default age limit and 32 and reach(0) in both directions at the last tick
    (the table indexed as i / view and row * view + s at V = 7 and 193) against the record; every
    earlier digest is unchanged afterwards."""
    ref = vs.reference("drain_v%d" % V)
    w, kw = ref["w"], ref["kw"]
    n, t = w["n"], w["ticks"]
    want = ref["census"][t]
    with PviewEngine(n, max_ticks=t, group=group, **kw) as eng:
        eng.step(t)
        for l in vs.CENSUS_LIMITS:
            got = eng.census() if l is None else eng.census(l)
            lim = vs.pe.limit(l, kw)
            tag = "age_limit %d" % lim
            assert got.tick == t and got.info["age_limit"] == lim and got.info["n"] == n, tag
            assert np.array_equal(got.state, want["state"]), "state " + tag
            assert np.array_equal(got.listed, want["listed"]), "listed " + tag
            assert np.array_equal(got.fresh, want["fresh"][lim]), "fresh " + tag
            assert np.array_equal(got.max_hb, want["max_hb"]), "max_hb " + tag
            assert got.info["alive"] == int((want["state"] == vs.pe.ALIVE).sum()), tag
            assert got.info["entries"] == int(want["listed"].sum(dtype=np.int64)), tag
        for dname, d in vs.pe.DIRS:
            for l in vs.CENSUS_LIMITS:
                got = eng.reach(0, dname) if l is None else eng.reach(0, dname, l)
                lim = vs.pe.limit(l, kw)
                tag = "%s age_limit %d" % (dname, lim)
                hops, info = ref["reach"][t][(lim, d)]
                assert np.array_equal(got.state, want["state"]), "state " + tag
                assert np.array_equal(got.hops, hops), "hops %s: %d differ" % (
                    tag, int((got.hops != hops).sum()))
                for f in INFO:
                    assert got.info[f] == info[f], "info.%s %s: %r != %r" % (f, tag, got.info[f], info[f])
        for tt in range(1, t + 1):
            assert eng.digest(tt) == ref["digest"][tt], "digest of tick %d after the census" % tt
