"""The view-size workloads (tests/view_sizes.py) reach what they are named for.

Everything here is read from the CPU oracle's record alone, so it runs without a GPU: if a
workload stopped filling its views, stopped making long rows or hubs, or no longer put ids on
both sides of 65,536 into one view (another seed, a changed rule), the GPU comparison in
tests/test_view_sizes_gpu.py would still pass and prove nothing -- these fail instead.
"""
import numpy as np
import pytest

from tests import view_sizes as vs

DRAIN = vs.names("drain", vs.DRAIN_VIEWS)
BOUNDED = vs.names("bounded", vs.BOUNDED_VIEWS) + ["bounded_v9_k1_f16"]
BURST = vs.names("burst", vs.BURST_VIEWS)
EXT = vs.names("ext", vs.EXT_VIEWS)
# the oracle runs the GPU module makes: every workload, and eviction order 1 where events are kept
RUNS = [(name, 0) for name in sorted(vs.WORKLOADS)] + \
    [(name, 1) for name in sorted(vs.WORKLOADS) if vs.WORKLOADS[name].get("events")]


def _live_long_k(ref):
    ticks = ref["w"]["ticks"]
    return np.concatenate([vs.long_rows(ref, t, live_only=True)[1] for t in range(1, ticks + 1)])


@pytest.mark.parametrize("name,evict_order", RUNS, ids=["%s-e%d" % c for c in RUNS])
def test_oracle_run_stays_short(name, evict_order):
    """The GPU module re-runs every oracle workload: each stays under 5 s of oracle steps."""
    ref = vs.reference(name, evict_order)
    print("%s: %.2f s in %d oracle steps" % (name, ref["seconds"], ref["w"]["ticks"]))
    assert len(ref["digest"]) == ref["w"]["ticks"] + 1
    assert ref["seconds"] < 5.0, "%s: %.2f s" % (name, ref["seconds"])


def test_the_table_walks_the_view_sizes():
    """The sizes the kernels branch on: below 8, 8, one past a power of two, 192 / 193, 255."""
    drained = {w["kw"]["view"] for w in vs.WORKLOADS.values() if w["kw"]["inbox"] == 0}
    bounded = {w["kw"]["view"] for w in vs.WORKLOADS.values() if w["kw"]["inbox"] > 0}
    assert {3, 7, 8, 9, 17, 33, 65, 129, 192, 193, 255} <= drained
    assert {3, 7, 9, 33, 65, 129, 193, 255} <= bounded
    for w in vs.WORKLOADS.values():
        assert w["kw"]["tremove"] == 6 and w["kw"]["drop_pct"] == 10 and w["kw"]["fail_tick"] == 4
    assert len({w["kw"]["seed"] for w in vs.WORKLOADS.values()}) == len(vs.WORKLOADS)


@pytest.mark.parametrize("name", DRAIN + BOUNDED)
def test_sweep_fills_its_views_and_evicts(name):
    """Evictions happen (the cut down to V runs), and at the last tick more than half of the
    views hold exactly V entries (a list of V ids, with Vp - V padding tuples behind it).  The
    inbox-1 case merges one message a tick against tremove = 6: its views reach V (96 of 1,500
    when it was written) but most stay shorter, so it is held to "some", not "half"."""
    ref = vs.reference(name)
    w = ref["w"]
    V, n, t = w["kw"]["view"], w["n"], w["ticks"]
    lens = np.array([len(ref["snap"][t].row(r)[0]) for r in range(n)])
    full = int((lens == V).sum())
    print("%s: evicts %d, %d of %d views full, longest %d" % (name, vs.total(ref, "evicts"), full, n,
                                                              lens.max()))
    assert vs.total(ref, "evicts") > 0 and vs.total(ref, "joins") > 0
    assert lens.max() == V and full > 0
    if w["kw"]["inbox"] != 1:
        assert 2 * full > n
    assert (ref["fail"] < t).any() and (ref["fail"] >= t).any()       # the failures of tick 4


@pytest.mark.parametrize("name", DRAIN + BURST + EXT)
def test_drain_workloads_have_long_rows(name):
    """Live receivers sent more than 7 messages exist (the rows of the drain kernels): thousands
    in the drain sweep from V = 7 on and hundreds in the extension workloads; at V = 3 views are
    too small for many (18 over 14 ticks when the workload was written), and a join burst has
    its hub and a few dozen others."""
    ref = vs.reference(name)
    k = _live_long_k(ref)
    print("%s: %d live long rows, longest k = %d" % (name, k.size, k.max() if k.size else 0))
    assert all(d["overflow"] == 0 for d in ref["digest"][1:])
    few = ref["w"]["kw"]["view"] == 3 or name in BURST
    assert k.size > (0 if few else 100)


def test_bounded_workloads_overflow():
    for name in BOUNDED:
        ref = vs.reference(name)
        inbox = ref["w"]["kw"]["inbox"]
        over = sum(int((ref["k"][t][ref["live"][t]] > inbox).sum()) for t in range(1, ref["w"]["ticks"] + 1))
        assert over > 0 and vs.total(ref, "overflow") > 0, name
    k1 = vs.reference("bounded_v9_k1_f16")
    assert k1["w"]["kw"]["inbox"] == 1 and k1["w"]["kw"]["fanout"] == 16
    assert vs.total(k1, "overflow") > 10 * k1["w"]["n"]


def test_pv_drain_need_restated():
    """pv_drain_need: vp (1 + k) + ceil(k / vp) vp with vp = pow2(view)."""
    assert vs.drain_need(8, 256) == 256 * 9 + 256 and vs.drain_need(8, 193) == vs.drain_need(8, 256)
    assert vs.drain_need(8, 9) == 16 * 9 + 16 and vs.drain_need(8, 8) == 8 * 9 + 8
    assert vs.drain_need(8, 3) == 4 * 9 + 8 and vs.drain_need(44, 33) == 64 * 45 + 64
    assert vs.drain_need(1, 1) == 3
    assert vs.drain_class(8, 7) == vs.HUB and vs.drain_class(8, 8) == 0 and vs.drain_class(65, 9) == vs.HUB
    assert vs.drain_class(10, 256) == 0 and vs.drain_class(11, 256) == 1 and vs.drain_class(62, 256) == 3
    assert vs.drain_class(63, 256) == vs.HUB and vs.drain_class(8, 33, lds=300) == vs.HUB
    assert [vs.drain_class(8, 9, wide=w) for w in (1, 2, 3)] == [1, 2, 3]


def test_drain_classes_reached_unforced():
    """Which row classes each drain-sweep workload reaches as sized (from the record's k): below 8
    slots only the hub kernel; V = 8 and 9 stay in class 0 (k <= 64 needs at most 1,104 tuples);
    V = 65 and 129 reach class 3.  At V = 33 no k can: k <= kDrainStage = 64 bounds the need by
    4,224 tuples, so its largest receivers (k > 64) are hub rows, the hub kernel unforced at a
    view past 8."""
    reached = {}
    for V in vs.DRAIN_VIEWS:
        ref = vs.reference("drain_v%d" % V)
        reached[V] = vs.classes_reached(ref)
        k = _live_long_k(ref)
        print("V = %d: classes %s, largest need %d" % (V, reached[V], vs.drain_need(int(k.max()), V)))
    assert set(reached[3]) == {vs.HUB} and set(reached[7]) == {vs.HUB}
    assert set(reached[8]) == {0} and set(reached[9]) == {0}
    assert max(vs.drain_need(k, 9) for k in range(8, 65)) == 1104
    assert all(vs.drain_class(k, 33) < 3 for k in range(8, 65))
    assert {0, 1, 2, vs.HUB} <= set(reached[33])
    assert _live_long_k(vs.reference("drain_v33")).max() > vs.STAGE
    for V in (65, 129):
        assert {0, 1, 2, 3} <= set(reached[V]), V
    for V in (17, 192, 193, 255):
        assert 0 in reached[V], V
    # the forced cases of the GPU module: the class they are named for gets rows
    for V in (8, 9, 33, 193):
        ref = vs.reference("drain_v%d" % V)
        for wide in (1, 2, 3):
            assert wide in vs.classes_reached(ref, wide=wide), (V, wide)
            assert not any(c < wide for c in vs.classes_reached(ref, wide=wide)), (V, wide)
    for V in (33, 193):
        assert set(vs.classes_reached(vs.reference("drain_v%d" % V), lds=300)) == {vs.HUB}
    # V = 8 / 9: a row's need stays under the 258-tuple floor of the LDS bound unless k >= ~27
    assert vs.drain_need(26, 8) <= 258 < vs.drain_need(29, 8) and vs.drain_need(13, 9) <= 258


@pytest.mark.parametrize("name", BURST)
def test_join_burst_makes_node_0_a_hub(name):
    """Every node starts by tick 1 knowing only node 0, so node 0 is sent more than kDrainStage =
    64 messages in one tick: a hub row at every V.  At V = 193 its tuples pass the 8,192-tuple
    HBM buffers of this n, so it merges in chunks with the list carried between them."""
    ref = vs.reference(name)
    w = ref["w"]
    V, n = w["kw"]["view"], w["n"]
    assert ref["start"].max() == 1 and (ref["start"] == 0).any()
    k0 = max(int(ref["k"][t][0]) for t in range(1, w["ticks"] + 1) if ref["live"][t][0])
    print("%s: node 0 is sent %d messages, need %d" % (name, k0, vs.drain_need(k0, V)))
    assert k0 > vs.STAGE and vs.drain_class(k0, V) == vs.HUB
    assert n + 3 * 256 <= 8192                                        # the buffers: 8,192 tuples
    if V == 193:
        assert vs.drain_need(k0, V) > 8192
    assert vs.total(ref, "evicts") > 0


@pytest.mark.parametrize("name", EXT)
def test_extension_workloads_join_remove_and_evict(name):
    ref = vs.reference(name)
    w = ref["w"]
    assert w["kw"]["tfail"] == 3 and w["kw"]["swim"] == 2 and w["policy"]["intro_list"] == 4
    assert vs.total(ref, "joins") > 0 and vs.total(ref, "removes") > 0 and vs.total(ref, "evicts") > 0
    assert ref["joinreps"] > 0, "no JOINREP is delivered"
    kinds = {k for ev in ref["events"][1:] for k, _, _ in ev}
    assert kinds == {1, 2, 3}
    for t in range(1, w["ticks"] + 1):
        d = ref["digest"][t]
        assert len(ref["events"][t]) == d["joins"] + d["removes"] + d["evicts"], t
    assert ref["start"].max() > 4                                     # nodes start across the run
    # a long row that takes a JOINREP with its introducer list exists or not, the list is used
    assert vs.reference(name, 1)["digest"] != ref["digest"]           # the eviction order matters


def test_ids_on_both_sides_of_65536():
    """n = 66,000, V = 9: at tick 4 and at the end some of the every-50th sampled views hold ids
    below and at or above 65,536 (two non-empty groups of the packed wire row)."""
    ref = vs.reference("ids64k_v9")
    n = ref["w"]["n"]
    assert n > vs.SPLIT and sorted(ref["snap"]) == [4, 6]
    for t in (4, 6):
        print("tick %d: %d of %d sampled views straddle 65,536" % (
            t, len(ref["straddle"][t]), len(range(0, n, 50))))
        assert len(ref["straddle"][t]) > 0
        got = [r for r in ref["sample"][t] if vs.straddles(ref["snap"][t].row(r)[0])]
        assert len(got) >= 60
    assert vs.total(ref, "evicts") > 0 and vs.total(ref, "overflow") > 0
