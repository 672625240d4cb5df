"""Traffic ledger (gsp_scale_traffic_* / gsp_pview_traffic_*) against the numpy rule over the CPU
oracle.

The expected arrays come from tests/traffic_oracle.py, which reads only the oracle's messages(),
joinreps(), start_tick(), fail_tick(), row() and step() digests -- never engine output.  Every
oracle workload runs once per process (tests/test_traffic_cpu.py shows that these runs satisfy
the five per-tick identities by themselves).  A ledger is opened at tick 0 with some seventy
watched nodes, the engine is stepped, and at the listed ticks every per-node array, by_tick, fanin,
the watch rows, state and every info field but kernel_ms (> 0) is compared.  A repeated get is
identical, and at the end every tick's digest equals the oracle's.

What the inputs exercise is asserted from the oracle's own record: a segment past 64 (the
wave-cooperative path), messages lost to receivers that are not alive, an inbox overflow, a merged
JOINREP, a TFAIL payload smaller than the view, and five populated fan-in buckets.
"""
import ctypes

import numpy as np
import pytest

from gossip_protocol_amd import _lib, traffic
from gossip_protocol_amd._lib import GspError
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import ScaleEngine, make_policy
from tests import traffic_oracle as to

pytestmark = pytest.mark.gpu

W = to.WORKLOADS
ARRAYS = traffic.ARRAYS + ("state", "by_tick", "fanin", "watch")


def _engine(kind, name, max_ticks=None, **layout):
    w = W[kind, name]
    pol = make_policy(**w["pol"]) if w["pol"] else None
    cls = PviewEngine if kind == "pview" else ScaleEngine
    return cls(w["n"], max_ticks=max_ticks or w["ticks"], policy=pol, **layout, **w["kw"])


def _compare(got, want, tag):
    assert got.tick == want["info"]["tick"], tag
    assert (got.sent.dtype, got.entries_in.dtype, got.peak_tick.dtype) == (np.uint32, np.uint64, np.int32)
    for a in ARRAYS:
        g, e = getattr(got, a), want[a]
        assert g.shape == e.shape, "%s %s: shape %s != %s" % (a, tag, g.shape, e.shape)
        diff = g.astype(np.int64) != e
        assert not diff.any(), "%s %s: %d differ, first at %s: %s != %s" % (
            a, tag, int(diff.sum()), np.argwhere(diff)[0].tolist(), g[diff][:4].tolist(), e[diff][:4].tolist())
    for f in to.INFO:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ARRAYS) \
        and {f: a.info[f] for f in to.INFO} == {f: b.info[f] for f in to.INFO}


def _run(eng, kind, name, chunk=1, at=None):
    """Open at tick 0, compare at the listed ticks, digests at the end."""
    w, ref = W[kind, name], to.reference(kind, name)
    eng.traffic_open(to.watch_of(w))
    for t in range(0, w["ticks"] + 1, chunk):
        if t:
            eng.step(chunk)
        if t not in (at or w["at"]):
            continue
        got = eng.traffic()
        _compare(got, ref["at"][t], "tick %d" % t)
        if t:
            assert got.info["kernel_ms"] > 0, t
        assert _same(eng.traffic(), got), "a repeated get at tick %d" % t
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d with a ledger open" % t


def _buckets(led):
    return led.fanin.sum(axis=0) > 0


def test_full_view_inputs_exercise_the_paths():
    for name in ("main", "join", "burst", "variants"):
        led = to.reference("full", name)["ledger"]
        b = _buckets(led)
        assert led.lost.sum() > 0 and b[0] and b[1:].sum() >= 4, (name, b.tolist())
        assert (led.recv == led.merged).all(), name      # the full view merges everything
    assert to.reference("full", "main")["ledger"].longest <= 64
    assert to.reference("full", "burst")["ledger"].longest > 64      # the wave-cooperative path
    assert to.reference("full", "join")["ledger"].joinreps_merged > 100
    assert to.reference("full", "variants")["ledger"].cut_payloads > 0


def test_partial_view_inputs_exercise_the_paths():
    for name in ("A7", "A2", "A0", "B", "join", "tfail"):
        led = to.reference("pview", name)["ledger"]
        b = _buckets(led)
        assert led.lost.sum() > 0 and b[0] and b[1:].sum() >= 4, (name, b.tolist())
    over = {k: int((to.reference("pview", k)["ledger"].recv - to.reference("pview", k)["ledger"].merged).sum())
            for k in ("A7", "A2", "A0", "B", "join", "tfail")}
    assert over["A2"] > over["A7"] > 0 and over["A0"] == 0 and over["B"] == 0, over
    assert over["join"] > 0 and over["tfail"] > 0
    assert to.reference("pview", "A7")["ledger"].longest > 64 and to.reference("pview", "A0")["ledger"].longest > 64
    assert to.reference("pview", "join")["ledger"].joinreps_merged > 0
    t = to.reference("pview", "tfail")["ledger"]
    assert t.cut_payloads > 0                            # a TFAIL payload smaller than the view


FULL_LAYOUTS = {
    "fused": dict(), "tiles2": dict(group=2), "tiles3": dict(group=3), "tiles8": dict(group=8),
    "rows2": dict(group=2, layout="rows"), "rows3": dict(group=3, layout="rows"),
}


@pytest.mark.parametrize("layout", sorted(FULL_LAYOUTS))
def test_full_view_traffic_matches_oracle(layout):
    with _engine("full", "main", **FULL_LAYOUTS[layout]) as eng:
        if layout == "tiles2":
            assert eng.layout() == (2, 0, 2048)
        _run(eng, "full", "main")


@pytest.mark.parametrize("sweep", ["0", "512"])
def test_full_view_traffic_both_row_forms(sweep, monkeypatch):
    """Column tiles with the workgroup-per-row kernel and with the sub-slab sweep."""
    monkeypatch.setenv("GSP_TEST_SCALE_SWEEP", sweep)
    with _engine("full", "main", group=2) as eng:
        _run(eng, "full", "main", at=(12, 40))


@pytest.mark.parametrize("name,layout", [("join", "fused"), ("join", "tiles2"), ("join", "rows3"),
                                         ("burst", "fused"), ("burst", "rows3"), ("variants", "fused"),
                                         ("variants", "tiles3")])
def test_full_view_traffic_join_burst_and_variants(name, layout):
    with _engine("full", name, **FULL_LAYOUTS[layout]) as eng:
        _run(eng, "full", name)


@pytest.mark.parametrize("name,group", [("A7", 1), ("A7", 2), ("A7", 3), ("A2", 1), ("A0", 1), ("A0", 3),
                                        ("B", 1), ("join", 1), ("join", 3), ("tfail", 1), ("tfail", 3)],
                         ids=["inbox7", "inbox7-rows2", "inbox7-rows3", "inbox2", "drain", "drain-rows3",
                              "B-drain", "join", "join-rows3", "tfail", "tfail-rows3"])
def test_partial_view_traffic_matches_oracle(name, group):
    with _engine("pview", name, group=group) as eng:
        _run(eng, "pview", name)


@pytest.mark.parametrize("kind,name,layout", [("full", "main", dict()), ("full", "burst", dict()),
                                              ("full", "join", dict(group=3, layout="rows")),
                                              ("pview", "A7", dict()), ("pview", "A0", dict()),
                                              ("pview", "join", dict(group=3))],
                         ids=["main", "burst", "join-rows3", "inbox7", "drain", "pview-join-rows3"])
def test_sender_side_from_the_csr_is_the_same_ledger(kind, name, layout, monkeypatch):
    """The measured alternative: sent taken from the next tick's receiver CSR with one atomic per
    message, the last tick folded at get."""
    monkeypatch.setenv("GSP_TEST_TRAFFIC_FORM", "1")
    with _engine(kind, name, **layout) as eng:
        _run(eng, kind, name)


@pytest.mark.parametrize("form", ["0", "1"])
def test_step_five_equals_five_steps(form, monkeypatch):
    monkeypatch.setenv("GSP_TEST_TRAFFIC_FORM", form)
    assert all(t % 5 == 0 for t in W["full", "join"]["at"])
    with _engine("full", "join") as eng:
        _run(eng, "full", "join", chunk=5)
    with _engine("pview", "A7") as eng:
        _run(eng, "pview", "A7", chunk=5, at=(0, 25, 40))


def _opened_at(kind, name, t0, ticks, at):
    w = W[kind, name]
    orc = to.make_oracle(kind, name)
    ref = to.run(orc, kind, w["n"], ticks, w["kw"].get("inbox", 0), w["kw"].get("tfail", 0),
                 (w["pol"] or {}).get("intro_list", 0), set(at), t0, to.watch_of(w))
    orc.close()
    return ref


@pytest.mark.parametrize("kind,form", [("full", "0"), ("pview", "0"), ("pview", "1")])
def test_open_mid_run_covers_only_the_later_ticks(kind, form, monkeypatch):
    monkeypatch.setenv("GSP_TEST_TRAFFIC_FORM", form)
    ref = _opened_at(kind, "join", 7, 20, (7, 8, 20))
    with _engine(kind, "join") as eng:
        eng.step(7)
        eng.traffic_open(to.watch_of(W[kind, "join"]))
        got = eng.traffic()
        _compare(got, ref["at"][7], "opened at 7")
        assert not (got.sent.any() or got.recv.any() or got.by_tick.any() or got.watch.any())
        assert (got.peak_tick == -1).all() and got.info["max_fanin_node"] == -1
        eng.step(1)
        _compare(eng.traffic(), ref["at"][8], "opened at 7, tick 8")
        eng.step(12)
        got = eng.traffic()
        _compare(got, ref["at"][20], "opened at 7, tick 20")
        assert not got.by_tick[:8].any() and not got.fanin[:8].any() and got.by_tick[8:].all(axis=0)[:2].all()


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_close_then_reopen_starts_empty(kind):
    ref = _opened_at(kind, "join", 6, 12, (12,))
    full = to.reference(kind, "join")
    with _engine(kind, "join") as eng:
        eng.traffic_open([0, 5])
        with pytest.raises(GspError, match="already open"):
            eng.traffic_open()
        eng.step(4)
        assert eng.traffic().info["sent"] == int(full["ledger"].by_tick[1:5, 0].sum()) > 0
        eng.traffic_close()
        for call in (eng.traffic, eng.traffic_close):
            with pytest.raises(GspError, match="no ledger is open"):
                call()
        eng.step(2)                                      # ticks without a ledger
        eng.traffic_open(to.watch_of(W[kind, "join"]))
        got = eng.traffic()
        assert not (got.sent.any() or got.lost.any() or got.entries_in.any() or got.fanin.any())
        assert (got.info["ticks_counted"], got.info["open_tick"], got.info["tick"]) == (0, 6, 6)
        eng.step(6)
        _compare(eng.traffic(), ref["at"][12], "reopened at 6")
        for t in range(1, 13):
            assert eng.digest(t) == full["digest"][t], t


@pytest.mark.parametrize("kind", ["full", "pview"])
def test_engine_without_a_ledger_is_undisturbed(kind):
    """Two engines side by side, one with a ledger: identical digests and rows."""
    w = W[kind, "join"]
    with _engine(kind, "join", max_ticks=20) as plain, _engine(kind, "join", max_ticks=20) as led:
        led.traffic_open(list(range(0, w["n"], 7))[:traffic.MAX_WATCH])
        for _ in range(4):
            plain.step(5)
            led.step(5)
        assert led.traffic().info["ticks_counted"] == 20
        for t in range(1, 21):
            assert plain.digest(t) == led.digest(t), t
        for r in range(0, w["n"], 37):
            a, b = plain.row(r), led.row(r)
            if kind == "pview":                          # (entries, length): the valid prefix
                assert a[1] == b[1], r
                a, b = a[0][:a[1]], b[0][:b[1]]
            assert np.array_equal(a, b), r


@pytest.mark.parametrize("kind,name", [("full", "burst"), ("pview", "A7")])
def test_write_msgcount_of_the_watched_nodes(kind, name, tmp_path):
    """The engine's watch rows through the writer equal the writer fed with the oracle's counts
    (more than 67 watched nodes: the reference's node-67 layout is among the rows)."""
    w, ref = W[kind, name], to.reference(kind, name)
    want = ref["at"][w["ticks"]]["watch"]
    assert want.shape[0] > 67 and want[66].any()
    with _engine(kind, name) as eng:
        eng.traffic_open(to.watch_of(w))
        eng.step(w["ticks"])
        got = eng.traffic()
    a, b = str(tmp_path / "engine.log"), str(tmp_path / "oracle.log")
    got.write_msgcount(a)
    traffic.write_msgcount(b, want[:, :, 0], want[:, :, 1])
    text = open(a, "rb").read()
    assert text == open(b, "rb").read()
    assert b"special" in text and text.count(b"sent_total") == want.shape[0]
    s = got.summary()
    led = ref["ledger"]
    assert s["sent"] == int(led.sent.sum()) and s["alive_node_rounds"] == int(led.fanin.sum())
    assert s["hubs"][0] == (want_hub(led))


def want_hub(led):
    top = int(led.peak.max())
    x = int(np.nonzero(led.peak == top)[0][0])
    return (x, top, int(led.peak_tick[x]))


def test_null_out_pointers_and_a_short_tick_cap():
    w, ref = W["full", "join"], to.reference("full", "join")
    want = ref["at"][20]
    with _engine("full", "join") as eng:
        eng.traffic_open([0, 599])
        eng.step(20)
        L = _lib.lib()
        info = _lib.GspTrafficInfo()
        assert L.gsp_scale_traffic_get(eng._h, *([None] * 11), 0, ctypes.byref(info)) == 0
        assert (info.tick, info.sent, info.lost, info.n_watch) == (20, want["info"]["sent"], want["info"]["lost"], 2)
        assert L.gsp_scale_traffic_get(eng._h, *([None] * 11), 0, None) == 0
        by_tick = np.full((5, 6), 77, np.uint64)
        watch = np.full((2, 5, 2), 77, np.uint32)
        PU64, PU32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        assert L.gsp_scale_traffic_get(eng._h, *([None] * 8), by_tick.ctypes.data_as(PU64), None,
                                       watch.ctypes.data_as(PU32), 5, None) == 0
        assert np.array_equal(by_tick, want["by_tick"][:5])
        ids = [to.watch_of(w).index(0), to.watch_of(w).index(599)]
        assert np.array_equal(watch, want["watch"][ids][:, :5])
        assert L.gsp_scale_traffic_get(eng._h, *([None] * 8), by_tick.ctypes.data_as(PU64), None, None, -1,
                                       None) == -1


def test_traffic_open_argument_errors():
    with ScaleEngine(64, max_ticks=2) as eng:
        for bad, msg in (([64], "outside"), ([-1], "outside"), ([3, 9, 3], "twice")):
            with pytest.raises(GspError, match=msg):
                eng.traffic_open(bad)
        for call in (eng.traffic, eng.traffic_close):
            with pytest.raises(GspError, match="no ledger is open"):
                call()
        eng.traffic_open(list(range(64)))                # the engine still answers
        eng.step(2)
        got = eng.traffic()
        assert got.watch.shape == (64, 3, 2) and got.info["ticks_counted"] == 2
        assert np.array_equal(got.watch[:, :, 0].sum(axis=1), got.sent)
        assert np.array_equal(got.watch[:, :, 1].sum(axis=1), got.recv)
    with PviewEngine(2048, view=32, max_ticks=2) as eng:
        with pytest.raises(GspError, match="gsp_pview_traffic_open.*n_watch"):
            eng.traffic_open(list(range(traffic.MAX_WATCH + 1)))
        eng.traffic_open(list(range(traffic.MAX_WATCH)))
        eng.step(1)
        assert eng.traffic().watch.shape == (traffic.MAX_WATCH, 2, 2)
