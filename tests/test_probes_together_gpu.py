"""The three per-tick probes -- rumor trace, detection ledger, traffic ledger -- open on ONE engine
at once, with the three snapshot probes (census, view audit, overlay reach) read beside them.

The per-probe files each open their own kind; here engine A holds all three, and four more engines
of the same workload hold exactly one kind each (rumor / detect / traffic) or none (plain).  The
per-tick probes share the engine's timing-event pool, its stream and its schedule, so what A
returns for a probe must be what the engine holding only that probe returns, integer for integer:
every array, the tick and every info field except kernel_ms.  The snapshot results are compared
with the plain engine's, every read is made twice (a get leaves the device state alone), and
every tick's digest of A is the plain engine's.  One comparison is anchored outside the engines:
A's traffic at tick 20 against the numpy rule over the CPU oracle (tests/traffic_oracle.py).

After tick 20 the probes are closed in another order than they were opened in, two ticks run
without them, all are reopened and the run goes to its end: the results agree again, and the
counters are those of a probe opened at that tick.  With the full view the whole run is repeated
with timing off: the same results, and every kernel_ms exactly 0.0.

Workloads: the join schedules of tests/traffic_oracle.py (full view n = 600, 35 ticks; partial view
n = 1200, view 32, inbox 3, 40 ticks), each fused and in shards, with event records on.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd import traffic
from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import ScaleEngine, make_policy
from tests import traffic_oracle as to

pytestmark = pytest.mark.gpu

CASES = {"full-fused": ("full", dict()), "full-rows3": ("full", dict(group=3, layout="rows")),
         "pview-fused": ("pview", dict()), "pview-rows2": ("pview", dict(group=2))}
OPENED = ("rumor", "detect", "traffic")          # the order A opens them in
CLOSED = ("traffic", "rumor", "detect")          # ... and closes them in
SNAPSHOTS = ("census", "audit", "reach")
T_CLOSE, T_REOPEN = 20, 22
TICKS_INFO = {"rumor0": "ticks_traced", "rumor3": "ticks_traced", "detect": "ticks_folded",
              "traffic": "ticks_counted"}


def _open(eng, kinds, w):
    n = w["n"]
    if "rumor" in kinds:
        eng.rumor_open(4)
        eng.rumor_seed(0, 0)
        eng.rumor_seed(3, [1, 7, n - 1])         # n - 1 has not started yet: ignored
    if "detect" in kinds:
        eng.detect_open()
    if "traffic" in kinds:
        eng.traffic_open(to.watch_of(w))


def _close(eng, kinds):
    for k in CLOSED:
        if k in kinds:
            getattr(eng, k + "_close")()


def _read(eng, kinds, snapshots):
    out = {}
    if snapshots:
        out.update(census=eng.census(), audit=eng.audit(), reach=eng.reach(0))
    if "rumor" in kinds:
        out.update(rumor0=eng.rumor(0), rumor3=eng.rumor(3))
    if "detect" in kinds:
        out["detect"] = eng.detect()
    if "traffic" in kinds:
        out["traffic"] = eng.traffic()
    return out


@functools.lru_cache(maxsize=None)
def _run(case, kinds, snapshots, timing=True):
    """One engine of the case's workload with `kinds` open from tick 0, closed after T_CLOSE and
    reopened at T_REOPEN: {tick: (first read, second read)} and the digests.  Computed once per
    process and left unchanged."""
    kind, layout = CASES[case]
    w = to.WORKLOADS[kind, "join"]
    cls = PviewEngine if kind == "pview" else ScaleEngine
    reads = {}
    with cls(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), events=True,
             event_cap=1 << 20, **layout, **w["kw"]) as eng:
        if not timing:
            eng.set_timing(False)
        _open(eng, kinds, w)
        for t in range(0, w["ticks"] + 1):
            if t:
                eng.step(1)
            if t == T_REOPEN:
                _open(eng, kinds, w)
            if t in w["at"] or t == T_REOPEN:
                reads[t] = (_read(eng, kinds, snapshots), _read(eng, kinds, snapshots))
            if t == T_CLOSE:
                _close(eng, kinds)
        digests = [eng.digest(t) for t in range(1, w["ticks"] + 1)]
    return reads, digests


def _facts(res):
    """Everything a result carries but the GPU time: its tick, its arrays, its info."""
    arrays = {k: v for k, v in vars(res).items() if isinstance(v, np.ndarray)}
    info = {k: v for k, v in res.info.items() if k != "kernel_ms"}
    return res.tick, arrays, info


def _assert_equal(a, b, tag):
    (ta, xa, ia), (tb, xb, ib) = _facts(a), _facts(b)
    assert type(a) is type(b) and ta == tb and ia == ib, (tag, ia, ib)
    assert xa.keys() == xb.keys() and len(xa) >= 2, tag
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape, (tag, k)
        assert np.array_equal(xa[k], xb[k]), "%s.%s: %d differ" % (tag, k, int((xa[k] != xb[k]).sum()))


def _assert_traffic_is_the_oracles(got, want, tag):
    """Field for field against a snapshot of tests/traffic_oracle.py, as tests/test_traffic_gpu.py
    compares its engines."""
    assert got.tick == want["info"]["tick"], tag
    for a in traffic.ARRAYS + ("state", "by_tick", "fanin", "watch"):
        g, e = getattr(got, a), want[a]
        assert g.shape == e.shape, "%s %s: shape %s != %s" % (a, tag, g.shape, e.shape)
        diff = g.astype(np.int64) != e
        assert not diff.any(), "%s %s: %d differ, first at %s" % (a, tag, int(diff.sum()), np.argwhere(diff)[0].tolist())
    for f in to.INFO:
        assert got.info[f] == want["info"][f], "info.%s %s: %r != %r" % (f, tag, got.info[f], want["info"][f])


def _assert_same_reads(got, want, names, tag):
    assert got.keys() == want.keys(), tag
    for t in got:
        for name in names:
            for again in range(2):
                _assert_equal(got[t][again][name], want[t][again][name], "%s %s tick %d read %d" % (tag, name, t, again))


@pytest.mark.parametrize("case", sorted(CASES))
def test_all_probes_on_one_engine_equal_one_probe_per_engine(case):
    kind = CASES[case][0]
    w = to.WORKLOADS[kind, "join"]
    assert T_CLOSE in w["at"] and max(w["at"]) > T_REOPEN and T_REOPEN not in w["at"]
    all_reads, all_digests = _run(case, OPENED, True)
    for t, (first, second) in all_reads.items():
        assert set(first) == set(SNAPSHOTS) | set(TICKS_INFO), t
        for name in first:                               # the repeated get is identical
            _assert_equal(first[name], second[name], "%s: repeated %s at tick %d" % (case, name, t))
    plain_reads, plain_digests = _run(case, (), True)
    _assert_same_reads(all_reads, plain_reads, SNAPSHOTS, case + " vs plain")
    assert all_digests == plain_digests
    for one, names in (("rumor", ("rumor0", "rumor3")), ("detect", ("detect",)), ("traffic", ("traffic",))):
        one_reads, one_digests = _run(case, (one,), False)
        _assert_same_reads(all_reads, one_reads, names, case + " vs " + one + " alone")
        assert one_digests == plain_digests, one
    # the counters of a probe opened at tick 0, then of one opened at T_REOPEN; the sources that
    # count are those alive at the seed tick by the oracle's schedule
    ref = to.reference(kind, "join")
    for t, (first, _) in all_reads.items():
        opened = 0 if t <= T_CLOSE else T_REOPEN
        for name, field in TICKS_INFO.items():
            assert first[name].info[field] == t - opened, (name, t, first[name].info)
        assert first["detect"].info["open_tick"] == first["traffic"].info["open_tick"] == opened, t
        for name, ids in (("rumor0", [0]), ("rumor3", [1, 7, w["n"] - 1])):
            alive = int(to.alive_at(ref["start"], ref["fail"], opened)[ids].sum())
            assert first[name].info["sources"] == alive, (name, t, first[name].info)
            assert first[name].info["seed_tick"] == (opened if alive else -1), (name, t)
    at_reopen = all_reads[T_REOPEN][0]
    assert not at_reopen["traffic"].sent.any() and at_reopen["detect"].info["ticks_folded"] == 0
    assert at_reopen["rumor3"].info["known"] == at_reopen["rumor3"].info["sources"] > 0
    # anchored outside the engines: the numpy rule over the CPU oracle, ledger opened at tick 0
    _assert_traffic_is_the_oracles(all_reads[T_CLOSE][0]["traffic"], ref["at"][T_CLOSE],
                                   "%s: traffic at tick %d with every probe open" % (case, T_CLOSE))
    # timing is on: a snapshot took GPU time, and so did a per-tick probe once it has run a tick
    for t, (first, _) in all_reads.items():
        for name in SNAPSHOTS:
            assert first[name].info["kernel_ms"] > 0, (name, t)
        for name, field in TICKS_INFO.items():
            assert first[name].info[field] == 0 or first[name].info["kernel_ms"] > 0, (name, t, first[name].info)


@pytest.mark.parametrize("case", ["full-fused", "full-rows3"])
def test_timing_off_changes_nothing_but_kernel_ms(case):
    timed, timed_digests = _run(case, OPENED, True)
    quiet, quiet_digests = _run(case, OPENED, True, timing=False)
    names = SNAPSHOTS + tuple(TICKS_INFO)
    _assert_same_reads(quiet, timed, names, case + " timing off vs on")
    assert quiet_digests == timed_digests
    for t, reads in quiet.items():
        for r in reads:
            for name in names:
                assert r[name].info["kernel_ms"] == 0.0, (name, t, r[name].info)
