"""The sub-slab sweep of a whole tile group in one launch (scale_sweep_kernel over every local
tile, DESIGN.md "Sub-slab sweep") with more than two tiles, compared the way
tests/test_scale_sweep_gpu.py compares: every tick's digest, its sorted event records with
lost == 0, then messages and sampled rows along the run and every 61st row at the end.

group=3 makes three 2,048-column tiles (4 sub-slabs of 512 columns each), a tile count that is
no power of two: n = 6,144 fills them, n = 5,000 leaves the last tile 904 nodes (one sub-slab
partly and two wholly beyond n) and n = 4,100 leaves it 4.  The last case lowers the in-register
bound (GSP_TEST_SCALE_SWEEP=512:24), so rows are deferred to the workgroup-per-row body: every
tile of the group reads the owner's lists, only the owner's sweep items append to them, and a
row appended once per tile would be run once per tile -- own heartbeat, digest and events
would all show it.  group=8 at n = 16,384 is past what the oracle runs in a test's time, so the
sweep is compared with the workgroup-per-row form (GSP_TEST_SCALE_SWEEP=0), which
tests/test_scale_sweep_gpu.py and tests/test_scale_gpu.py hold to the oracle.

The rows compared always include 0 and n - 1 and those whose own column is the first or the
last of a sub-slab (so also of a tile), and receivers of the last tick's messages from such
senders.  The oracle runs once per (n, fanout).
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, unpack
from tests.oracle_binding import ScaleOracle

pytestmark = pytest.mark.gpu

STRIDE = 2048      # columns per tile in every case here
W = 512            # columns per sub-slab

CASES = [
    # id, n, fanout, switch, in-register bound of the case (None: the default)
    ("n6144_three_tiles", 6144, 3, "512", None),
    ("n5000_ragged_last_tile", 5000, 3, "512", None),
    ("n4100_fanout16_deferred", 4100, 16, "512:24", 24),
]


def _edges(n):
    """Rows whose own column is the first or the last of a sub-slab (every fourth: of a tile)."""
    return sorted({c for b in range(W, n + W, W) for c in (b - 1, b) if c < n})


def _workload(n, fanout):
    return dict(fanout=fanout, tremove=9 if fanout == 3 else 4, fail_mode=FAIL_RANDOM, fail_tick=2,
                fail_ppm=20000, seed=n + fanout), (12 if fanout == 3 else 7)


def _event_keys(k, r, x):
    """One sortable key per record of a tick (kind, row, column)."""
    return np.sort((k.astype(np.uint64) << np.uint64(42)) | (r.astype(np.uint64) << np.uint64(21)) |
                   x.astype(np.uint64))


def _pairs(src, dst):
    return sorted(zip(src.tolist(), dst.tolist()))


@functools.lru_cache(maxsize=None)
def _reference(n, fanout):
    """The oracle's run: per tick the digest, the sorted event keys and the messages sent (index
    0: the initial sends); at the compared ticks and at the end, the rows compared."""
    kw, ticks = _workload(n, fanout)
    orc = ScaleOracle(n, **kw)
    rng = np.random.default_rng(n)
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    edges = _edges(n)
    ref = {"fail": fail, "digest": [None], "events": [None], "msgs": [orc.messages()], "rows": {}}

    def rows_of(t, ids):
        out = {}
        for r in ids:
            pres, hb, ts = orc.row(r)
            out[r] = (pres.astype(bool), hb, ts & 31, orc.own_hb(r) if fail[r] >= t else None)
        return out

    for t in range(1, ticks + 1):
        src, dst = ref["msgs"][t - 1]
        ref["digest"].append(orc.step())
        ref["events"].append(_event_keys(*orc.events()))
        ref["msgs"].append(orc.messages())
        if t % 4 == 0 or t == ticks:
            edge_recv = sorted(set(dst[np.isin(src, edges)].tolist()))
            assert edge_recv, "no receiver with a sender on a sub-slab boundary"
            ids = set(rng.integers(0, n, 8).tolist()) | {0, n - 1} | set(edges) | set(edge_recv[:4])
            if t == ticks:
                ids |= set(range(0, n, 61))
            ref["rows"][t] = rows_of(t, sorted(ids))
    assert sum(d["removes"] for d in ref["digest"][1:]) > 0, "the run made no removal"
    orc.close()
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_group_sweep_matches_oracle(case, monkeypatch):
    _, n, fanout, switch, bound = case
    monkeypatch.setenv("GSP_TEST_SCALE_SWEEP", switch)
    kw, ticks = _workload(n, fanout)
    ref = _reference(n, fanout)
    if bound is not None:          # live rows past the in-register bound, none past the block form's
        deferred = 0
        for t in range(1, ticks + 1):
            k = np.bincount(ref["msgs"][t - 1][1], minlength=n)
            assert k.max() <= 1024
            deferred += int(((k > bound) & (ref["fail"] >= t)).sum())
        assert deferred > 0, "no live row got more than %d messages" % bound

    def messages_equal(eng, t):
        m = eng.messages()
        assert sorted((s, d) for s in range(n) for d in m[s] if d >= 0) == _pairs(*ref["msgs"][t]), \
            "messages tick %d" % t

    with ScaleEngine(n, max_ticks=ticks, group=3, events=True, **kw) as eng:
        assert eng.layout() == (3, 0, STRIDE)
        # the sweep is what runs (not the workgroup-per-row form behind a switch that did not take)
        assert eng.sweep() == (W, bound if bound is not None else 64)
        messages_equal(eng, 0)
        eng.drain_events()
        for t in range(1, ticks + 1):
            eng.step(1)
            got = eng.digest(t)
            assert got == ref["digest"][t], "tick %d\n got %s\nwant %s" % (t, got, ref["digest"][t])
            rec, lost = eng.drain_events()
            k, tk, r, x = _lib.split_events(rec)
            assert lost == 0 and np.all(tk == t)
            assert np.array_equal(_event_keys(k, r, x), ref["events"][t]), "events tick %d" % t
            if t in ref["rows"]:
                messages_equal(eng, t)
                for r, (pres, hb, ts5, own) in ref["rows"][t].items():
                    p2, h2, t2 = unpack(eng.row(r))
                    assert np.array_equal(p2, pres), "presence row %d tick %d" % (r, t)
                    assert np.array_equal(h2[p2], hb[p2]), "hb row %d tick %d" % (r, t)
                    assert np.array_equal(t2[p2], ts5[p2]), "ts row %d tick %d" % (r, t)
                    if own is not None:
                        assert eng.own_hb(r) == own, "own hb row %d tick %d" % (r, t)


def _engine_record(n, ticks, kw, row_ids, width):
    """One engine run of eight tiles in the form `width` (eng.sweep): per tick the digest and the
    sorted event keys; at every fourth tick and at the end the messages and the rows `row_ids`
    with their own heartbeats."""
    rec = {"digest": [], "events": [], "msgs": {}, "rows": {}}
    with ScaleEngine(n, max_ticks=ticks, group=8, events=True, **kw) as eng:
        assert eng.layout() == (8, 0, STRIDE)
        assert eng.sweep()[0] == width
        rec["msgs"][0] = np.asarray(eng.messages()).copy()
        eng.drain_events()
        for t in range(1, ticks + 1):
            eng.step(1)
            rec["digest"].append(eng.digest(t))
            ev, lost = eng.drain_events()
            k, tk, r, x = _lib.split_events(ev)
            assert lost == 0 and np.all(tk == t)
            rec["events"].append(_event_keys(k, r, x))
            if t % 4 == 0 or t == ticks:
                rec["msgs"][t] = np.asarray(eng.messages()).copy()
                rec["rows"][t] = [(np.asarray(eng.row(r)).copy(), eng.own_hb(r)) for r in row_ids]
    return rec


def test_group8_sweep_matches_block_form(monkeypatch):
    n = 16384
    kw, ticks = _workload(n, 3)
    rng = np.random.default_rng(n)
    row_ids = sorted(set(rng.integers(0, n, 8).tolist()) | {0, n - 1} | set(_edges(n)))
    monkeypatch.setenv("GSP_TEST_SCALE_SWEEP", "0")
    want = _engine_record(n, ticks, kw, row_ids, 0)
    monkeypatch.setenv("GSP_TEST_SCALE_SWEEP", "512")
    got = _engine_record(n, ticks, kw, row_ids, W)
    assert sum(d["removes"] for d in want["digest"]) > 0, "the run made no removal"
    for t in range(1, ticks + 1):
        assert got["digest"][t - 1] == want["digest"][t - 1], \
            "tick %d\n got %s\nwant %s" % (t, got["digest"][t - 1], want["digest"][t - 1])
        assert np.array_equal(got["events"][t - 1], want["events"][t - 1]), "events tick %d" % t
    assert sorted(got["msgs"]) == sorted(want["msgs"])
    for t in want["msgs"]:
        assert np.array_equal(got["msgs"][t], want["msgs"][t]), "messages tick %d" % t
    for t in want["rows"]:
        for r, (a, ha), (b, hb) in zip(row_ids, got["rows"][t], want["rows"][t]):
            assert np.array_equal(a, b), "row %d tick %d" % (r, t)
            assert ha == hb, "own hb row %d tick %d" % (r, t)
