"""The sub-slab sweep of a column tile (scale_sweep_kernel, DESIGN.md "Column tiles") against
the scale-protocol oracle, the way test_columns8_matches_oracle compares: every tick's digest,
its sorted event records, then messages and sampled rows along the run and every 61st row at
the end.

group=2 makes 2,048-column tiles at n = 4,096 (4 sub-slabs of 512 columns) and one ragged tile
pair at n = 3,000 (the second tile holds 952 nodes: a sub-slab partly and sub-slabs wholly
beyond n).  GSP_TEST_SCALE_SWEEP=512 selects the sweep, 0 the workgroup-per-row kernel.

The rows compared always include those whose own column is the first or the last of a sub-slab
and, each time rows are compared, receivers of the last tick's messages from such senders (the
two single-entry patches of the merge).

Rows with more messages than a wave orders in registers (64) are left to the workgroup-per-row
body.  The plain protocol cannot make one: a receiver's fan-in is a sum of independent choices
of probability fanout / members over the live senders, about Poisson(fanout) with fanout <= 16,
and only a join policy (which the sweep does not take) concentrates messages.  So the deferred
path is reached by lowering the bound (GSP_TEST_SCALE_SWEEP=512:K defers k > K), and the case
asserts from the oracle's own message list that such rows exist.

The oracle runs once per (n, fanout); the cases that share a workload share its record.
"""
import functools

import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine, unpack
from tests.oracle_binding import ScaleOracle

pytestmark = pytest.mark.gpu

EDGE = [511, 512, 1023, 1024, 2047, 2048]

CASES = [
    # id, n, fanout, switch, in-register bound of the case (None: the default)
    ("n4096_w512", 4096, 3, "512", None),
    ("n3000_w512", 3000, 3, "512", None),
    ("n4096_block_form", 4096, 3, "0", None),
    ("n4096_fanout16", 4096, 16, "512", None),
    ("n4096_fanout16_deferred", 4096, 16, "512:24", 24),
]


def _workload(n, fanout):
    # TREMOVE as small as the fanout allows: removals (and the joins that follow them) start
    # inside a short run, by the thousand and not by the million
    return dict(fanout=fanout, tremove=9 if fanout == 3 else 4, fail_mode=FAIL_RANDOM, fail_tick=2,
                fail_ppm=20000, seed=n + fanout), (12 if fanout == 3 else 7)


def _pairs(src, dst):
    return sorted(zip(src.tolist(), dst.tolist()))


@functools.lru_cache(maxsize=None)
def _reference(n, fanout):
    """The oracle's run: per tick the digest, the sorted events and the messages sent (index 0:
    the initial sends); at the compared ticks and at the end, the rows compared."""
    kw, ticks = _workload(n, fanout)
    orc = ScaleOracle(n, **kw)
    rng = np.random.default_rng(n)
    fail = np.array([orc.fail_tick(r) for r in range(n)])
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
        k, r, x = orc.events()
        ref["events"].append(sorted(zip(k.tolist(), r.tolist(), x.tolist())))
        ref["msgs"].append(orc.messages())
        if t % 4 == 0 or t == ticks:
            edge_recv = sorted(set(dst[np.isin(src, EDGE)].tolist()))
            assert edge_recv, "no receiver with a sender on a sub-slab boundary"
            ids = set(rng.integers(0, n, 8).tolist()) | {0, n - 1} | set(EDGE) | set(edge_recv[:4])
            if t == ticks:
                ids |= set(range(0, n, 61))
            ref["rows"][t] = rows_of(t, sorted(ids))
    assert sum(d["removes"] for d in ref["digest"][1:]) > 0, "the run made no removal"
    orc.close()
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sweep_matches_oracle(case, monkeypatch):
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

    with ScaleEngine(n, max_ticks=ticks, group=2, events=True, **kw) as eng:
        assert eng.layout() == (2, 0, 2048)
        messages_equal(eng, 0)
        eng.drain_events()
        for t in range(1, ticks + 1):
            eng.step(1)
            got = eng.digest(t)
            assert got == ref["digest"][t], "tick %d\n got %s\nwant %s" % (t, got, ref["digest"][t])
            rec, lost = eng.drain_events()
            k, tk, r, x = _lib.split_events(rec)
            assert lost == 0 and np.all(tk == t)
            assert sorted(zip(k.tolist(), r.tolist(), x.tolist())) == ref["events"][t], "events tick %d" % t
            if t in ref["rows"]:
                messages_equal(eng, t)
                for r, (pres, hb, ts5, own) in ref["rows"][t].items():
                    p2, h2, t2 = unpack(eng.row(r))
                    assert np.array_equal(p2, pres), "presence row %d tick %d" % (r, t)
                    assert np.array_equal(h2[p2], hb[p2]), "hb row %d tick %d" % (r, t)
                    assert np.array_equal(t2[p2], ts5[p2]), "ts row %d tick %d" % (r, t)
                    if own is not None:
                        assert eng.own_hb(r) == own, "own hb row %d tick %d" % (r, t)
