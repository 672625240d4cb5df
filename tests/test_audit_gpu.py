"""The view audit (gsp_scale_audit / gsp_pview_audit) against the CPU oracle.

The expected arrays come from tests/audit_oracle.py: numpy over the oracle's rows of the rows
alive at T, never the engine's own row().  The engine is stepped one tick at a time, the audit
taken at the listed ticks with every limit (and once more: identical arrays), its totals compared
with the same engine's census, and at the end every tick's digest still equals the oracle's, so
the audit disturbed nothing.

What the inputs exercise is asserted from the oracle's record itself: one class at T = 0 and 1,
thousands of classes and no exact view at T = 12, dead members listed at T = 12 and 20 and gone
from T = 24 on, suspects at limit 3 and none at limit 9, ticks past the mod-32 wrap of the stored
timestamp, stale entries in the rows that are not alive (a kernel that read them would differ),
nodes that have not started, rows shorter than the view and an empty live row.
"""
import numpy as np
import pytest

from gossip_protocol_amd.pview import PviewEngine
from gossip_protocol_amd.scale import ScaleEngine, make_policy
from tests import audit_oracle as ao
from tests.audit_oracle import ALIVE, FULL, NOT_STARTED, PVIEW

pytestmark = pytest.mark.gpu


def _summary(ref, t, lim):
    return ao.as_audit(ref["audit"][t], t, lim).summary()


def _run(eng, w, ref):
    """Step to the end, audit at the listed ticks, digests at the end."""
    n = w["n"]
    for t in range(0, w["ticks"] + 1):
        if t:
            eng.step(1)
        if t not in w["at"]:
            continue
        want = ref["audit"][t]
        for lim in w["limits"]:
            got = eng.audit() if lim is None else eng.audit(lim)
            lim = ao.limit_of(lim, w["kw"])
            tag = "tick %d age_limit %d" % (t, lim)
            assert got.tick == t and got.info["age_limit"] == lim and got.info["n"] == n, tag
            assert ao.mismatches(got, want, lim) == [], tag
            assert got.info["alive"] == int(want["live"].sum()), tag
            assert got.info["entries"] == int(want["size"].sum(dtype=np.int64)), tag
            assert got.info["kernel_ms"] > 0, tag
            assert got.summary() == ao.as_audit(want, t, lim).summary(), tag
        again = eng.audit(lim)
        for f in ao.FIELDS:
            assert np.array_equal(getattr(again, f), getattr(got, f)), "repeat %s %s" % (f, tag)
        # rows and columns sum to the same totals
        s, c = got.summary(), eng.census(lim)
        assert got.info["entries"] == c.info["entries"], tag
        assert s["dead_pairs"] == c.summary()["stale_pairs"], tag
        if not (want["state"] == NOT_STARTED).any():
            assert s["missing_pairs"] == c.summary()["missing_pairs"], tag
    for t in range(1, w["ticks"] + 1):
        assert eng.digest(t) == ref["digest"][t], "digest of tick %d after the audit" % t


def test_full_view_inputs_exercise_the_paths():
    ref = ao.full_reference("main")
    for t in (0, 1):
        s = _summary(ref, t, 9)
        assert s["classes"] == 1 and s["exact"] == s["alive"] == 3000 and s["converged"]
    s12, s20 = _summary(ref, 12, 9), _summary(ref, 20, 9)
    assert s12["alive"] == 2948 and s12["classes"] == 2374 and s12["exact"] == 0
    assert s12["dead_pairs"] == 150992 and s12["views_with_dead"] == 2948
    assert s20["exact"] == 806 and s20["dead_pairs"] == 266 and s20["views_with_dead"] == 234
    assert s20["classes"] == 1909
    for t in (24, 33, 40):
        assert _summary(ref, t, 9)["dead_pairs"] == 0, t
    for t in (12, 13, 20, 24, 33, 40):
        assert _summary(ref, t, 3)["suspect_pairs"] > 0, t
        assert _summary(ref, t, 9)["suspect_pairs"] == 0, t
        assert _summary(ref, t, 32)["suspect_pairs"] == 0, t
        assert ref["audit"][t]["stale_rows"] > 0, t           # a crashed row's buffer is stale
    assert max(_summary(ref, t, 9)["max_age"] for t in FULL["main"]["at"]) == 8
    assert not _summary(ref, 40, 9)["converged"]
    # the other buffer holds another tick's views
    assert not np.array_equal(ref["audit"][12]["print"], ref["audit"][13]["print"])
    j = ao.full_reference("join")["audit"]
    assert np.array_equal(np.nonzero(j[5]["state"] == NOT_STARTED)[0], np.arange(120, 600))
    assert all((j[5][f][120:] == 0).all() for f in ("size", "dead", "age_sum", "age_max", "print"))


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_audit_matches_oracle(layout):
    w = FULL["main"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **layout, **w["kw"]) as eng:
        if layout.get("group") == 2:
            assert eng.layout() == (2, 0, 2048)
        _run(eng, w, ao.full_reference("main"))


@pytest.mark.parametrize("layout", [dict(), dict(group=2), dict(group=3, layout="rows")],
                         ids=["fused", "tiles2", "rows3"])
def test_full_view_audit_join_schedule(layout):
    w = FULL["join"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], policy=make_policy(**w["pol"]), **layout,
                     **w["kw"]) as eng:
        _run(eng, w, ao.full_reference("join"))


def test_full_view_audit_tfail_swim_default_age_limit():
    w = FULL["variants"]
    with ScaleEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, ao.full_reference("variants"))
        assert eng.audit().info["age_limit"] == 4


def test_audit_age_limit_out_of_range():
    from gossip_protocol_amd._lib import GspError
    with ScaleEngine(64, max_ticks=2) as eng:
        for bad in (0, 33, -1):
            with pytest.raises(GspError, match="gsp_scale_audit: age_limit"):
                eng.audit(bad)
    with PviewEngine(64, view=8, max_ticks=2) as eng:
        with pytest.raises(GspError, match="gsp_pview_audit: age_limit"):
            eng.audit(0)


def test_partial_view_inputs_exercise_the_paths():
    a = ao.pview_reference("A")
    assert _summary(a, 12, 9)["dead_pairs"] == 38 and _summary(a, 25, 9)["dead_pairs"] == 0
    assert _summary(a, 25, 9)["size_min"] == 4 and _summary(a, 25, 9)["size_max"] == 32
    assert a["audit"][12]["stale_rows"] > 0
    assert _summary(a, 12, 3)["suspect_pairs"] > 0
    b = ao.pview_reference("B")["audit"][40]
    empty = np.nonzero(b["live"] & (b["size"] == 0))[0]
    assert empty.size > 0, "no empty live row"
    assert np.array_equal(b["print"][empty], ao.fp(empty))


@pytest.mark.parametrize("group", [1, 3], ids=["one", "rows3"])
def test_partial_view_audit_matches_oracle(group):
    w = PVIEW["A"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], group=group, **w["kw"]) as eng:
        _run(eng, w, ao.pview_reference("A"))


def test_partial_view_audit_drain_all():
    w = PVIEW["B"]
    with PviewEngine(w["n"], max_ticks=w["ticks"], **w["kw"]) as eng:
        _run(eng, w, ao.pview_reference("B"))
