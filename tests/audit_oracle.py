"""The view audit expected from the CPU oracle (shared by tests/test_audit_gpu.py and
tests/audit_ranks.py).

The expected arrays are numpy over the oracle's rows (ScaleOracle.row / PviewOracle.row) of the
rows alive at T -- start_tick(r) <= T <= fail_tick(r) -- never the engine's own row().  fp is
restated here in numpy uint64.  Every oracle workload runs once per process; the cases that
share it share its record.  The workloads are the census tests' (tests/test_census_gpu.py): they
are already the smallest shapes that reach the edges.
"""
import functools

import numpy as np

from tests.oracle_binding import PviewOracle, ScaleOracle
from tests.oracle_binding import make_policy as oracle_policy

NOT_STARTED, ALIVE, CRASHED = 0, 1, 2
FAIL_RANDOM = 1
FIELDS = ("state", "size", "dead", "suspect", "age_sum", "age_max", "print")
LIMITS = (3, 9, 32)

FULL = {
    # n = 3000 in 2,048-column tiles: a ragged second tile of 952 nodes and a ragged 16-byte
    # vector at the table's edge (3000 = 8 * 375); T = 33, 40 lie past the mod-32 wrap
    "main": dict(n=3000, ticks=40, at=(0, 1, 12, 13, 20, 24, 33, 40), limits=LIMITS, pol=None,
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=2, fail_ppm=20000,
                         seed=3003)),
    # node i starts at int(0.05 i): at T = 5 exactly the nodes >= 120 have not started
    "join": dict(n=600, ticks=35, at=(5, 20, 35), limits=LIMITS,
                 pol=dict(step_rate=0.05, intro_list=8),
                 kw=dict(fanout=3, tremove=9, fail_mode=FAIL_RANDOM, fail_tick=10, fail_ppm=20000,
                         seed=600)),
    # TFAIL + SWIM change nothing in what is audited; age_limit defaults to tfail
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


def fp(x):
    """splitmix64 finaliser of the ids x, mod 2^64."""
    z = np.asarray(x).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def limit_of(lim, kw):
    return lim if lim is not None else (kw.get("tfail") or kw["tremove"])


def states(orc, n, t):
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    start = np.array([orc.start_tick(r) for r in range(n)])
    return np.where(start > t, NOT_STARTED, np.where(fail >= t, ALIVE, CRASHED)).astype(np.uint8)


def _finish(n, state, out, limits, kw):
    """Zero the rows that are not alive; the per-limit suspect arrays keyed by the limit."""
    live = state == ALIVE
    res = {"state": state, "live": live}
    for f in ("size", "dead", "age_sum", "age_max", "print"):
        res[f] = np.where(live, out[f], 0).astype(
            {"age_max": np.uint8, "print": np.uint64}.get(f, np.uint32))
    res["suspect"] = {limit_of(l, kw): np.where(live, out["suspect"](limit_of(l, kw)), 0).astype(np.uint32)
                      for l in limits}
    return res


def audit_of_matrix(n, t, state, pres, ts, limits, kw):
    """The audit of tick t from the matrices [observer][member] of the oracle's rows."""
    live = state == ALIVE
    age = (t - ts) & 31
    pa = pres & live[None, :]                       # entries of alive members
    fpx = fp(np.arange(n))
    out = {"size": pres.sum(1), "dead": (pres & ~live[None, :]).sum(1),
           "age_sum": np.where(pa, age, 0).sum(1), "age_max": np.where(pa, age, 0).max(1),
           "print": np.where(pres, fpx[None, :], np.uint64(0)).sum(1, dtype=np.uint64) + fpx,
           "suspect": lambda lim: (pa & (age >= lim)).sum(1)}
    res = _finish(n, state, out, limits, kw)
    # what the rows that are not alive still hold: a kernel that read them would report it
    res["stale_rows"] = int((pres[~live].sum(1) > 0).sum())
    return res


def audit_of_lists(n, t, state, rows, limits, kw):
    """The audit of tick t from the oracle's partial views, rows[r] = (ids, hb, ts)."""
    live = state == ALIVE
    z = lambda dt=np.int64: np.zeros(n, dt)
    size, dead, age_sum, age_max, prints = z(), z(), z(), z(), z(np.uint64)
    sus = {limit_of(l, kw): z() for l in limits}
    fpx = fp(np.arange(n))
    for r in np.nonzero(live)[0]:
        ids, _, ts = rows[r]
        assert ((ids >= 0) & (ids < n)).all()
        al = live[ids]
        age = ((t - ts) & 31)[al]
        size[r], dead[r] = len(ids), int((~al).sum())
        age_sum[r], age_max[r] = int(age.sum()), int(age.max()) if age.size else 0
        prints[r] = np.append(fpx[ids], fpx[r]).sum(dtype=np.uint64)      # wraps mod 2^64
        for lim in sus:
            sus[lim][r] = int((age >= lim).sum())
    out = {"size": size, "dead": dead, "age_sum": age_sum, "age_max": age_max, "print": prints,
           "suspect": lambda lim: sus[lim]}
    res = _finish(n, state, out, limits, kw)
    res["stale_rows"] = int(sum(len(rows[r][0]) > 0 for r in np.nonzero(~live)[0]))
    return res


@functools.lru_cache(maxsize=None)
def full_reference(name, ticks=None, at=None):
    w = FULL[name]
    n = w["n"]
    ticks, at = ticks or w["ticks"], at or w["at"]
    orc = ScaleOracle(n, policy=oracle_policy(**w["pol"]) if w["pol"] else None, **w["kw"])
    ref = {"digest": [None], "audit": {}}
    for t in range(0, ticks + 1):
        if t:
            ref["digest"].append(orc.step())
        if t in at:
            rows = [orc.row(r) for r in range(n)]
            pres = np.stack([x[0] for x in rows]).astype(bool)
            ts = np.stack([x[2] for x in rows])
            ref["audit"][t] = audit_of_matrix(n, t, states(orc, n, t), pres, ts, w["limits"], w["kw"])
    orc.close()
    return ref


@functools.lru_cache(maxsize=None)
def pview_reference(name, ticks=None, at=None):
    w = PVIEW[name]
    n = w["n"]
    ticks, at = ticks or w["ticks"], at or w["at"]
    orc = PviewOracle(n, **w["kw"])
    ref = {"digest": [None], "audit": {}}
    for t in range(0, ticks + 1):
        if t:
            ref["digest"].append(orc.step())
        if t in at:
            rows = [orc.row(r) for r in range(n)]
            ref["audit"][t] = audit_of_lists(n, t, states(orc, n, t), rows, w["limits"], w["kw"])
    orc.close()
    return ref


def as_audit(want, t, lim):
    """The expected arrays as an Audit, for its summary()."""
    from gossip_protocol_amd.audit import Audit
    return Audit(t, want["state"], want["size"], want["dead"], want["suspect"][lim], want["age_sum"],
                 want["age_max"], want["print"])


def mismatches(got, want, lim):
    """The fields of the Audit `got` that differ from the expectation, with a count each."""
    bad = []
    for f in FIELDS:
        w = want["suspect"][lim] if f == "suspect" else want[f]
        g = getattr(got, f)
        if g.dtype != w.dtype or not np.array_equal(g, w):
            bad.append((f, int((g != w).sum())))
    return bad
