#!/usr/bin/env python3
"""One rank of a census run across ranks (tests/test_census_rccl.py launches it under
torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/census_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 4096, view 32, row shards

Every rank steps the engine 13 ticks and runs the CPU oracle on the same inputs.  The census
is collective: each rank counts the rows and columns it holds and the arrays are all-reduced
over RCCL, so EVERY rank's census at ticks 0, 12 and 13 must equal the one numpy makes from the
oracle's rows.  torch.distributed (gloo) carries only the RCCL id and the verdicts.  Rank 0
prints one JSON line; exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANDOM = 1
TICKS, AT, LIMITS = 13, (0, 12, 13), (3, 9)


def expected(orc, n, t, pview):
    """The census of tick t from the oracle's rows: rows alive at t only."""
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    state = np.where(fail >= t, 1, 2).astype(np.uint8)      # no join schedule: all start at 0
    ids, hb, ts = [], [], []
    for r in np.nonzero(fail >= t)[0]:
        a, b, c = orc.row(int(r))
        if not pview:
            a, b, c = np.nonzero(a)[0], b[a.astype(bool)], c[a.astype(bool)]
        ids.append(a), hb.append(b), ts.append(c)
    ids, hb, ts = (np.concatenate(x) for x in (ids, hb, ts))
    max_hb = np.zeros(n, np.uint32)
    np.maximum.at(max_hb, ids, hb.astype(np.uint32))
    age = (t - ts) & 31
    return {"state": state, "max_hb": max_hb, "listed": np.bincount(ids, minlength=n).astype(np.uint32),
            "fresh": {l: np.bincount(ids[age < l], minlength=n).astype(np.uint32) for l in LIMITS}}


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine
    from tests import ranks_common
    from tests.oracle_binding import PviewOracle, ScaleOracle
    dist, rank, world, dev, uid = ranks_common.start()
    pview = case == "pview_rows"
    if pview:
        from gossip_protocol_amd.pview import PviewEngine
        n = 4096
        kw = dict(view=32, fanout=3, inbox=7, tremove=9, fail_mode=RANDOM, fail_tick=2,
                  fail_ppm=50000, seed=4128)
        orc = PviewOracle(n, **kw)
        eng = PviewEngine(n, max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid, **kw)
    else:
        n = 3000
        kw = dict(fanout=3, tremove=9, fail_mode=RANDOM, fail_tick=2, fail_ppm=20000, seed=3003)
        orc = ScaleOracle(n, **kw)
        eng = ScaleEngine(n, max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          tiles=2 if case == "columns_tiled" else 1,
                          layout="columns" if case == "columns_tiled" else "rows", **kw)
    bad = []
    for t in range(0, TICKS + 1):
        if t:
            orc.step()
            eng.step(1)
        if t not in AT:
            continue
        want = expected(orc, n, t, pview)
        for lim in LIMITS:
            got = eng.census(lim)
            for f, w in (("state", want["state"]), ("listed", want["listed"]),
                         ("fresh", want["fresh"][lim]), ("max_hb", want["max_hb"])):
                if not np.array_equal(getattr(got, f), w):
                    bad.append((f, t, lim, int((getattr(got, f) != w).sum())))
            if got.tick != t or got.info["entries"] != int(want["listed"].sum(dtype=np.int64)):
                bad.append(("info", t, lim, got.info))
    eng.close()
    orc.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
