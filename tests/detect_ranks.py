#!/usr/bin/env python3
"""One rank of a detection-ledger run across ranks (tests/test_detect_rccl.py launches it under
torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/detect_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 1200, view 32, inbox 3, a join schedule, row shards

Every rank steps the engine 20 ticks with a ledger opened at tick 0 and runs the CPU oracle on the
same inputs.  Each rank folds the records its own shards made; get and close are collective, and a
get all-reduces the arrays (MIN / MAX / SUM) into a staging buffer, so EVERY rank's result at ticks
0, 12 and 20 -- each read twice -- must equal the numpy rule over the oracle's events
(tests/detect_oracle.py).  torch.distributed (gloo) carries only the RCCL id and the verdicts.
Rank 0 prints one JSON line; exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANDOM = 1
TICKS, AT = 20, (0, 12, 20)


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine, make_policy
    from tests import ranks_common
    from tests import detect_oracle as do
    from tests.oracle_binding import PviewOracle, ScaleOracle
    from tests.oracle_binding import make_policy as oracle_policy
    dist, rank, world, dev, uid = ranks_common.start()
    if case == "pview_rows":
        from gossip_protocol_amd.pview import PviewEngine
        n = 1200
        pol = dict(step_rate=0.02, intro_list=8)
        kw = dict(view=32, fanout=3, inbox=3, tremove=9, fail_mode=RANDOM, fail_tick=10, fail_ppm=30000,
                  seed=77)
        orc = PviewOracle(n, policy=oracle_policy(**pol), **kw)
        eng = PviewEngine(n, max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          events=True, event_cap=1 << 20, policy=make_policy(**pol), **kw)
    else:
        n = 3000
        kw = dict(fanout=3, tremove=9, fail_mode=RANDOM, fail_tick=2, fail_ppm=20000, seed=3003)
        orc = ScaleOracle(n, **kw)
        eng = ScaleEngine(n, max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          events=True, event_cap=1 << 20,
                          tiles=2 if case == "columns_tiled" else 1,
                          layout="columns" if case == "columns_tiled" else "rows", **kw)
    ref = do.run(orc, n, TICKS, set(AT), keep_r=False)
    orc.close()
    bad = []
    eng.detect_open()
    for t in range(0, TICKS + 1):
        if t:
            eng.step(1)
        if t not in AT:
            continue
        want = ref["at"][t]
        for again in range(2):                       # a get leaves the device state alone
            got = eng.detect()
            for a in do.ARRAYS + ("state", "by_tick"):
                if not np.array_equal(getattr(got, a), want[a]):
                    bad.append((a, t, again, int((getattr(got, a) != want[a]).sum())))
            if any(got.info[f] != want["info"][f] for f in do.INFO):
                bad.append(("info", t, again, got.info))
    eng.detect_close()
    eng.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
