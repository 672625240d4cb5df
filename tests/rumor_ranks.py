#!/usr/bin/env python3
"""One rank of a rumor-trace run across ranks (tests/test_rumor_rccl.py launches it under
torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/rumor_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 4096, view 32, inbox 7, row shards

Every rank steps the engine 13 ticks with a trace of three rumors (node 0 at tick 0, node n - 1
at tick 0, and at tick 6 a set with a duplicate and a crashed node) and runs the CPU oracle on the
same inputs.  Open, seed, get and close are collective: with column shards every rank computes
the whole map from the CSR it holds, row shards all-reduce know every tick (MAX) and heard /
known at a get (MIN / SUM), so EVERY rank's result at ticks 0, 6, 12 and 13 must equal the numpy
rule over the oracle's messages (tests/rumor_oracle.py).  torch.distributed (gloo) carries only
the RCCL id and the verdicts.  Rank 0 prints one JSON line; exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANDOM = 1
TICKS, AT, RUMORS, MID = 13, (0, 6, 12, 13), 3, 6
FIELDS = ("tick", "n", "rumor", "seed_tick", "sources", "alive", "known", "known_alive",
          "last_heard", "ticks_traced")


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine
    from tests import ranks_common
    from tests import rumor_oracle as ru
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
    start, fail = ru.schedule(orc, n)
    dead = int(np.nonzero(fail < MID)[0][0])
    seeds = {0: [(0, [0]), (1, [n - 1])], MID: [(2, [n // 3, dead, n // 3, n // 2])]}
    ref = ru.run(orc, n, TICKS, kw.get("inbox", 0), RUMORS, seeds, set(AT))
    orc.close()
    bad = []
    eng.rumor_open(RUMORS)
    for t in range(0, TICKS + 1):
        if t:
            eng.step(1)
        for rumor, sources in seeds.get(t, ()):
            eng.rumor_seed(rumor, sources)
        if t not in AT:
            continue
        for b in range(RUMORS):
            heard, state, known, info = ref["at"][t][b]
            for again in range(2):                   # a get leaves the device state alone
                got = eng.rumor(b)
                if not np.array_equal(got.heard, heard):
                    bad.append(("heard", t, b, again, int((got.heard != heard).sum())))
                if not np.array_equal(got.known, known):
                    bad.append(("known", t, b, again, got.known.tolist(), known.tolist()))
                if not np.array_equal(got.state, state):
                    bad.append(("state", t, b, again))
                if any(got.info[f] != info[f] for f in FIELDS):
                    bad.append(("info", t, b, again, got.info))
    eng.rumor_close()
    eng.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
