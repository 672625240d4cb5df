#!/usr/bin/env python3
"""One rank of a multi-source reach run across ranks (tests/test_reach_multi_rccl.py launches it
under torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/reach_multi_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 4096, view 32, row shards

Every rank steps the engine 13 ticks and runs the CPU oracle on the same inputs.  The call is
collective: per level each rank ORs the share of the rows and columns it holds into its next
frontier, the frontiers are all-gathered over RCCL and ORed down, so EVERY rank's result at ticks
0, 12 and 13, in both directions, must equal the stack of numpy BFS over the oracle's rows
(tests/reach_multi_oracle.py): the five-id set at two age limits, the 64-id sample at one.
torch.distributed (gloo) carries only the RCCL id and the verdicts.  Rank 0 prints one JSON line;
exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANDOM = 1
TICKS, AT = 13, (0, 12, 13)
FEW = ((3, "few"), (32, "few"))                           # (age limit, source set)
# the 64-id sample where its numpy stack is short: the partial view's sparse graph at every tick,
# the full view (9e6 edges per BFS at limit 32) once, at limit 1: the entries refreshed at T
CASES = {True: {0: FEW + ((32, "sample"),), 12: FEW + ((3, "sample"),), 13: FEW + ((3, "sample"),)},
         False: {0: FEW[:1], 12: FEW, 13: FEW[:1] + ((1, "sample"),)}}
ARRAYS = ("hops", "seen", "reached", "ecc", "sum_hops", "level_sizes")


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine
    from tests import ranks_common
    from tests import reach_multi_oracle as rm
    from tests import reach_oracle as ro
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
    sets = {"few": rm.few(orc, n), "sample": [int(v) for v in rm.sample(n)]}
    bad = []
    for t in range(0, TICKS + 1):
        if t:
            orc.step()
            eng.step(1)
        if t not in AT:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        for lim, name in CASES[pview][t]:
            for dname, d in (("from", ro.FROM), ("to", ro.TO)):
                want = rm.expected(n, t, state, ro.graph(n, t, edges, lim, d), lim, d, sets[name])
                got = eng.reach_multi(sets[name], dname, lim)
                for a in ARRAYS:
                    if not np.array_equal(getattr(got, a), want[a]):
                        bad.append((a, t, lim, dname, name, int((getattr(got, a) != want[a]).sum())))
                if not np.array_equal(got.state, state):
                    bad.append(("state", t, lim, dname, name))
                if any(got.info[f] != want["info"][f] for f in rm.INFO):
                    bad.append(("info", t, lim, dname, name, got.info))
    eng.close()
    orc.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
