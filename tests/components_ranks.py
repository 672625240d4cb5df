#!/usr/bin/env python3
"""One rank of an overlay-components run across ranks (tests/test_components_rccl.py launches it
under torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/components_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, fanout 1, 2 column tiles per rank
  rows            full view, n = 3000, fanout 1, row shards
  pview_rows      partial view, the 2,048-node view-8 lattice with a crashed block, row shards

Every rank steps the engine and runs the CPU oracle on the same inputs.  The call is collective:
each rank sweeps its shards, the label arrays are all-reduced over RCCL (MIN / MAX) after every
sweep and the n-length kernels run on the reduced arrays, so EVERY rank's labels, state and info
of both kinds at the listed ticks must equal tests/components_oracle.py's over the oracle's rows.
torch.distributed (gloo) carries only the RCCL id and the verdicts.  Rank 0 prints one JSON line;
exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANDOM, BLOCK = 1, 2
# tick -> the age limits compared there: the fragmented ticks at limit 1, one whole overlay
AT = {True: {2: (1,), 3: (1, 32)}, False: {0: (32,), 10: (1,)}}


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine
    from tests import components_oracle as co
    from tests import ranks_common
    from tests import reach_oracle as ro
    from tests.oracle_binding import PviewOracle, ScaleOracle
    dist, rank, world, dev, uid = ranks_common.start()
    pview = case == "pview_rows"
    at = AT[pview]
    ticks = max(at)
    if pview:
        from gossip_protocol_amd.pview import PviewEngine
        n = 2048
        kw = dict(view=8, fanout=2, inbox=7, tremove=9, fail_mode=BLOCK, fail_tick=0, fail_ppm=100000, seed=77)
        orc = PviewOracle(n, **kw)
        eng = PviewEngine(n, max_ticks=ticks, device=dev, rank=rank, world=world, nccl_id=uid, **kw)
    else:
        n = 3000
        kw = dict(fanout=1, tremove=9, fail_mode=RANDOM, fail_tick=2, fail_ppm=20000, seed=3003)
        orc = ScaleOracle(n, **kw)
        eng = ScaleEngine(n, max_ticks=ticks, device=dev, rank=rank, world=world, nccl_id=uid,
                          tiles=2 if case == "columns_tiled" else 1,
                          layout="columns" if case == "columns_tiled" else "rows", **kw)
    bad = []
    for t in range(0, ticks + 1):
        if t:
            orc.step()
            eng.step(1)
        if t not in at:
            continue
        state = ro.states(orc, n, t)
        edges = ro.edges_at(orc, n, state, pview)
        for lim in at[t]:
            for name, kind in (("weak", co.WEAK), ("strong", co.STRONG)):
                want = co.expected(n, t, state, edges, lim, kind)
                got = eng.components(name, lim)
                if not np.array_equal(got.label, want["label"]):
                    bad.append(("label", t, lim, name, int((got.label != want["label"]).sum())))
                if not np.array_equal(got.state, state):
                    bad.append(("state", t, lim, name))
                if any(got.info[f] != want["info"][f] for f in co.INFO):
                    bad.append(("info", t, lim, name, got.info))
    eng.close()
    orc.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
