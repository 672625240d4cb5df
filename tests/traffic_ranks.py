#!/usr/bin/env python3
"""One rank of a traffic-ledger run across ranks (tests/test_traffic_rccl.py launches it under
torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/traffic_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 1200, view 32, inbox 3, a join schedule, row shards
  pview_tfail     partial view, n = 1024, view 32, inbox 3, TFAIL 4, row shards (the sizing pass)

Every rank steps the engine 20 ticks with a ledger opened at tick 0 and runs the CPU oracle on the
same inputs.  Column ranks each count the whole job from the one CSR; row ranks count their own
rows and a get all-reduces the buffers (SUM; MAX for the peaks) into staging, so EVERY rank's
result at ticks 0, 12 and 20 -- each read twice -- must equal the numpy rule over the oracle
(tests/traffic_oracle.py).  torch.distributed (gloo) carries only the RCCL id and the verdicts.
Rank 0 prints one JSON line; exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TICKS, AT = 20, (0, 12, 20)
CASES = {"columns_tiled": ("full", "main"), "rows": ("full", "main"), "pview_rows": ("pview", "join"),
         "pview_tfail": ("pview", "tfail")}


def run(case):
    from gossip_protocol_amd import traffic
    from gossip_protocol_amd.scale import ScaleEngine, make_policy
    from tests import ranks_common
    from tests import traffic_oracle as to
    dist, rank, world, dev, uid = ranks_common.start()
    kind, name = CASES[case]
    w = to.WORKLOADS[kind, name]
    pol = make_policy(**w["pol"]) if w["pol"] else None
    if kind == "pview":
        from gossip_protocol_amd.pview import PviewEngine
        eng = PviewEngine(w["n"], max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          policy=pol, **w["kw"])
    else:
        eng = ScaleEngine(w["n"], max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          tiles=2 if case == "columns_tiled" else 1,
                          layout="columns" if case == "columns_tiled" else "rows", policy=pol, **w["kw"])
    orc = to.make_oracle(kind, name)
    ref = to.run(orc, kind, w["n"], TICKS, w["kw"].get("inbox", 0), w["kw"].get("tfail", 0),
                 (w["pol"] or {}).get("intro_list", 0), set(AT), 0, to.watch_of(w))
    orc.close()
    bad = []
    eng.traffic_open(to.watch_of(w))
    for t in range(0, TICKS + 1):
        if t:
            eng.step(1)
        if t not in AT:
            continue
        want = ref["at"][t]
        for again in range(2):                       # a get leaves the device state alone
            got = eng.traffic()
            for a in traffic.ARRAYS + ("state", "by_tick", "fanin", "watch"):
                g = getattr(got, a).astype(np.int64)
                if g.shape != want[a].shape or not np.array_equal(g, want[a]):
                    bad.append((a, t, again))
            if any(got.info[f] != want["info"][f] for f in to.INFO):
                bad.append(("info", t, again, got.info))
    eng.traffic_close()
    eng.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
