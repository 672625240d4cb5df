#!/usr/bin/env python3
"""One rank of a view audit across ranks (tests/test_audit_rccl.py launches it under
torch.distributed.run, one fresh process per GPU, no GPU call before it starts).

    python -m torch.distributed.run --nproc-per-node N tests/audit_ranks.py <case>

cases:
  columns_tiled   full view, n = 3000, 2 column tiles per rank
  rows            full view, n = 3000, row shards
  pview_rows      partial view, n = 4096, view 32, row shards

Every rank steps the engine 13 ticks and runs the CPU oracle on the same inputs
(tests/audit_oracle.py).  The audit is collective: each rank audits the rows and columns it holds
and the arrays are all-reduced over RCCL (SUM for the counts and the wrapping print, MAX for
age_max), so EVERY rank's audit at ticks 0, 12 and 13 must equal the one numpy makes from the
oracle's rows.  torch.distributed (gloo) carries only the RCCL id and the verdicts.  Rank 0
prints one JSON line; exit status 0 means parity.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TICKS, AT, LIMITS = 13, (0, 12, 13), (3, 9)


def run(case):
    from gossip_protocol_amd.scale import ScaleEngine
    from tests import ranks_common
    from tests import audit_oracle as ao
    dist, rank, world, dev, uid = ranks_common.start()
    if case == "pview_rows":
        from gossip_protocol_amd.pview import PviewEngine
        w, ref = ao.PVIEW["A"], ao.pview_reference("A", TICKS, AT)
        eng = PviewEngine(w["n"], max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          **w["kw"])
    else:
        w, ref = ao.FULL["main"], ao.full_reference("main", TICKS, AT)
        eng = ScaleEngine(w["n"], max_ticks=TICKS, device=dev, rank=rank, world=world, nccl_id=uid,
                          tiles=2 if case == "columns_tiled" else 1,
                          layout="columns" if case == "columns_tiled" else "rows", **w["kw"])
    bad = []
    for t in range(0, TICKS + 1):
        if t:
            eng.step(1)
        if t not in AT:
            continue
        want = ref["audit"][t]
        for lim in LIMITS:
            got = eng.audit(lim)
            bad += [(f, t, lim, cnt) for f, cnt in ao.mismatches(got, want, lim)]
            if got.tick != t or got.info["entries"] != int(want["size"].sum(dtype=np.int64)):
                bad.append(("info", t, lim, got.info))
    eng.close()
    return ranks_common.finish(dist, case, rank, world, bad)


if __name__ == "__main__":
    sys.exit(run(sys.argv[1]))
