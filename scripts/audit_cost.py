#!/usr/bin/env python3
"""Cost of the view audit at the benchmark sizes, beside the census of the same engine at the
same tick (profiles/audit/).

    python scripts/audit_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 12]
    python scripts/audit_cost.py pview [--nodes 1048576] [--at 25 75]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU.
pview: config 5's workload (view 256, drain all) at each listed tick.
Each measurement: one warm-up call of each, then five audit and five census calls interleaved,
info.kernel_ms of every call, the medians, their ratio and the achieved rate by algorithmic
bytes (full: n * stride_total * 2 B; pview: the stored entries * 8 B).  One JSON line per
measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAIL_PPM, FAIL_TICK, FANOUT, PV_KW, SEED  # noqa: E402


def timed(eng, calls=5):
    """(last audit, audit ms list, census ms list), interleaved after one warm-up of each."""
    eng.audit()
    eng.census()
    aud, cen, a = [], [], None
    for _ in range(calls):
        a = eng.audit()
        aud.append(a.info["kernel_ms"])
        cen.append(eng.census().info["kernel_ms"])
    return a, aud, cen


def report(what, a, aud, cen, nbytes, **extra):
    am, cm = float(np.median(aud)), float(np.median(cen))
    s = a.summary()
    s["mean_age"] = round(s["mean_age"], 4)
    print(json.dumps(dict(extra, what=what, tick=a.tick, audit_ms=aud, census_ms=cen,
                          audit_median_ms=am, census_median_ms=cm, ratio=am / cm if cm else None,
                          bytes=nbytes, audit_tb_per_s=nbytes / (am * 1e-3) / 1e12 if am else None,
                          census_tb_per_s=nbytes / (cm * 1e-3) / 1e12 if cm else None,
                          summary=s)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["full", "pview"])
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--at", type=int, nargs="+", default=[25, 75])
    args = ap.parse_args()
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n = args.nodes or 65536
        with ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                         fail_ppm=FAIL_PPM, seed=SEED, max_ticks=args.ticks, group=args.tiles) as eng:
            eng.step(args.ticks)
            shards, _, stride = eng.layout()
            a, aud, cen = timed(eng)
            report("full", a, aud, cen, n * stride * shards * 2, n=n, tiles=shards)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n = args.nodes or (1 << 20)
    last = max(args.at)
    with PviewEngine(n, max_ticks=last, **PV_KW) as eng:
        for t in range(1, last + 1):
            eng.step(1)
            if t in args.at:
                a, aud, cen = timed(eng)
                report("pview", a, aud, cen, int(a.info["entries"]) * 8, n=n, view=PV_KW["view"])


if __name__ == "__main__":
    main()
