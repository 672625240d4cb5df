#!/usr/bin/env python3
"""Cost of the membership census at the benchmark sizes (profiles/census/).

    python scripts/census_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 12]
    python scripts/census_cost.py pview [--nodes 1048576] [--at 25 75]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU; info.kernel_ms over 5
       calls after one warm-up call, and the achieved rate n * stride_total * 2 B / time.
pview: config 5's workload (view 256, drain all); at each listed tick both kernel forms
       (GSP_TEST_PV_CENSUS=0 plain, 1 LDS-privatised), 5 calls each after one warm-up, and a check
       that the two forms return the same arrays.
One JSON line per measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAIL_PPM, FAIL_TICK, FANOUT, PV_KW, SEED  # noqa: E402


def timed(eng, age_limit=None, calls=5):
    eng.census(age_limit)
    runs = [eng.census(age_limit) for _ in range(calls)]
    return runs[-1], [r.info["kernel_ms"] for r in runs]


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
            c, ms = timed(eng)
            nbytes = n * stride * shards * 2
            print(json.dumps({"what": "full", "n": n, "tiles": shards, "tick": c.tick,
                              "kernel_ms": ms, "median_ms": float(np.median(ms)),
                              "table_bytes": nbytes,
                              "tb_per_s": nbytes / (float(np.median(ms)) * 1e-3) / 1e12,
                              "summary": c.summary()}), flush=True)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n = args.nodes or (1 << 20)
    last = max(args.at)
    with PviewEngine(n, max_ticks=last, **PV_KW) as eng:
        for t in range(1, last + 1):
            eng.step(1)
            if t not in args.at:
                continue
            got = {}
            for form in ("0", "1"):
                os.environ["GSP_TEST_PV_CENSUS"] = form
                got[form], ms = timed(eng)
                print(json.dumps({"what": "pview", "n": n, "view": PV_KW["view"], "tick": t,
                                  "form": "plain" if form == "0" else "lds", "kernel_ms": ms,
                                  "median_ms": float(np.median(ms)),
                                  "summary": got[form].summary()}), flush=True)
            same = all(np.array_equal(getattr(got["0"], f), getattr(got["1"], f))
                       for f in ("listed", "fresh", "max_hb", "state"))
            print(json.dumps({"what": "pview", "tick": t, "forms_agree": bool(same)}), flush=True)
            assert same
    os.environ.pop("GSP_TEST_PV_CENSUS", None)


if __name__ == "__main__":
    main()
