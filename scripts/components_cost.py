#!/usr/bin/env python3
"""Cost of overlay components at the benchmark sizes, beside the census of the same engine at the
same tick (profiles/components/).

    python scripts/components_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 12] [--limits 1 0]
    python scripts/components_cost.py pview [--nodes 1048576] [--at 25 75]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU, at the listed age limits
       (0: the default, tremove).
pview: config 5's workload (view 256, drain all), at each listed tick, at the default limit.
Per measurement and kind ("weak", "strong"): info.kernel_ms and the wall time of 3 components()
calls after one warm-up call, their median and range, the sweeps and rounds the call made and its
summary; then the yardstick measured on the same engine at the same tick and limit: the census's
kernel_ms over 5 calls after one warm-up, and sweeps x that.  One JSON line per measurement, also
appended to --out (default profiles/components/components_cost.jsonl).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAIL_PPM, FAIL_TICK, FANOUT, PV_KW, SEED  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t0) * 1e3


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def measure(eng, base, limit, out, calls=3):
    eng.census(limit)
    census_ms = [eng.census(limit).info["kernel_ms"] for _ in range(5)]
    census = float(np.median(census_ms))
    for kind in ("weak", "strong"):
        eng.components(kind, limit)
        runs = [timed(lambda: eng.components(kind, limit)) for _ in range(calls)]
        r = runs[-1][0]
        assert all(x.converged and np.array_equal(x.label, r.label) for x, _ in runs)
        ms = [x.info["kernel_ms"] for x, _ in runs]
        s = r.summary()
        line = dict(base, kind=kind, age_limit=r.info["age_limit"], alive=r.info["alive"],
                    sweeps=[x.info["sweeps"] for x, _ in runs], rounds=[x.info["rounds"] for x, _ in runs],
                    kernel_ms=ms, wall_ms=[round(w, 3) for _, w in runs], components_ms=spread(ms),
                    census_kernel_ms=census_ms, census=spread(census_ms),
                    sweeps_x_census=round(r.info["sweeps"] * census, 3),
                    components_over_yardstick=round(float(np.median(ms)) / (r.info["sweeps"] * census), 3),
                    components=s["components"], giant=s["giant"], singletons=s["singletons"],
                    nontrivial=s["nontrivial"], histogram=s["histogram"])
        text = json.dumps(line)
        print(text, flush=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["full", "pview"])
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--limits", type=int, nargs="+", default=[1, 0])
    ap.add_argument("--at", type=int, nargs="+", default=[25, 75])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components", "components_cost.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n = args.nodes or 65536
        with ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                         fail_ppm=FAIL_PPM, seed=SEED, max_ticks=args.ticks, group=args.tiles) as eng:
            eng.step(args.ticks)
            for lim in args.limits:
                measure(eng, {"what": "full", "n": n, "tiles": eng.layout()[0], "tick": args.ticks},
                        lim or None, args.out)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n = args.nodes or (1 << 20)
    last = max(args.at)
    with PviewEngine(n, max_ticks=last, **PV_KW) as eng:
        for t in range(1, last + 1):
            eng.step(1)
            if t in args.at:
                measure(eng, {"what": "pview", "n": n, "view": PV_KW["view"], "tick": t}, None, args.out)


if __name__ == "__main__":
    main()
