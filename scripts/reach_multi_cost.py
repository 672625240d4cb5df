#!/usr/bin/env python3
"""Cost of multi-source reach at the benchmark sizes, beside the 64 single-source reach() calls it
replaces and the census of the same engine at the same tick (profiles/reach_multi/).

    python scripts/reach_multi_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 12]
    python scripts/reach_multi_cost.py pview [--nodes 1048576] [--at 25 75]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU.
pview: config 5's workload (view 256, drain all), at each listed tick.
Sources: 64 ids spread over [0, n) (0, n - 1 and multiples of 2654435761 mod n).  Per tick and
direction, info.kernel_ms and the wall time of 5 reach_multi() calls after one warm-up call, with
hops left out and with hops wanted; levels, depth, pairs and the spread of the reach sets; then
the two yardsticks measured on the same engine at the same tick: the 64 reach() calls of the same
sources (kernel_ms and wall time, summed over one pass), whose hops rows the multi-source call
must equal, and the census's kernel_ms over 5 calls.
One JSON line per measurement, also appended to --out (default
profiles/reach_multi/reach_multi_cost.jsonl).
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


def sample(n):
    return [int(v) for v in np.unique(np.r_[0, n - 1, np.arange(62) * 2654435761 % n])[:64]]


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return r, (time.perf_counter() - t0) * 1e3


def measure(eng, base, out, calls=5):
    src = sample(eng.n)
    eng.census()
    census_ms = [eng.census().info["kernel_ms"] for _ in range(calls)]
    for direction in ("from", "to"):
        line = dict(base, direction=direction, sources=len(src), census_kernel_ms=census_ms,
                    census_median_ms=float(np.median(census_ms)))
        for key, hops in (("nohops", False), ("hops", True)):
            eng.reach_multi(src, direction, hops=hops)
            runs = [timed(lambda: eng.reach_multi(src, direction, hops=hops)) for _ in range(calls)]
            r = runs[-1][0]
            assert all(np.array_equal(x.seen, r.seen) for x, _ in runs)
            line[key + "_kernel_ms"] = [x.info["kernel_ms"] for x, _ in runs]
            line[key + "_wall_ms"] = [round(w, 3) for _, w in runs]
            line[key + "_median_ms"] = float(np.median(line[key + "_kernel_ms"]))
        s = r.summary()
        line.update(age_limit=r.info["age_limit"], levels=r.info["levels"], depth=r.info["depth"],
                    alive=r.info["alive"], alive_sources=r.info["alive_sources"], pairs=r.info["pairs"],
                    mean_hops=s["mean_hops"], reached_min=s["reached_min"], reached_max=s["reached_max"],
                    distinct_sets=s["distinct_sets"])
        eng.reach(src[0], direction)
        single = [timed(lambda b=b: eng.reach(b, direction)) for b in src]
        assert all(np.array_equal(x.hops, r.hops[i]) for i, (x, _) in enumerate(single))
        line.update(single_kernel_ms_sum=float(sum(x.info["kernel_ms"] for x, _ in single)),
                    single_wall_ms_sum=round(sum(w for _, w in single), 3),
                    single_kernel_ms_min=float(min(x.info["kernel_ms"] for x, _ in single)),
                    single_kernel_ms_max=float(max(x.info["kernel_ms"] for x, _ in single)),
                    single_levels_sum=int(sum(x.info["levels"] for x, _ in single)))
        line["speedup_nohops"] = round(line["single_kernel_ms_sum"] / line["nohops_median_ms"], 2)
        line["speedup_hops"] = round(line["single_kernel_ms_sum"] / line["hops_median_ms"], 2)
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
    ap.add_argument("--at", type=int, nargs="+", default=[25, 75])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_multi", "reach_multi_cost.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n = args.nodes or 65536
        with ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                         fail_ppm=FAIL_PPM, seed=SEED, max_ticks=args.ticks, group=args.tiles) as eng:
            eng.step(args.ticks)
            measure(eng, {"what": "full", "n": n, "tiles": eng.layout()[0], "tick": args.ticks}, args.out)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n = args.nodes or (1 << 20)
    last = max(args.at)
    with PviewEngine(n, max_ticks=last, **PV_KW) as eng:
        for t in range(1, last + 1):
            eng.step(1)
            if t in args.at:
                measure(eng, {"what": "pview", "n": n, "view": PV_KW["view"], "tick": t}, args.out)


if __name__ == "__main__":
    main()
