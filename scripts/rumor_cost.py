#!/usr/bin/env python3
"""Cost of an open rumor trace at the benchmark sizes, and what it shows there (DESIGN.md 4g;
profiles/rumor/).

    python scripts/rumor_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 40]
    python scripts/rumor_cost.py pview [--nodes 1048576] [--ticks 80]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU.
pview: config 5's workload (view 256, drain all).
A trace of 32 rumors is opened at tick 0: rumor 0 at node 0, rumor 31 at node n - 1, the others
at evenly spaced ids.  Per tick the trace's kernel_ms (HIP events around the trace launches) is
read next to the same run's tick-kernel time (gsp_scale_perf merge_ms); the line names the mean,
the median and the slowest tick of both.  Then, for node 0 and the high id: ticks to 50 % / 99 % /
full coverage of the nodes alive at the end and the live nodes never reached, beside reach's depth
and unreached count at the seed tick.  One JSON line, also appended to --out (default
profiles/rumor/rumor_cost.jsonl).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAIL_PPM, FAIL_TICK, FANOUT, PV_KW, SEED  # noqa: E402


def measure(eng, n, ticks, base, out):
    eng.rumor_open(32)
    sources = [0] + [b * (n // 31) for b in range(1, 31)] + [n - 1]
    reach = {}
    for b, s in enumerate(sources):
        eng.rumor_seed(b, s)
        if b in (0, 31):
            reach[b] = eng.reach(s, "from").summary()
    trace, tick = [], []
    p0, k0 = eng.perf(), 0.0
    for _ in range(ticks):
        eng.step(1)
        p1 = eng.perf()                              # synchronises: the tick's events are in
        k1 = eng.rumor(0).info["kernel_ms"]
        trace.append(k1 - k0)
        tick.append(p1["merge_ms"] - p0["merge_ms"])
        p0, k0 = p1, k1
    trace, tick = np.array(trace), np.array(tick)
    worst = int(trace.argmax())
    line = dict(base, rumors=32, ticks=ticks,
                trace_ms_mean=float(trace.mean()), trace_ms_median=float(np.median(trace)),
                tick_ms_mean=float(tick.mean()), tick_ms_median=float(np.median(tick)),
                trace_share_of_tick=float(trace.sum() / tick.sum()),
                slowest_trace_tick=worst + 1, slowest_trace_ms=float(trace[worst]),
                tick_ms_there=float(tick[worst]),
                trace_ms_per_tick=[round(float(v), 5) for v in trace])
    for b in (0, 31):
        r = eng.rumor(b)
        line["source_%d" % sources[b]] = dict(
            ticks_to_50=r.ticks_to(0.5), ticks_to_99=r.ticks_to(0.99), ticks_to_full=r.ticks_to(1.0),
            unknown_alive=r.summary()["unknown_alive"], alive=r.info["alive"],
            reach_depth_at_seed=reach[b]["depth"], reach_unreached_at_seed=reach[b]["unreached"])
    eng.rumor_close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["full", "pview"])
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--tiles", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rumor", "rumor_cost.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n, ticks = args.nodes or 65536, args.ticks or 40
        with ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                         fail_ppm=FAIL_PPM, seed=SEED, max_ticks=ticks, group=args.tiles) as eng:
            measure(eng, n, ticks, {"what": "full", "n": n, "tiles": eng.layout()[0]}, args.out)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n, ticks = args.nodes or (1 << 20), args.ticks or 80
    with PviewEngine(n, max_ticks=ticks, **PV_KW) as eng:
        measure(eng, n, ticks, {"what": "pview", "n": n, "view": PV_KW["view"], "inbox": PV_KW["inbox"]},
                args.out)


if __name__ == "__main__":
    main()
