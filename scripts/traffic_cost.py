#!/usr/bin/env python3
"""Cost of an open traffic ledger at the benchmark sizes (profiles/traffic/).

    python scripts/traffic_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 45]
    python scripts/traffic_cost.py pview [--nodes 1048576] [--ticks 35] [--inbox 0] [--tfail 0]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU.
pview: config 5's workload (view 256; --inbox 0 drains all, --inbox 7 is the bounded inbox;
       --tfail 4 adds the payload sizing pass).
The engine is stepped 5 ticks; the window is ticks 6..--ticks.  Three runs of the same window: the
ledger closed, and the ledger open with each form of the sender side (one lane per sender over the
send slots; one atomic per message of the next tick's receiver CSR, the last tick folded at get),
with 1,024 watched nodes.  Per run: wall time per tick over the window (one step call, then a sync),
the tick kernels' time per tick (gsp_scale_perf merge_ms), and for an open ledger its kernel_ms
per tick, its share of the tick kernels, the totals and Traffic.summary().  One JSON line per run,
also appended to --out (default profiles/traffic/traffic_cost.jsonl).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAIL_PPM, FAIL_TICK, FANOUT, PV_KW, SEED  # noqa: E402

WARMUP = 5
MODES = (("closed", None), ("open_slots", "0"), ("open_csr", "1"))


def measure(make, n, ticks, base, out):
    watch = list(range(0, n, max(1, n // 1024)))[:1024]
    for mode, form in MODES:
        with make() as eng:
            eng.step(WARMUP)
            if form is not None:
                os.environ["GSP_TEST_TRAFFIC_FORM"] = form
                eng.traffic_open(watch)
            eng.sync()
            p0 = eng.perf()
            t0 = time.perf_counter()
            eng.step(ticks - WARMUP)
            eng.sync()
            el = time.perf_counter() - t0
            p1 = eng.perf()
            w = ticks - WARMUP
            tick_ms = p1["merge_ms"] - p0["merge_ms"]
            line = dict(base, mode=mode, window=[WARMUP + 1, ticks], wall_ms_per_tick=el * 1e3 / w,
                        tick_kernels_ms_per_tick=tick_ms / w)
            if form is not None:
                d = eng.traffic()
                line.update(ledger_ms_per_tick=d.info["kernel_ms"] / w,
                            ledger_share_of_tick_kernels=d.info["kernel_ms"] / tick_ms,
                            **{k: d.info[k] for k in ("sent", "recv", "merged", "lost", "entries", "overflow",
                                                      "max_fanin", "max_fanin_node")},
                            summary=d.summary())
                eng.traffic_close()
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
    ap.add_argument("--inbox", type=int, default=0, help="partial view: 0 drains all, 1..7 bounded")
    ap.add_argument("--tfail", type=int, default=0, help="partial view: TFAIL (the sizing pass runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic", "traffic_cost.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n, ticks = args.nodes or 65536, args.ticks or 45
        make = lambda: ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                                   fail_ppm=FAIL_PPM, seed=SEED, max_ticks=ticks, group=args.tiles)
        measure(make, n, ticks, {"what": "full", "n": n, "tiles": args.tiles}, args.out)
        return
    from gossip_protocol_amd.pview import PviewEngine
    n, ticks = args.nodes or (1 << 20), args.ticks or 35
    kw = dict(PV_KW, inbox=args.inbox, tfail=args.tfail)
    make = lambda: PviewEngine(n, max_ticks=ticks, **kw)
    measure(make, n, ticks, {"what": "pview", "n": n, "view": kw["view"], "inbox": args.inbox,
                             "tfail": args.tfail}, args.out)


if __name__ == "__main__":
    main()
