#!/usr/bin/env python3
"""Cost of an open detection ledger at the benchmark sizes (profiles/detect/).

    python scripts/detect_cost.py full  [--nodes 65536] [--tiles 8] [--ticks 45] [--cap 0]
    python scripts/detect_cost.py pview [--nodes 1048576] [--ticks 35] [--cap 0]

full:  config 3's workload (bench.py's rules) as column tiles on one GPU, events on.
pview: config 5's workload (view 256, drain all), events on.
The engine is stepped 5 ticks and its ring drained; the window is ticks 6..--ticks.  Three runs of
the same window: the ledger closed (the ring fills, and is drained once by the host at the end: the
records it kept and lost are reported), and the ledger open with each form of the fold (plain global
atomics, LDS-aggregated).  Per run: wall time per tick over the window (one step call, then a
sync), the tick kernels' time per tick (gsp_scale_perf merge_ms), and for an open ledger its
kernel_ms per tick, records, lost, the totals and busiest_tick_records (the most records of one
tick that fall in one of by_tick's four classes; joins of live members are in none).  --cap is event_cap (0: the default ring of 2^24
records).  One JSON line per run, also appended to --out (default
profiles/detect/detect_cost.jsonl).
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
MODES = (("closed", None), ("open_plain", "0"), ("open_lds", "1"))


def measure(make, ticks, base, out):
    for mode, form in MODES:
        with make() as eng:
            eng.step(WARMUP)
            eng.drain_events()
            if form is not None:
                os.environ["GSP_TEST_DETECT_FORM"] = form
                eng.detect_open()
            eng.sync()
            p0 = eng.perf()
            t0 = time.perf_counter()
            eng.step(ticks - WARMUP)
            eng.sync()
            el = time.perf_counter() - t0
            p1 = eng.perf()
            w = ticks - WARMUP
            line = dict(base, mode=mode, window=[WARMUP + 1, ticks], wall_ms_per_tick=el * 1e3 / w,
                        tick_kernels_ms_per_tick=(p1["merge_ms"] - p0["merge_ms"]) / w)
            if form is None:
                rec, lost = eng.drain_events()
                line.update(host_drained_records=int(len(rec)), host_drained_lost=int(lost))
            else:
                d = eng.detect()
                line.update(fold_ms_per_tick=d.info["kernel_ms"] / w,
                            fold_share_of_tick_kernels=d.info["kernel_ms"] / (p1["merge_ms"] - p0["merge_ms"]),
                            **{k: d.info[k] for k in ("records", "lost", "true_removes", "false_removes",
                                                      "joins", "revivals", "evicts")},
                            busiest_tick_records=int(d.by_tick.sum(axis=1).max()),
                            summary=d.summary())
                eng.detect_close()
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
    ap.add_argument("--cap", type=int, default=0, help="event_cap (0: the default ring)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect", "detect_cost.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.what == "full":
        from gossip_protocol_amd.scale import FAIL_RANDOM, ScaleEngine
        n, ticks = args.nodes or 65536, args.ticks or 45
        make = lambda: ScaleEngine(n, fanout=FANOUT, fail_mode=FAIL_RANDOM, fail_tick=FAIL_TICK,
                                   fail_ppm=FAIL_PPM, seed=SEED, max_ticks=ticks, group=args.tiles,
                                   events=True, event_cap=args.cap)
        measure(make, ticks, {"what": "full", "n": n, "tiles": args.tiles, "event_cap": args.cap}, args.out)
        return
    from gossip_protocol_amd import _lib
    from gossip_protocol_amd.pview import PviewEngine
    n, ticks = args.nodes or (1 << 20), args.ticks or 35
    # removes only, as bench.py's config-5 event item records them
    make = lambda: PviewEngine(n, max_ticks=ticks, events=_lib.EVENTS_REMOVE, event_cap=args.cap, **PV_KW)
    measure(make, ticks, {"what": "pview", "n": n, "view": PV_KW["view"], "inbox": PV_KW["inbox"],
                          "events": "removes", "event_cap": args.cap}, args.out)


if __name__ == "__main__":
    main()
