#!/usr/bin/env python3
"""The failure-detection curve of a .conf run, from the detection ledger: the companion of
census_curve.py.

    python scripts/detect_curve.py CONF [--pview] [--every K] [--ticks N] [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview; the engine
records every event kind) with a ledger opened at tick 0 and prints one JSON line per sampled tick
(every K-th tick and the last one): Detect.summary() -- crashed and detected nodes, removes per
detected node, first / full detection latency, false removes, revivals -- plus the ledger's record
totals and, from the census of that tick, `crashed_unlisted`: the crashed members no live node
lists any more (listed == 0).  That is "fully detected" read from the state itself, next to the
ledger's reading of it from the records.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("conf")
    ap.add_argument("--pview", action="store_true", help="the partial-view engine (VIEW / INBOX keys)")
    ap.add_argument("--every", type=int, default=10, help="sample every K-th tick")
    ap.add_argument("--ticks", type=int, default=None, help="stop after N ticks (default: the .conf's)")
    ap.add_argument("--group", type=int, default=1, help="in-process column tiles / row shards")
    args = ap.parse_args()
    if args.pview:
        from gossip_protocol_amd.pview import PviewEngine as Engine
        from gossip_protocol_amd.pview import params_from_conf
    else:
        from gossip_protocol_amd.scale import ScaleEngine as Engine
        from gossip_protocol_amd.scale import params_from_conf
    from gossip_protocol_amd.census import CRASHED
    params = params_from_conf(args.conf)
    params.events = 1
    ticks = min(args.ticks, params.max_ticks) if args.ticks is not None else params.max_ticks
    every = max(1, args.every)
    with Engine(params.n, params=params, group=args.group) as eng:
        eng.detect_open()
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
            if t % every and t != ticks:
                continue
            d, c = eng.detect(), eng.census()
            crashed = c.state == CRASHED
            line = d.summary()
            line.update(crashed_unlisted=int((c.listed[crashed] == 0).sum()),
                        records=d.info["records"], true_removes=d.info["true_removes"],
                        false_removes=d.info["false_removes"], evicts=d.info["evicts"],
                        fold_ms=round(d.info["kernel_ms"], 4))
            print(json.dumps(line), flush=True)
        eng.detect_close()


if __name__ == "__main__":
    main()
