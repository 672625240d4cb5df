#!/usr/bin/env python3
"""The convergence / completeness / accuracy curve of a .conf run, from the membership census.

    python scripts/census_curve.py CONF [--pview] [--every K] [--ticks T] [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview) and
prints one JSON line per sampled tick (tick 0, every K-th tick and the last one) with
Census.summary(): alive, crashed, undetected and stale_pairs (completeness: both reach 0 once
every crashed node has been removed by everyone), orphans and missing_pairs (accuracy and
convergence), max_listed, and the census kernels' ms.  No event stream is needed.
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
    ap.add_argument("--ticks", type=int, default=None, help="stop after T ticks (default: the .conf's)")
    ap.add_argument("--group", type=int, default=1, help="in-process column tiles / row shards")
    args = ap.parse_args()
    if args.pview:
        from gossip_protocol_amd.pview import PviewEngine as Engine
        from gossip_protocol_amd.pview import params_from_conf
    else:
        from gossip_protocol_amd.scale import ScaleEngine as Engine
        from gossip_protocol_amd.scale import params_from_conf
    params = params_from_conf(args.conf)
    ticks = min(args.ticks, params.max_ticks) if args.ticks is not None else params.max_ticks
    every = max(1, args.every)
    with Engine(params.n, params=params, group=args.group) as eng:
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
            if t % every == 0 or t == ticks:
                c = eng.census()
                print(json.dumps(dict(c.summary(), age_limit=c.info["age_limit"],
                                      entries=c.info["entries"],
                                      kernel_ms=round(c.info["kernel_ms"], 4))), flush=True)


if __name__ == "__main__":
    main()
