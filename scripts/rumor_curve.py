#!/usr/bin/env python3
"""The dissemination curve of a .conf run, from the rumor trace: the companion of reach_curve.py.

    python scripts/rumor_curve.py CONF [--pview] [--source S ...] [--at T] [--every K]
                                       [--ticks N] [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview), opens a
trace at tick T (default 0) with one rumor per source S (default: node 0; up to 32) and prints one
JSON line per sampled tick (every K-th tick and the last one): per rumor the share of the nodes
alive at that tick that have heard it.  The last line gives, per source, the ticks from the seed
to 50 % / 99 % / full coverage of the nodes alive at the end and the live nodes never reached,
next to reach(S, "from") taken at the seed tick: its depth (a bound on the ticks only while the
graph stands still) and its unreached count.  The two are printed side by side and no ordering
is asserted: the graph changes while the rumor travels.
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
    ap.add_argument("--source", type=int, nargs="+", default=[0], help="one rumor per node S")
    ap.add_argument("--at", type=int, default=0, help="the seed tick T")
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
    params = params_from_conf(args.conf)
    ticks = min(args.ticks, params.max_ticks) if args.ticks is not None else params.max_ticks
    every = max(1, args.every)
    sources = args.source[:32]
    if not 0 <= args.at <= ticks:
        ap.error("--at %d outside [0, %d]" % (args.at, ticks))
    with Engine(params.n, params=params, group=args.group) as eng:
        eng.step(args.at)
        eng.rumor_open(len(sources))
        reach = []
        for b, s in enumerate(sources):
            eng.rumor_seed(b, s)
            reach.append(eng.reach(s, "from").summary())
        last = []
        for t in range(args.at, ticks + 1):
            if t > args.at:
                eng.step(1)
            if (t - args.at) % every == 0 or t == ticks:
                last = [eng.rumor(b) for b in range(len(sources))]
                print(json.dumps({"tick": t, "alive": last[0].info["alive"], "known_share": [
                    round(r.info["known_alive"] / max(r.info["alive"], 1), 6) for r in last]}), flush=True)
        print(json.dumps({"seed_tick": args.at, "sources": [
            dict(source=s, ticks_to_50=r.ticks_to(0.5), ticks_to_99=r.ticks_to(0.99),
                 ticks_to_full=r.ticks_to(1.0), unknown_alive=r.summary()["unknown_alive"],
                 reach_depth=q["depth"], reach_unreached=q["unreached"],
                 trace_kernel_ms=round(r.info["kernel_ms"], 4))
            for s, r, q in zip(sources, last, reach)]}), flush=True)


if __name__ == "__main__":
    main()
