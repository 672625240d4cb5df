#!/usr/bin/env python3
"""The traffic curve of a .conf run, from the traffic ledger: the companion of detect_curve.py.

    python scripts/traffic_curve.py CONF [--pview] [--every K] [--ticks N] [--group G]
                                    [--watch ID ...] [--msgcount PATH]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview) with a
ledger opened at tick 0 and prints one JSON line per sampled tick (every K-th tick and the last
one): that tick's sent / recv / lost / overflow / entries, its largest fan-in and its fan-in
histogram (bucket 0: no message, bucket b: 2^(b-1) <= k < 2^b).  The last line is
Traffic.summary() of the whole run: the totals, the load per alive node-round, the share lost to
receivers that are not alive, the overflow share and the hubs.  --watch keeps per-tick (sent, recv)
rows of those nodes; --msgcount writes them in the reference's msgcount.log format.
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
    ap.add_argument("--watch", type=int, nargs="*", default=[], help="node ids to keep per-tick rows of")
    ap.add_argument("--msgcount", default=None, help="write the watched rows as a msgcount.log")
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
        eng.traffic_open(args.watch)
        eng.step(ticks)
        d = eng.traffic()
        for t in range(1, ticks + 1):
            if t % every and t != ticks:
                continue
            sent, recv, merged, lost, entries, top = (int(x) for x in d.by_tick[t])
            line = dict(tick=t, sent=sent, recv=recv, lost=lost, overflow=recv - merged, entries=entries,
                        max_fanin=top, fanin=[int(x) for x in d.fanin[t]])
            if len(d.watch_ids):
                line["watch"] = {int(x): [int(v) for v in d.watch[i, t]] for i, x in enumerate(d.watch_ids)}
            print(json.dumps(line), flush=True)
        s = d.summary()
        s["ledger_ms"] = round(d.info["kernel_ms"], 4)
        print(json.dumps(s), flush=True)
        if args.msgcount:
            d.write_msgcount(args.msgcount)
        eng.traffic_close()


if __name__ == "__main__":
    main()
