#!/usr/bin/env python3
"""Into how many pieces a .conf run's overlay falls over time: the weak and strong components of
every sampled tick, beside reach_survey's core size.

    python scripts/components_curve.py CONF [--pview] [--every K] [--age-limit L] [--ticks T] [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview) and, at
tick 0, every K-th tick and the last one, makes one components() call of each kind.  One JSON line
per sampled tick:
  alive       the nodes alive at the tick
  weak, strong   per kind: components, giant (the largest component's size), giant_share of the
              alive nodes, singletons, nontrivial (components of two nodes or more), histogram
              (entry k: components of 2^k .. 2^(k+1) - 1 nodes), and the call's sweeps, rounds
              and kernel_ms
  nested_max  the most strong components inside one weak component
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _num(v):
    """JSON has no NaN: None where a ratio has no denominator."""
    return None if isinstance(v, float) and v != v else v


def line_at(eng, age_limit):
    from gossip_protocol_amd.components import nesting
    out, res = {}, {}
    for kind in ("weak", "strong"):
        c = res[kind] = eng.components(kind, age_limit)
        s = c.summary()
        out[kind] = dict({k: _num(v) for k, v in s.items() if k not in ("tick", "kind", "alive")},
                         sweeps=c.info["sweeps"], rounds=c.info["rounds"],
                         kernel_ms=round(c.info["kernel_ms"], 4))
        out["alive"], out["age_limit"] = s["alive"], c.info["age_limit"]
    counts = nesting(res["strong"], res["weak"])[1]
    out["nested_max"] = int(counts.max()) if counts.size else 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("conf")
    ap.add_argument("--pview", action="store_true", help="the partial-view engine (VIEW / INBOX keys)")
    ap.add_argument("--every", type=int, default=10, help="sample every K-th tick")
    ap.add_argument("--ticks", type=int, default=None, help="stop after T ticks (default: the .conf's)")
    ap.add_argument("--age-limit", type=int, default=None, help="1..32 (default: as for reach())")
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
                print(json.dumps(dict({"tick": t}, **line_at(eng, args.age_limit))), flush=True)


if __name__ == "__main__":
    main()
