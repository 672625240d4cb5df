#!/usr/bin/env python3
"""The directed structure of a .conf run's overlay, from multi-source reach: what reach_curve.py
says of one node, asked of a sample of them.

    python scripts/reach_survey.py CONF [--pview] [--samples K] [--every N] [--seed S] [--ticks T]
                                        [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview) and, at
tick 0, every N-th tick and the last one, grows the BFS trees of K sampled nodes (node 0 and K - 1
ids drawn with seed S; K <= 64) in both directions with two reach_multi() calls.  One JSON line per
sampled tick:
  from / to   ReachMulti.summary(): mean path length (mean_hops), diameter_bound, the spread of
              the reach-set sizes, the number of distinct reach sets, and the call's ms
  core        the largest strongly connected component a sampled node lies in: its size, its
              share of the alive nodes, the nodes upstream of it (they reach it, it does not reach
              them), downstream of it, and alive in neither
  outside     the sampled alive nodes that are not in the core: id, the size of their own
              component, and where they stand (upstream / downstream / apart)
  node0_in_core   is node 0's view the typical one
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def survey(eng, sources):
    """One tick's line (without the tick)."""
    from gossip_protocol_amd.reach_multi import bowtie
    frm = eng.reach_multi(sources, "from", hops=False)
    to = eng.reach_multi(sources, "to", hops=False)
    line = {"age_limit": frm.info["age_limit"]}
    for name, r in (("from", frm), ("to", to)):
        line[name] = dict(r.summary(), kernel_ms=round(r.info["kernel_ms"], 4))
    bt = bowtie(frm, to)
    alive = line["from"]["alive"]
    if not bt["scc"].any():
        return dict(line, core=None, outside=[], node0_in_core=False)
    c = int(np.argmax(bt["scc"]))                            # a sampled member of the core
    line["core"] = {"size": int(bt["scc"][c]), "share": round(float(bt["scc"][c]) / max(alive, 1), 6),
                    "upstream": int(bt["upstream"][c]), "downstream": int(bt["downstream"][c]),
                    "neither": int(bt["neither"][c]), "sampled_in_core": int(bt["same"][c].sum())}
    ids = frm.sources.astype(np.int64)
    above = (to.seen[ids] >> np.uint64(c)) & np.uint64(1)    # the sampled node reaches the core
    below = (frm.seen[ids] >> np.uint64(c)) & np.uint64(1)   # the core reaches it
    line["outside"] = [{"id": int(ids[b]), "scc": int(bt["scc"][b]),
                        "where": "upstream" if above[b] else "downstream" if below[b] else "apart"}
                       for b in range(ids.size) if frm.ecc[b] >= 0 and not bt["same"][c, b]]
    line["node0_in_core"] = bool(bt["same"][c, 0])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("conf")
    ap.add_argument("--pview", action="store_true", help="the partial-view engine (VIEW / INBOX keys)")
    ap.add_argument("--samples", type=int, default=64, help="sampled nodes K (1..64), node 0 among them")
    ap.add_argument("--every", type=int, default=10, help="sample every N-th tick")
    ap.add_argument("--seed", type=int, default=1, help="the seed of the sample")
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
    k = max(1, min(args.samples, 64, params.n))
    rest = np.random.default_rng(args.seed).choice(np.arange(1, params.n), k - 1, replace=False)
    sources = [0] + sorted(int(v) for v in rest)
    with Engine(params.n, params=params, group=args.group) as eng:
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
            if t % every == 0 or t == ticks:
                print(json.dumps(dict({"tick": t}, **survey(eng, sources))), flush=True)


if __name__ == "__main__":
    main()
