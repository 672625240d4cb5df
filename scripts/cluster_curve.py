#!/usr/bin/env python3
"""How clustered a .conf run's overlay is over time, beside its path length: the two numbers
that tell a random overlay from a lattice, asked of a sample of nodes.

    python scripts/cluster_curve.py CONF [--pview] [--samples K] [--every N] [--seed S] [--ticks T]
                                         [--age-limit L] [--group G]

Runs the .conf (gsp_scale_params_from_conf, or gsp_pview_params_from_conf with --pview) and, at
tick 0, every N-th tick and the last one, makes one cluster() call for K sampled nodes (node 0 and
K - 1 ids drawn with seed S; K <= 64) and one reach_multi() call ("from") for the same sample.  One
JSON line per sampled tick:
  cluster     Cluster.summary(): mean_degree, density, mean_clustering (the mean local clustering
              coefficient), transitivity, reciprocity and clustering_over_density (1 for a random
              graph of this density), with rows (the rows the link pass walked) and the call's ms
  jaccard     the mean Jaccard index of the sampled views (Cluster.overlap())
  mean_hops, diameter_bound   of the same sample, with the reach_multi call's ms
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _num(v):
    """JSON has no NaN: None where a ratio has no denominator."""
    return None if isinstance(v, float) and v != v else v


def line_at(eng, observers, age_limit):
    c = eng.cluster(observers, age_limit)
    r = eng.reach_multi(observers, "from", age_limit, hops=False)
    s, rs = c.summary(), r.summary()
    return {"age_limit": c.info["age_limit"],
            "cluster": dict({k: _num(v) for k, v in s.items() if k != "tick"}, rows=c.info["rows"],
                            kernel_ms=round(c.info["kernel_ms"], 4)),
            "jaccard": _num(c.overlap()[1]),
            "mean_hops": rs["mean_hops"], "diameter_bound": rs["diameter_bound"],
            "reach_kernel_ms": round(r.info["kernel_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("conf")
    ap.add_argument("--pview", action="store_true", help="the partial-view engine (VIEW / INBOX keys)")
    ap.add_argument("--samples", type=int, default=64, help="sampled nodes K (1..64), node 0 among them")
    ap.add_argument("--every", type=int, default=10, help="sample every N-th tick")
    ap.add_argument("--seed", type=int, default=1, help="the seed of the sample")
    ap.add_argument("--ticks", type=int, default=None, help="stop after T ticks (default: the .conf's)")
    ap.add_argument("--age-limit", type=int, default=None, help="1..32 (default: as for census())")
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
    observers = [0] + sorted(int(v) for v in rest)
    with Engine(params.n, params=params, group=args.group) as eng:
        for t in range(0, ticks + 1):
            if t:
                eng.step(1)
            if t % every == 0 or t == ticks:
                print(json.dumps(dict({"tick": t}, **line_at(eng, observers, args.age_limit))), flush=True)


if __name__ == "__main__":
    main()
