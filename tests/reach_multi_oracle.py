"""The expected multi-source reach, in numpy: tests/reach_oracle.py's single-source BFS stacked
per source over the CPU oracle's rows -- never the engine's own row().

expected():  per source b one reach_oracle.bfs from {sources[b]} (nothing for a source that is
             not alive), and from that stack alone every array and every gsp_reach_multi_info
             field the call must return
sample():    the issue's 64-id sample of a workload
few():       five ids: a duplicate, a node the schedule crashes early, and the highest id (under a
             join schedule the last to start)
"""
import numpy as np

from tests import reach_oracle as ro

INFO = ("tick", "n", "age_limit", "direction", "alive", "n_sources", "alive_sources", "depth", "levels",
        "reserved", "pairs", "sum_hops")
PER_SOURCE = ("reached", "ecc", "sum_hops")


def sample(n):
    return np.unique(np.r_[0, n - 1, np.arange(62) * 2654435761 % n])[:64]


def few(orc, n):
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    crashes = np.nonzero(fail < 10000)[0]
    stays = np.nonzero(fail >= 10000)[0]
    stays = stays[stays > 0]
    a, b = int(stays[0]), int(stays[len(stays) // 2])
    return [a, int(crashes[0]), b, a, n - 1]


def expected(n, t, state, adj, age_limit, direction, sources, level_cap=256):
    """What reach_multi(sources) must return over adj = reach_oracle.graph(...), as a dict of the
    arrays (hops [k, n], seen, reached, ecc, sum_hops, level_sizes [k, level_cap]) and "info"."""
    off, nbr = adj
    src = np.asarray(sources, np.int64)
    k = int(src.size)
    rows = {}                                             # one BFS per distinct alive id
    hops = np.full((k, n), -1, np.int32)
    for b, s in enumerate(src):
        if state[s] != ro.ALIVE:
            continue
        if int(s) not in rows:
            rows[int(s)] = ro.bfs(n, off, nbr, [int(s)])
        hops[b] = rows[int(s)]
    got = hops >= 0
    seen = np.zeros(n, np.uint64)
    for b in range(k):
        seen |= got[b].astype(np.uint64) << np.uint64(b)
    reached = got.sum(axis=1).astype(np.int32)
    ecc = hops.max(axis=1).astype(np.int32) if n else np.full(k, -1, np.int32)
    sums = np.where(got, hops, 0).sum(axis=1, dtype=np.int64)
    sizes = np.zeros((k, level_cap), np.uint32)
    for b in range(k):
        cnt = np.bincount(hops[b][got[b]])[:level_cap]
        sizes[b, :cnt.size] = cnt
    depth = int(ecc.max())
    info = {"tick": t, "n": n, "age_limit": age_limit, "direction": direction,
            "alive": int((state == ro.ALIVE).sum()), "n_sources": k,
            "alive_sources": int((state[src] == ro.ALIVE).sum()), "depth": depth, "levels": depth + 1,
            "reserved": 0, "pairs": int(reached.sum(dtype=np.int64)), "sum_hops": int(sums.sum())}
    return {"hops": hops, "seen": seen, "reached": reached, "ecc": ecc, "sum_hops": sums,
            "level_sizes": sizes, "info": info}


def distinct_sets(exp):
    """The number of different reach sets among the alive sources of an expected()."""
    live = exp["ecc"] >= 0
    return len({exp["hops"][b].__ge__(0).tobytes() for b in np.nonzero(live)[0]})


def component_sizes(frm, to):
    """Per source the size of its strongly connected component (0: not alive), from the
    expected() of both directions."""
    return ((frm["hops"] >= 0) & (to["hops"] >= 0)).sum(axis=1)
