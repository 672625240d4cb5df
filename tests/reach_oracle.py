"""The expected overlay reach, in numpy, from the CPU oracle's rows (ScaleOracle.row /
PviewOracle.row, fail_tick, start_tick) -- never from the engine's own row().

edges_at():  the (r, x, ts) triples stored by the rows alive at T, restricted to alive x
csr():       adjacency by np.argsort / np.searchsorted, out-edges (FROM) or in-edges (TO)
bfs():       level-synchronous, the levels by np.unique
expected():  hops plus every gsp_reach_info field the BFS determines
"""
import numpy as np

NOT_STARTED, ALIVE, CRASHED = 0, 1, 2
FROM, TO = 0, 1


def states(orc, n, t):
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    start = np.array([orc.start_tick(r) for r in range(n)])
    return np.where(start > t, NOT_STARTED, np.where(fail >= t, ALIVE, CRASHED)).astype(np.uint8)


def edges_at(orc, n, state, pview):
    """(r, x, ts) of every entry of an alive row for an alive member, and what the rows that
    are not alive still hold (entries a kernel that walked dead rows would follow)."""
    live = state == ALIVE
    rs, xs, tss, dead = [], [], [], 0
    for r in range(n):
        a, _, c = orc.row(r)
        if not pview:
            keep = a.astype(bool)
            a, c = np.nonzero(keep)[0], c[keep]
        if not live[r]:
            dead += int(a.size)
            continue
        ok = live[a]
        rs.append(np.full(int(ok.sum()), r, np.int32))
        xs.append(a[ok].astype(np.int32))
        tss.append(c[ok].astype(np.int32))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int32)
    return cat(rs), cat(xs), cat(tss), dead


def csr(n, key, val):
    """off, nbr: the vals of key k are nbr[off[k]:off[k + 1]]."""
    order = np.argsort(key, kind="stable")
    off = np.searchsorted(key[order], np.arange(n + 1)).astype(np.int64)
    return off, val[order]


def bfs(n, off, nbr, level0):
    hops = np.full(n, -1, np.int32)
    frontier = np.unique(np.asarray(level0, np.int64))
    hops[frontier] = 0
    level = 0
    while frontier.size:
        cnt = off[frontier + 1] - off[frontier]
        idx = np.repeat(off[frontier] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
        cand = nbr[idx]
        frontier = np.unique(cand[hops[cand] < 0]).astype(np.int64)
        level += 1
        hops[frontier] = level
    return hops


def graph(n, t, edges, age_limit, direction):
    """The CSR of G(t, age_limit): out-edges for FROM, in-edges for TO."""
    r, x, ts, _ = edges
    keep = ((t - ts) & 31) < age_limit
    r, x = r[keep], x[keep]
    return csr(n, r, x) if direction == FROM else csr(n, x, r)


def expected(n, t, state, adj, age_limit, direction, sources):
    """The Reach the engine must return, over adj = graph(...): hops and the info fields."""
    off, nbr = adj
    src = np.asarray(sources, np.int64)
    src = src[state[src] == ALIVE]
    hops = bfs(n, off, nbr, src)
    reached = hops >= 0
    depth = int(hops.max()) if reached.any() else -1
    info = {"tick": t, "n": n, "age_limit": age_limit, "direction": direction,
            "alive": int((state == ALIVE).sum()), "sources": int(np.unique(src).size),
            "reached": int(reached.sum()), "depth": depth, "levels": depth + 1,
            "sum_hops": int(hops[reached].sum(dtype=np.int64))}
    return hops, info


def source_sets(orc, n, high):
    """node 0; a high id; and a set with a duplicate, one node the schedule crashes and two that
    it never does."""
    fail = np.array([orc.fail_tick(r) for r in range(n)])
    crashes = np.nonzero(fail < 10000)[0]
    stays = np.nonzero(fail >= 10000)[0]
    stays = stays[stays > 0]
    a, b = int(stays[0]), int(stays[1])
    return {"zero": [0], "high": [high], "multi": [a, int(crashes[0]), b, a]}
