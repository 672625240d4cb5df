"""The expected overlay clustering, in numpy, from the CPU oracle's rows through
tests/reach_oracle.py (edges_at, then graph) -- never from the engine's own row().

adjacency():  the dense boolean matrix of G(T, L): A[r, x] iff r -> x (n <= 4,096)
counts():     degree, links and mutual of EVERY node, from A alone
expected():   what cluster(observers) must return: every array and every gsp_cluster_info field
              but kernel_ms
edge():       the observer set that reaches the corners of the counts (see there)
"""
import numpy as np

from tests import reach_oracle as ro

INFO = ("tick", "n", "age_limit", "alive", "n_observers", "alive_observers", "rows", "reserved",
        "sum_degree", "sum_links", "sum_mutual")
ARRAYS = ("member", "degree", "links", "mutual")


def adjacency(n, adj):
    """adj = reach_oracle.graph(..., FROM): the out-edge CSR, as a dense bool matrix."""
    off, nbr = adj
    a = np.zeros((n, n), bool)
    a[np.repeat(np.arange(n), np.diff(off)), nbr] = True
    return a


def counts(a):
    """Of every node o with N = {x: a[o, x]}: degree |N|, links #{(u, v): u, v in N, a[u, v]},
    mutual #{u in N: a[u, o]}.  links[o] is the sum over v in N of the two-step paths o -> u -> v:
    in a sparse graph the sub-matrix of N summed per node, in a dense one (A A) masked by A, in
    float32, which is exact here: an entry of A A is at most n <= 4,096 < 2^24."""
    n = a.shape[0]
    assert n <= 4096
    degree = a.sum(axis=1).astype(np.int64)
    mutual = (a & a.T).sum(axis=1).astype(np.int64)
    if degree.mean() > 128:
        f = a.astype(np.float32)
        links = np.where(a, f @ f, 0).astype(np.int64).sum(axis=1)
    else:
        links = np.zeros(n, np.int64)
        for o in np.nonzero(degree)[0]:
            nb = np.nonzero(a[o])[0]
            links[o] = int(a[np.ix_(nb, nb)].sum())
    return degree, links, mutual


def expected(n, t, state, a, cnt, age_limit, observers):
    """What cluster(observers) must return over a = adjacency(...), cnt = counts(a): a dict of
    the arrays (member, degree, links, mutual) and "info"."""
    degree, links, mutual = cnt
    obs = np.asarray(observers, np.int64)
    k = int(obs.size)
    live = state[obs] == ro.ALIVE
    member = np.zeros(n, np.uint64)
    for b in np.nonzero(live)[0]:
        member |= a[obs[b]].astype(np.uint64) << np.uint64(b)
    deg = np.where(live, degree[obs], 0)
    lnk = np.where(live, links[obs], 0)
    mut = np.where(live, mutual[obs], 0)
    info = {"tick": t, "n": n, "age_limit": age_limit, "alive": int((state == ro.ALIVE).sum()),
            "n_observers": k, "alive_observers": int(live.sum()), "rows": int((member != 0).sum()),
            "reserved": 0, "sum_degree": int(deg.sum()), "sum_links": int(lnk.sum()),
            "sum_mutual": int(mut.sum())}
    return {"member": member, "degree": deg.astype(np.uint32), "links": lnk.astype(np.uint64),
            "mutual": mut.astype(np.uint32), "info": info}


def edge(n, state, cnt):
    """The `edge` observer set of one (tick, age limit), as (ids, slots): the first alive node
    with no neighbour, the first with exactly one (left out where there is none), the alive node
    with the largest links, a node that is not alive (crashed where one is, else not started),
    a duplicate of the largest-links node, and n - 1.  slots names each position."""
    degree, links, _ = cnt
    live = state == ro.ALIVE
    ids, slots = [], []

    def add(name, where):
        if where.size:
            ids.append(int(where[0]))
            slots.append(name)

    add("empty", np.nonzero(live & (degree == 0))[0])
    add("single", np.nonzero(live & (degree == 1))[0])
    top = int(np.argmax(np.where(live, links, -1)))
    add("top", np.array([top]))
    crashed = np.nonzero(state == ro.CRASHED)[0]
    add("dead", crashed if crashed.size else np.nonzero(~live)[0])
    add("again", np.array([top]))
    add("last", np.array([n - 1]))
    return ids, slots


def mean_clustering(state, cnt):
    """The mean local clustering coefficient over every alive node with k >= 2, the density
    mean degree / (alive - 1) and the reciprocity sum mutual / sum degree, over every alive node."""
    degree, links, mutual = cnt
    live = state == ro.ALIVE
    k = degree[live].astype(np.float64)
    big = k >= 2
    coef = links[live][big] / (k[big] * (k[big] - 1))
    return (float(coef.mean()) if coef.size else float("nan"), float(k.mean() / (live.sum() - 1)),
            float(mutual[live].sum() / max(k.sum(), 1)))
