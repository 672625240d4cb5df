"""The expected overlay components, in numpy, over tests/reach_oracle.py's edges of the CPU oracle's
rows (states, edges_at, graph) -- never from the engine's own row().

weak():      min-label propagation over the undirected edges with pointer jumping
strong():    an iterative Tarjan over the CSR of graph()
expected():  the canonical labels plus every gsp_components_info field they determine
depth():     the longest path of the condensation, in components
Labels are the smallest id of the component, -1 for a node that is not alive.  Needs no scipy.
"""
import numpy as np

from tests import reach_oracle as ro

WEAK, STRONG = 0, 1
INFO = ("tick", "n", "age_limit", "kind", "alive", "components", "largest", "largest_label", "singletons",
        "converged")


def pairs(t, edges, age_limit):
    """(r, x) of every edge of G(t, age_limit), self-loops included."""
    r, x, ts, _ = edges
    keep = ((t - ts) & 31) < age_limit
    return r[keep].astype(np.int64), x[keep].astype(np.int64)


def weak(n, live, r, x):
    """Labels of the undirected graph: every alive node starts as its own label and takes the
    smallest label across any edge until nothing changes; jumping keeps the rounds few."""
    lab = np.where(live, np.arange(n, dtype=np.int64), -1)
    a, b = np.concatenate([r, x]), np.concatenate([x, r])
    while a.size:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        for _ in range(64):                              # pointer jumping: label of the label
            nxt = np.where(new >= 0, new[np.maximum(new, 0)], -1)
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return lab.astype(np.int32)


def strong(n, live, off, nbr):
    """Labels of the directed graph by an iterative Tarjan over out-edge CSR (off, nbr)."""
    index = np.full(n, -1, np.int64)
    low = np.zeros(n, np.int64)
    on = np.zeros(n, bool)
    lab = np.full(n, -1, np.int32)
    off = off.tolist()
    nbr = nbr.tolist()
    idx, low_, on_ = index.tolist(), low.tolist(), on.tolist()
    out = lab.tolist()
    counter = 0
    stack = []
    for root in np.nonzero(live)[0].tolist():
        if idx[root] >= 0:
            continue
        work = [(root, off[root])]
        idx[root] = low_[root] = counter
        counter += 1
        stack.append(root)
        on_[root] = True
        while work:
            v, e = work[-1]
            if e < off[v + 1]:
                work[-1] = (v, e + 1)
                w = nbr[e]
                if idx[w] < 0:
                    idx[w] = low_[w] = counter
                    counter += 1
                    stack.append(w)
                    on_[w] = True
                    work.append((w, off[w]))
                elif on_[w]:
                    low_[v] = min(low_[v], idx[w])
                continue
            work.pop()
            if work:
                u = work[-1][0]
                low_[u] = min(low_[u], low_[v])
            if low_[v] == idx[v]:
                members = []
                while True:
                    w = stack.pop()
                    on_[w] = False
                    members.append(w)
                    if w == v:
                        break
                m = min(members)
                for w in members:
                    out[w] = m
    return np.asarray(out, np.int32)


def labels(n, t, state, edges, age_limit, kind):
    live = state == ro.ALIVE
    r, x = pairs(t, edges, age_limit)
    if kind == WEAK:
        return weak(n, live, r, x)
    off, nbr = ro.csr(n, r, x)
    return strong(n, live, off, nbr)


def sizes(label):
    """(labels, sizes), the largest first and equal sizes by ascending label."""
    lab, cnt = np.unique(label[label >= 0], return_counts=True)
    order = np.lexsort((lab, -cnt))
    return lab[order], cnt[order]


def expected(n, t, state, edges, age_limit, kind):
    """{"label", "info", "sizes"}: what the engine must return for this graph."""
    label = labels(n, t, state, edges, age_limit, kind)
    lab, cnt = sizes(label)
    info = {"tick": t, "n": n, "age_limit": age_limit, "kind": kind, "alive": int((state == ro.ALIVE).sum()),
            "components": int(cnt.size), "largest": int(cnt[0]) if cnt.size else 0,
            "largest_label": int(lab[0]) if cnt.size else -1, "singletons": int((cnt == 1).sum()),
            "converged": 1}
    return {"label": label, "info": info, "sizes": cnt}


def depth(n, t, edges, age_limit, label):
    """The number of components on the longest path of the condensation of the strong labels
    `label` (1 for a single component, 0 for no alive node)."""
    r, x = pairs(t, edges, age_limit)
    a, b = label[r].astype(np.int64), label[x].astype(np.int64)
    cross = a != b
    dag = np.unique(np.stack([a[cross], b[cross]], axis=1), axis=0)
    comps = np.unique(label[label >= 0])
    if not comps.size:
        return 0
    level = np.zeros(n, np.int64)
    level[comps] = 1
    indeg = np.bincount(dag[:, 1], minlength=n)
    off, nbr = ro.csr(n, dag[:, 0], dag[:, 1])
    ready = [int(c) for c in comps if indeg[c] == 0]
    while ready:
        c = ready.pop()
        for w in nbr[off[c]:off[c + 1]].tolist():
            level[w] = max(level[w], level[c] + 1)
            indeg[w] -= 1
            if indeg[w] == 0:
                ready.append(w)
    return int(level.max())
