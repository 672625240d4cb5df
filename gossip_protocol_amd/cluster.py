"""Overlay clustering of the scale engines (gsp_scale_cluster / gsp_pview_cluster in
include/gossip/gossip.h): for up to 64 observers at once, over the graph of reach.py, how many of
an observer's out-neighbours list each other (links) and how many list the observer back (mutual).
Bit b of a node's 64-bit member word belongs to observers[b] alone.

With the path lengths of reach_multi this tells a random overlay from a lattice: a random graph
of density p has a clustering coefficient of about p, a bounded gossip view many times that.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE
from .reach_multi import bit_rows

MAX_OBSERVERS = _lib.CLUSTER_MAX_OBSERVERS


def _ratio(a, b):
    return float(a / b) if b else float("nan")


class Cluster:
    """One clustering call: `tick`, `observers` (int32, bit b is observers[b]), per node `member`
    (uint64: bit b set iff observers[b] lists the node) and `state` (uint8, as in census.Census),
    per observer `degree` (uint32), `links` (uint64: ordered pairs of neighbours with an edge
    between them) and `mutual` (uint32: neighbours that list the observer), and `info`, the call's
    gsp_cluster_info as a dict.  An observer that is not alive has zeros."""

    def __init__(self, tick, observers, member, degree, links, mutual, state, info=None):
        self.tick = int(tick)
        self.observers = np.asarray(observers, np.int32)
        self.member = np.asarray(member, np.uint64)
        self.degree = np.asarray(degree, np.uint32)
        self.links = np.asarray(links, np.uint64)
        self.mutual = np.asarray(mutual, np.uint32)
        self.state = np.asarray(state, np.uint8)
        self.info = dict(info or {})

    @property
    def live(self):
        """Per observer: alive at the call's tick."""
        return self.state[self.observers.astype(np.int64)] == ALIVE

    @property
    def coefficient(self):
        """The local clustering coefficient links / (k (k - 1)) per observer as float64; NaN where
        the degree k is below 2."""
        k = self.degree.astype(np.float64)
        out = np.full(k.shape, np.nan)
        np.divide(self.links.astype(np.float64), k * (k - 1), out=out, where=k >= 2)
        return out

    def sets(self):
        """The neighbour sets as a bool matrix [n_observers, n] (row b: bit b of member)."""
        return bit_rows(self.member, self.observers.size)

    def summary(self):
        """Over the alive observers: mean_degree; density, mean_degree / (alive - 1);
        mean_clustering, the mean coefficient over the observers with k >= 2 (NaN with none);
        transitivity, sum links / sum k (k - 1); reciprocity, sum mutual / sum k;
        clustering_over_density, how many times a random graph of this density the overlay is
        clustered."""
        live = self.live
        k = self.degree[live].astype(np.int64)
        alive = int((self.state == ALIVE).sum())
        coef = self.coefficient[live]
        coef = coef[~np.isnan(coef)]
        mean_degree = float(k.mean()) if k.size else float("nan")
        density = _ratio(mean_degree, alive - 1) if k.size else float("nan")
        mean_clustering = float(coef.mean()) if coef.size else float("nan")
        return {
            "tick": self.tick,
            "alive": alive,
            "observers": int(live.sum()),
            "mean_degree": mean_degree,
            "density": density,
            "mean_clustering": mean_clustering,
            "transitivity": _ratio(int(self.links[live].sum(dtype=np.uint64)), int((k * (k - 1)).sum())),
            "reciprocity": _ratio(int(self.mutual[live].sum(dtype=np.int64)), int(k.sum())),
            "clustering_over_density": _ratio(mean_clustering, density) if density == density else float("nan"),
        }

    def overlap(self):
        """How far the sampled views are from independent, from `member` alone: (matrix, jaccard)
        with matrix[a, b] = |N(a) & N(b)| (int64 [n_observers, n_observers]) and jaccard the mean
        of |N(a) & N(b)| / |N(a) | N(b)| over the pairs a < b of alive observers with distinct
        ids and a non-empty union (NaN with no such pair)."""
        sets = self.sets().astype(np.int64)
        inter = sets @ sets.T
        size = np.diagonal(inter)
        union = size[:, None] + size[None, :] - inter
        live = self.live
        ids = self.observers
        pair = np.triu(live[:, None] & live[None, :] & (ids[:, None] != ids[None, :]) & (union > 0), 1)
        jac = float((inter[pair] / union[pair]).mean()) if pair.any() else float("nan")
        return inter, jac


def run(fn, handle, n, observers, age_limit, what):
    """Call gsp_scale_cluster / gsp_pview_cluster `fn` on an engine handle."""
    obs = np.ascontiguousarray(np.atleast_1d(np.asarray(observers, np.int64)).astype(np.int32))
    k = int(obs.size)
    member, state = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    degree, mutual = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    links = np.zeros(k, np.uint64)
    info = _lib.GspClusterInfo()
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    check(fn(handle, int(age_limit), ptr(obs, ctypes.c_int32), k, ptr(member, ctypes.c_uint64),
             ptr(degree, ctypes.c_uint32), ptr(links, ctypes.c_uint64), ptr(mutual, ctypes.c_uint32),
             ptr(state, ctypes.c_uint8), ctypes.byref(info)), what)
    return Cluster(info.tick, obs, member, degree, links, mutual, state,
                   {f: getattr(info, f) for f, _ in info._fields_})
