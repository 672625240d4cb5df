"""Multi-source overlay reach of the scale engines (gsp_scale_reach_multi /
gsp_pview_reach_multi in include/gossip/gossip.h): up to 64 exact single-source BFS trees over the
graph of reach.py, grown together on the device -- bit b of a node's 64-bit word belongs to
sources[b] alone, and row b of every array equals what reach() returns for that one source.

With a "from" and a "to" result of the same sources, bowtie() gives each source's place in the
directed structure: its strongly connected component is what it both reaches and is reached by.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE
from .reach import DIRECTIONS, FROM, TO

MAX_SOURCES = _lib.REACH_MAX_SOURCES


def bit_rows(seen, k):
    """seen (uint64 per node) as a bool matrix [k, n]: row b is bit b."""
    seen = np.asarray(seen, np.uint64)
    return ((seen[None, :] >> np.arange(k, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)


class ReachMulti:
    """One multi-source reach: `tick`, `sources` (int32, bit b is sources[b]), per node `seen`
    (uint64) and `state` (uint8, as in census.Census), `hops` (int32 [n_sources, n], -1: not alive
    or not reached; None when not asked for), per source `reached`, `ecc` (-1: the source is not
    alive) and `sum_hops`, `level_sizes` (uint32 [n_sources, level_cap]) and `info`, the call's
    gsp_reach_multi_info as a dict."""

    def __init__(self, tick, sources, seen, hops, reached, ecc, sum_hops, level_sizes, state, info=None):
        self.tick = int(tick)
        self.sources = np.asarray(sources, np.int32)
        self.seen = np.asarray(seen, np.uint64)
        self.hops = None if hops is None else np.asarray(hops, np.int32)
        self.reached = np.asarray(reached, np.int32)
        self.ecc = np.asarray(ecc, np.int32)
        self.sum_hops = np.asarray(sum_hops, np.int64)
        self.level_sizes = np.asarray(level_sizes, np.uint32)
        self.state = np.asarray(state, np.uint8)
        self.info = dict(info or {})

    def sets(self):
        """The reach sets as a bool matrix [n_sources, n] (row b: bit b of seen)."""
        return bit_rows(self.seen, self.sources.size)

    def summary(self):
        """Over the alive sources (ecc >= 0): mean_hops, the mean hop count over every (source,
        reached node) pair, the source itself included at 0; diameter_bound, the largest ecc (a
        lower bound of the diameter; the diameter of what the sources span); the min / median /
        max of reached; distinct_sets, the number of different reach sets."""
        live = self.ecc >= 0
        reached = self.reached[live]
        pairs = int(reached.sum(dtype=np.int64))
        direction = self.info.get("direction")
        sets = self.sets()[live]
        return {
            "tick": self.tick,
            "direction": {FROM: "from", TO: "to"}.get(direction, direction),
            "alive": int((self.state == ALIVE).sum()),
            "sources": int(self.sources.size),
            "alive_sources": int(live.sum()),
            "mean_hops": float(self.sum_hops[live].sum(dtype=np.int64) / pairs) if pairs else 0.0,
            "diameter_bound": int(self.ecc[live].max()) if live.any() else -1,
            "reached_min": int(reached.min()) if live.any() else 0,
            "reached_median": float(np.median(reached)) if live.any() else 0.0,
            "reached_max": int(reached.max()) if live.any() else 0,
            "distinct_sets": int(np.unique(np.packbits(sets, axis=1), axis=0).shape[0]) if live.any() else 0,
        }


def bowtie(frm, to):
    """Each source's place in the directed graph, from a "from" and a "to" ReachMulti of the same
    sources at the same tick.  Per source b (int64 arrays of n_sources; all 0 but `neither` for a
    source that is not alive):
      scc         nodes b reaches and is reached by: its strongly connected component, b included
      downstream  nodes b reaches that cannot reach b
      upstream    nodes that reach b and that b cannot reach
      neither     live nodes in none of the three
    and same[a, b]: sources a and b lie in one strongly connected component."""
    if frm.tick != to.tick or not np.array_equal(frm.sources, to.sources):
        raise ValueError("bowtie: the two results are of different ticks or sources")
    if frm.info.get("direction", FROM) != FROM or to.info.get("direction", TO) != TO:
        raise ValueError("bowtie: needs a 'from' and a 'to' result, in this order")
    f, t = frm.sets(), to.sets()
    core = f & t
    live = frm.state == ALIVE
    return {
        "scc": core.sum(axis=1, dtype=np.int64),
        "downstream": (f & ~t).sum(axis=1, dtype=np.int64),
        "upstream": (t & ~f).sum(axis=1, dtype=np.int64),
        "neither": (live[None, :] & ~f & ~t).sum(axis=1, dtype=np.int64),
        "same": core[:, frm.sources.astype(np.int64)],
    }


def run(fn, handle, n, sources, direction, age_limit, hops, level_cap, what):
    """Call gsp_scale_reach_multi / gsp_pview_reach_multi `fn` on an engine handle."""
    if isinstance(direction, str):
        if direction not in DIRECTIONS:
            raise ValueError("direction %r: 'from' or 'to'" % (direction,))
        direction = DIRECTIONS[direction]
    src = np.ascontiguousarray(np.atleast_1d(np.asarray(sources, np.int64)).astype(np.int32))
    k, cap = int(src.size), int(level_cap)
    seen, state = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    hop = np.full((k, n), -1, np.int32) if hops else None
    reached, ecc = np.zeros(k, np.int32), np.full(k, -1, np.int32)
    sums, sizes = np.zeros(k, np.int64), np.zeros((k, max(cap, 0)), np.uint32)
    info = _lib.GspReachMultiInfo()
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    check(fn(handle, int(direction), int(age_limit), ptr(src, ctypes.c_int32), k,
             ptr(seen, ctypes.c_uint64), ptr(hop, ctypes.c_int32) if hops else None,
             ptr(reached, ctypes.c_int32), ptr(ecc, ctypes.c_int32), ptr(sums, ctypes.c_int64),
             ptr(sizes, ctypes.c_uint32), cap, ptr(state, ctypes.c_uint8), ctypes.byref(info)), what)
    return ReachMulti(info.tick, src, seen, hop, reached, ecc, sums, sizes, state,
                      {f: getattr(info, f) for f, _ in info._fields_})
