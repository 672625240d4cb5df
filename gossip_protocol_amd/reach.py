"""Overlay reach of the scale engines (gsp_scale_reach / gsp_pview_reach in
include/gossip/gossip.h): BFS hop counts over the "r lists x" graph of the nodes alive at the
engine's current tick, computed on the device from the tables in HBM.

direction "from": hops[x] is the fewest edges from any source to x -- a lower bound on the ticks
what the sources know needs to reach x; "to": hops[r] is the fewest edges from r to any source
-- whose gossip can reach the sources.  A live node with hops -1 cannot be reached at all.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE

FROM, TO = 0, 1
DIRECTIONS = {"from": FROM, "to": TO}


class Reach:
    """One reach: `tick`, and per node `hops` (int32, -1: not alive or not reached) and `state`
    (uint8, as in census.Census); `info` is the call's gsp_reach_info as a dict (tick, n,
    age_limit, direction, alive, sources, reached, depth, levels, sum_hops, kernel_ms)."""

    def __init__(self, tick, hops, state, info=None):
        self.tick = int(tick)
        self.hops = np.asarray(hops, np.int32)
        self.state = np.asarray(state, np.uint8)
        self.info = dict(info or {})

    def level_sizes(self):
        """Nodes per hop count: level_sizes()[k] nodes have hops == k (empty: nobody reached)."""
        return np.bincount(self.hops[self.hops >= 0])

    def summary(self):
        """alive: nodes alive at the tick; sources: the level-0 set; reached: nodes with
        hops >= 0; unreached: alive - reached, the live nodes no path connects; depth: the
        largest hop count (-1: no alive source); mean_hops over the reached nodes."""
        sizes = self.level_sizes()
        reached = int(sizes.sum())
        alive = int((self.state == ALIVE).sum())
        direction = self.info.get("direction")
        return {
            "tick": self.tick,
            "direction": {FROM: "from", TO: "to"}.get(direction, direction),
            "alive": alive,
            "sources": int(sizes[0]) if sizes.size else 0,
            "reached": reached,
            "unreached": alive - reached,
            "depth": int(sizes.size) - 1,
            "mean_hops": float((sizes * np.arange(sizes.size)).sum() / reached) if reached else 0.0,
            "level_sizes": [int(v) for v in sizes],
        }


def run(fn, handle, n, sources, direction, age_limit, what):
    """Call gsp_scale_reach / gsp_pview_reach `fn` on an engine handle."""
    if isinstance(direction, str):
        if direction not in DIRECTIONS:
            raise ValueError("direction %r: 'from' or 'to'" % (direction,))
        direction = DIRECTIONS[direction]
    src = np.ascontiguousarray(np.atleast_1d(np.asarray(sources, np.int64)).astype(np.int32))
    hops, state = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    info = _lib.GspReachInfo()
    P32 = ctypes.POINTER(ctypes.c_int32)
    check(fn(handle, int(direction), int(age_limit), src.ctypes.data_as(P32), src.size,
             hops.ctypes.data_as(P32), state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
             ctypes.byref(info)), what)
    return Reach(info.tick, hops, state, {k: getattr(info, k) for k, _ in info._fields_})
