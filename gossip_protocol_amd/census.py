"""The membership census of the scale engines (gsp_scale_census / gsp_pview_census in
include/gossip/gossip.h): per member x, how many alive nodes list x, how many of those entries
are fresh, the largest heartbeat stored for x and x's own state, at the engine's current tick.

The reference's Grader asks three things of a run at N = 10 -- did everyone join, was every
crashed node removed by everyone (completeness), was no live node removed (accuracy);
Census.summary() answers them at any size from the census arrays.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

NOT_STARTED, ALIVE, CRASHED = 0, 1, 2


class Census:
    """One census: `tick`, and per member the arrays `state` (uint8: NOT_STARTED / ALIVE /
    CRASHED), `listed`, `fresh`, `max_hb` (uint32); `info` is the call's gsp_census_info as a
    dict (tick, n, age_limit, alive, entries, kernel_ms)."""

    def __init__(self, tick, state, listed, fresh, max_hb, info=None):
        self.tick = int(tick)
        self.state = np.asarray(state, np.uint8)
        self.listed = np.asarray(listed, np.uint32)
        self.fresh = np.asarray(fresh, np.uint32)
        self.max_hb = np.asarray(max_hb, np.uint32)
        self.info = dict(info or {})

    def summary(self):
        """alive, crashed: nodes in that state; undetected: crashed members somebody still
        lists, stale_pairs: the entries that do (completeness: both reach 0); orphans: alive
        members nobody lists; missing_pairs: sum over alive x of alive - 1 - listed[x], the
        (alive node, alive member) pairs not listed (accuracy and convergence: 0 once everyone
        lists everyone -- meaningful for the full view, where a view holds every member);
        max_listed: the most-listed member's count (the hubs of a partial view)."""
        alive = self.state == ALIVE
        crashed = self.state == CRASHED
        listed = self.listed.astype(np.int64)
        n_alive = int(alive.sum())
        return {
            "tick": self.tick,
            "alive": n_alive,
            "crashed": int(crashed.sum()),
            "undetected": int((crashed & (listed > 0)).sum()),
            "stale_pairs": int(listed[crashed].sum()),
            "orphans": int((alive & (listed == 0)).sum()),
            "missing_pairs": int((n_alive - 1 - listed[alive]).sum()),
            "max_listed": int(listed.max()) if listed.size else 0,
        }


def run(fn, handle, n, age_limit, what):
    """Call gsp_scale_census / gsp_pview_census `fn` on an engine handle."""
    u32 = lambda: np.zeros(n, np.uint32)
    listed, fresh, max_hb, state = u32(), u32(), u32(), np.zeros(n, np.uint8)
    info = _lib.GspCensusInfo()
    P32 = ctypes.POINTER(ctypes.c_uint32)
    check(fn(handle, age_limit, listed.ctypes.data_as(P32), fresh.ctypes.data_as(P32),
             max_hb.ctypes.data_as(P32), state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
             ctypes.byref(info)), what)
    return Census(info.tick, state, listed, fresh, max_hb,
                  {k: getattr(info, k) for k, _ in info._fields_})


def default_age_limit(params):
    """tfail if the engine suspects, else tremove."""
    return params.tfail if params.tfail > 0 else params.tremove
