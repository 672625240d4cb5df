"""Rumor trace of the scale engines (gsp_scale_rumor_* / gsp_pview_rumor_* in
include/gossip/gossip.h): the tick at which every node first heard each of up to 32 rumors,
carried over the messages the engine really delivered -- dropped, cut by the inbox bound and
merged as the tick kernels do it -- one hop per tick.

heard[x] is the tick node x first heard the rumor (-1: never); known[t] is the number of nodes
with heard == t, counted on the device, so a per-tick coverage curve needs no n-length readback.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE

MAX_RUMORS = 32


class Rumor:
    """One rumor at one tick: `tick`, per node `heard` (int32, -1: not heard) and `state` (uint8,
    as in census.Census), `known` (int32, known[t] = nodes that first heard at t, t = 0..tick);
    `info` is the call's gsp_rumor_info as a dict (tick, n, rumor, seed_tick, sources, alive,
    known, known_alive, last_heard, ticks_traced, kernel_ms)."""

    def __init__(self, tick, heard, state, known, info=None):
        self.tick = int(tick)
        self.heard = np.asarray(heard, np.int32)
        self.state = np.asarray(state, np.uint8)
        self.known = np.asarray(known, np.int32)
        self.info = dict(info or {})

    def coverage(self):
        """Per tick 0..tick, the nodes that have heard by then (the running sum of `known`)."""
        return np.cumsum(self.known.astype(np.int64))

    def ticks_to(self, share):
        """Ticks after seed_tick until `share` (0..1] of the nodes alive now had heard; None if
        that many have not (or the rumor was never seeded)."""
        seed = int(self.info.get("seed_tick", -1))
        live = self.state == ALIVE
        h = np.sort(self.heard[live & (self.heard >= 0)])
        need = int(np.ceil(share * live.sum()))
        if seed < 0 or need < 1 or h.size < need:
            return None
        return int(h[need - 1]) - seed

    def summary(self):
        """alive: nodes alive at the tick; known: nodes that heard; known_alive: those of them
        alive now; unknown_alive: the live nodes the rumor has not reached; last_heard: the last
        tick anyone first heard it (-1: nobody); latency_*: nearest-rank percentiles and maximum
        of heard - seed_tick over the nodes that heard (None: nobody did, or never seeded)."""
        got = self.heard >= 0
        live = self.state == ALIVE
        seed = int(self.info.get("seed_tick", -1))
        lat = np.sort(self.heard[got].astype(np.int64) - seed) if seed >= 0 and got.any() else None

        def pct(q):          # nearest rank: the smallest value with at least q % at or below it
            return int(lat[max(0, -(-q * lat.size // 100) - 1)]) if lat is not None else None

        return {
            "tick": self.tick,
            "seed_tick": seed,
            "sources": int(self.info.get("sources", 0)),
            "alive": int(live.sum()),
            "known": int(got.sum()),
            "known_alive": int((got & live).sum()),
            "unknown_alive": int((~got & live).sum()),
            "last_heard": int(self.heard.max()) if self.heard.size and got.any() else -1,
            "latency_p50": pct(50),
            "latency_p90": pct(90),
            "latency_max": int(lat.max()) if lat is not None else None,
        }


def open_trace(fn, handle, rumors, what):
    check(fn(handle, int(rumors)), what)


def seed(fn, handle, rumor, sources, what):
    src = np.ascontiguousarray(np.atleast_1d(np.asarray(sources, np.int64)).astype(np.int32))
    check(fn(handle, int(rumor), src.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), src.size), what)


def get(fn, handle, n, max_ticks, rumor, what):
    """Call gsp_scale_rumor_get / gsp_pview_rumor_get `fn` on an engine handle."""
    heard, state = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    known = np.zeros(max_ticks + 1, np.int32)
    info = _lib.GspRumorInfo()
    P32 = ctypes.POINTER(ctypes.c_int32)
    check(fn(handle, int(rumor), heard.ctypes.data_as(P32),
             state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), known.ctypes.data_as(P32),
             known.size, ctypes.byref(info)), what)
    return Rumor(info.tick, heard, state, known[:info.tick + 1],
                 {k: getattr(info, k) for k, _ in info._fields_})
