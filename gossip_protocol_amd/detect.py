"""Detection ledger of the scale engines (gsp_scale_detect_* / gsp_pview_detect_* in
include/gossip/gossip.h): the event records of every tick folded per member on the device -- when
each crashed node was first removed, when the last holder removed it, how often live nodes were
removed, and how often stale gossip brought a crashed node back.

Per member x (crash[x] is the engine's failure schedule, INT32_MAX = never; x is alive at t while
t <= crash[x]): first_remove / last_remove / removers over the remove records with t > crash[x],
false_removes / first_false over those with t <= crash[x], revivals = the join records with
t > crash[x], evicts = the evict records.  by_tick[t] = (true removes, false removes, revivals,
evictions) with record tick t.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

NEVER = np.iinfo(np.int32).max
ARRAYS = ("first_remove", "last_remove", "removers", "false_removes", "first_false", "revivals",
          "evicts")


class Detect:
    """The ledger at one tick: `tick`, `crash` (int32 per member), the per-member arrays named in
    ARRAYS (first_* / last_remove int32 with -1 for none, the counts uint32), `state` (uint8, as
    in census.Census), `by_tick` (uint64, [tick + 1][4]); `info` is the call's gsp_detect_info as
    a dict (tick, n, open_tick, kinds, ticks_folded, records, lost, true_removes, false_removes,
    joins, revivals, evicts, kernel_ms)."""

    def __init__(self, tick, crash, first_remove, last_remove, removers, false_removes, first_false,
                 revivals, evicts, state=None, by_tick=None, info=None):
        self.tick = int(tick)
        self.crash = np.asarray(crash, np.int32)
        self.first_remove = np.asarray(first_remove, np.int32)
        self.last_remove = np.asarray(last_remove, np.int32)
        self.removers = np.asarray(removers, np.uint32)
        self.false_removes = np.asarray(false_removes, np.uint32)
        self.first_false = np.asarray(first_false, np.int32)
        self.revivals = np.asarray(revivals, np.uint32)
        self.evicts = np.asarray(evicts, np.uint32)
        n = self.crash.size
        self.state = np.asarray(state if state is not None else np.zeros(n), np.uint8)
        self.by_tick = np.asarray(by_tick if by_tick is not None else np.zeros((0, 4)), np.uint64)
        self.info = dict(info or {})

    def summary(self):
        """bench.event_summary's fields under its definitions (last_tick = tick): crashed_nodes
        (crash < tick), crashed_nodes_detected (... with a remove after the crash),
        removes_per_detected_node, removes_of_live_nodes (false removes of members whose crash
        tick is >= tick), first_ / full_detection_latency_ticks (min / mean / max of first_remove
        - crash and last_remove - crash over the detected; None: nobody detected).  Added:
        revived_nodes (members re-added after their crash), revivals, falsely_removed_nodes
        (members removed while alive), lost."""
        crash = self.crash.astype(np.int64)
        count = self.removers.astype(np.int64)
        crashed = crash < self.tick
        det = crashed & (count > 0)

        def stat(a):
            return {"min": int(a.min()), "mean": float(a.mean()), "max": int(a.max())} if len(a) else None

        return {
            "tick": self.tick,
            "crashed_nodes": int(crashed.sum()),
            "crashed_nodes_detected": int(det.sum()),
            "removes_per_detected_node": float(count[det].mean()) if det.any() else 0.0,
            "removes_of_live_nodes": int(self.false_removes[crash >= self.tick].astype(np.int64).sum()),
            "first_detection_latency_ticks": stat((self.first_remove.astype(np.int64) - crash)[det]),
            "full_detection_latency_ticks": stat((self.last_remove.astype(np.int64) - crash)[det]),
            "revived_nodes": int((self.revivals > 0).sum()),
            "revivals": int(self.revivals.astype(np.int64).sum()),
            "falsely_removed_nodes": int((self.false_removes > 0).sum()),
            "lost": int(self.info.get("lost", 0)),
        }


def get(fn, handle, params, what):
    """Call gsp_scale_detect_get / gsp_pview_detect_get `fn` on an engine handle; params: the
    engine's gsp_scale_params / gsp_pview_params (the crash schedule is computed from them)."""
    n, span = params.n, params.max_ticks + 1
    i32 = lambda: np.zeros(n, np.int32)
    u32 = lambda: np.zeros(n, np.uint32)
    first, last, removers, false, first_false, revivals, evicts = i32(), i32(), u32(), u32(), i32(), u32(), u32()
    state = np.zeros(n, np.uint8)
    by_tick = np.zeros((span, 4), np.uint64)
    info = _lib.GspDetectInfo()
    P32, PU32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    check(fn(handle, first.ctypes.data_as(P32), last.ctypes.data_as(P32), removers.ctypes.data_as(PU32),
             false.ctypes.data_as(PU32), first_false.ctypes.data_as(P32), revivals.ctypes.data_as(PU32),
             evicts.ctypes.data_as(PU32), state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
             by_tick.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), span, ctypes.byref(info)), what)
    crash = _lib.fail_schedule(n, params.seed, params.fail_mode, params.fail_tick, params.fail_ppm,
                               params.policy)
    return Detect(info.tick, crash, first, last, removers, false, first_false, revivals, evicts, state,
                  by_tick[:info.tick + 1],
                  {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"})
