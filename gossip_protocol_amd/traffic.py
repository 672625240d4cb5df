"""Traffic ledger of the scale engines (gsp_scale_traffic_* / gsp_pview_traffic_* in
include/gossip/gossip.h): what the protocol costs and who pays -- per node the messages it sent,
the messages addressed to it while alive (before and after the inbox cut) and while not alive,
the member entries it had to merge and its largest fan-in of one tick; per tick the totals and
the fan-in histogram; for up to 1,024 watched nodes the reference's sent_msgs / recv_msgs rows.

A ledger opened at tick T0 covers the ticks in (T0, tick].  fanin[t][b]: the receivers alive at t
that were sent k messages, b = 0 for k = 0, else 2^(b-1) <= k < 2^b, the last bucket open-ended.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check

ARRAYS = ("sent", "recv", "merged", "lost", "entries_in", "peak_recv", "peak_tick")
BY_TICK = ("sent", "recv", "merged", "lost", "entries", "max_fanin")
BUCKETS = 18
MAX_WATCH = 1024


def bucket_of(k):
    """The fanin bucket of a message count (array or scalar)."""
    k = np.asarray(k, np.int64)
    b = np.where(k > 0, np.floor(np.log2(np.maximum(k, 1))).astype(np.int64) + 1, 0)
    return np.minimum(b, BUCKETS - 1)


class Traffic:
    """The ledger at one tick: `tick`, the per-node arrays named in ARRAYS (uint32; entries_in
    uint64; peak_tick int32 with -1 for none), `state` (uint8, as in census.Census), `by_tick`
    (uint64, [tick + 1][6], columns BY_TICK), `fanin` (uint64, [tick + 1][18]), `watch_ids` and
    `watch` (uint32, [n_watch][tick + 1][2]: sent, recv); `info` is the call's gsp_traffic_info as a
    dict (tick, n, open_tick, ticks_counted, n_watch, sent, recv, merged, lost, entries, overflow,
    max_fanin, max_fanin_node, kernel_ms)."""

    def __init__(self, tick, sent, recv, merged, lost, entries_in, peak_recv, peak_tick, state=None,
                 by_tick=None, fanin=None, watch_ids=(), watch=None, info=None):
        self.tick = int(tick)
        self.sent = np.asarray(sent, np.uint32)
        self.recv = np.asarray(recv, np.uint32)
        self.merged = np.asarray(merged, np.uint32)
        self.lost = np.asarray(lost, np.uint32)
        self.entries_in = np.asarray(entries_in, np.uint64)
        self.peak_recv = np.asarray(peak_recv, np.uint32)
        self.peak_tick = np.asarray(peak_tick, np.int32)
        n = self.sent.size
        self.state = np.asarray(state if state is not None else np.ones(n), np.uint8)
        self.by_tick = np.asarray(by_tick if by_tick is not None else np.zeros((0, 6)), np.uint64)
        self.fanin = np.asarray(fanin if fanin is not None else np.zeros((0, BUCKETS)), np.uint64)
        self.watch_ids = np.asarray(watch_ids, np.int32)
        self.watch = np.asarray(watch if watch is not None else np.zeros((len(self.watch_ids), 0, 2)),
                                np.uint32)
        self.info = dict(info or {})

    def summary(self, top=5):
        """Totals over the covered ticks; alive_node_rounds (the fanin rows summed: every alive
        node of every covered tick once); messages_ / entries_per_alive_node_round (recv and
        entries over them); lost_share (the share of the messages that arrived in the covered ticks
        whose receiver was not alive: lost / (recv + lost)); overflow_share ((recv - merged) / recv); hubs: the
        `top` nodes by peak_recv as (node, peak_recv, peak_tick), ties by id; recv_max_over_mean
        and recv_gini over the nodes that received anything or are alive."""
        sent, recv = int(self.sent.astype(np.int64).sum()), int(self.recv.astype(np.int64).sum())
        merged, lost = int(self.merged.astype(np.int64).sum()), int(self.lost.astype(np.int64).sum())
        entries = int(self.entries_in.astype(np.uint64).sum())
        rounds = int(self.fanin.astype(np.int64).sum())
        order = np.lexsort((np.arange(self.recv.size), -self.peak_recv.astype(np.int64)))[:top]
        hubs = [(int(x), int(self.peak_recv[x]), int(self.peak_tick[x])) for x in order
                if self.peak_recv[x] > 0]
        pool = self.recv[(self.recv > 0) | (self.state == 1)].astype(np.float64)
        gini, over = 0.0, 0.0
        if pool.size and pool.sum() > 0:
            v = np.sort(pool)
            i = np.arange(1, v.size + 1)
            gini = float((2.0 * (i * v).sum()) / (v.size * v.sum()) - (v.size + 1.0) / v.size)
            over = float(v.max() / v.mean())
        return {
            "tick": self.tick,
            "open_tick": int(self.info.get("open_tick", 0)),
            "sent": sent, "recv": recv, "merged": merged, "lost": lost, "entries": entries,
            "overflow": recv - merged,
            "alive_node_rounds": rounds,
            "messages_per_alive_node_round": recv / rounds if rounds else 0.0,
            "entries_per_alive_node_round": entries / rounds if rounds else 0.0,
            "lost_share": lost / (recv + lost) if recv + lost else 0.0,
            "overflow_share": (recv - merged) / recv if recv else 0.0,
            "hubs": hubs,
            "recv_max_over_mean": over,
            "recv_gini": gini,
        }

    def write_msgcount(self, path):
        """The watched nodes' rows as the reference's msgcount.log (gsp_traffic_write_msgcount):
        the w-th watched node is printed as node w + 1, one column per tick 0..tick."""
        write_msgcount(path, self.watch[:, :, 0], self.watch[:, :, 1])


def write_msgcount(path, sent, recv):
    """gsp_traffic_write_msgcount of two [nodes][ticks] count arrays."""
    sent = np.ascontiguousarray(sent, np.int32)
    recv = np.ascontiguousarray(recv, np.int32)
    assert sent.shape == recv.shape and sent.ndim == 2, (sent.shape, recv.shape)
    P32 = ctypes.POINTER(ctypes.c_int32)
    check(_lib.lib().gsp_traffic_write_msgcount(path.encode(), sent.ctypes.data_as(P32),
                                                recv.ctypes.data_as(P32), sent.shape[0], sent.shape[1]),
          "gsp_traffic_write_msgcount")


def open_(fn, handle, watch, what):
    """Call gsp_scale_traffic_open / gsp_pview_traffic_open `fn`; returns the watch ids kept."""
    ids = np.ascontiguousarray(np.atleast_1d(watch) if watch is not None else [], np.int32)
    check(fn(handle, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if ids.size else None, ids.size),
          what)
    return ids


def get(fn, handle, params, watch_ids, what):
    """Call gsp_scale_traffic_get / gsp_pview_traffic_get `fn` on an engine handle."""
    n, span = params.n, params.max_ticks + 1
    u32 = lambda: np.zeros(n, np.uint32)
    sent, recv, merged, lost, peak = u32(), u32(), u32(), u32(), u32()
    entries = np.zeros(n, np.uint64)
    peak_tick = np.zeros(n, np.int32)
    state = np.zeros(n, np.uint8)
    by_tick = np.zeros((span, 6), np.uint64)
    fanin = np.zeros((span, BUCKETS), np.uint64)
    watch = np.zeros((max(len(watch_ids), 1), span, 2), np.uint32)
    info = _lib.GspTrafficInfo()
    PU32, PU64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    check(fn(handle, sent.ctypes.data_as(PU32), recv.ctypes.data_as(PU32), merged.ctypes.data_as(PU32),
             lost.ctypes.data_as(PU32), entries.ctypes.data_as(PU64), peak.ctypes.data_as(PU32),
             peak_tick.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
             state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), by_tick.ctypes.data_as(PU64),
             fanin.ctypes.data_as(PU64), watch.ctypes.data_as(PU32), span, ctypes.byref(info)), what)
    T = info.tick
    return Traffic(T, sent, recv, merged, lost, entries, peak, peak_tick, state, by_tick[:T + 1],
                   fanin[:T + 1], watch_ids, watch[:len(watch_ids), :T + 1],
                   {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"})
