"""The view audit of the scale engines (gsp_scale_audit / gsp_pview_audit in
include/gossip/gossip.h): the row-wise twin of the census.  Per alive observer r, over the
entries its view stores at the engine's current tick: how many there are, how many name a member
that is not alive, how many alive members' entries are age_limit ticks old or older, the sum and
maximum of their age, and the 64-bit fingerprint of view(r) + {r}.

The reference's Grader asks its questions per node (did node i remove the failed node, did node i
keep every live one); Audit.summary() answers them per observer at any size, and adds what column
sums cannot give: how many distinct views the live nodes hold and how many hold the true one.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE

_M64 = (1 << 64) - 1


def fp(x):
    """The fingerprint of the ids x (uint64 array): the splitmix64 finaliser."""
    with np.errstate(over="ignore"):
        z = np.asarray(x).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


class Audit:
    """One audit: `tick`, and per observer the arrays `state` (uint8, as in census.Census),
    `size`, `dead`, `suspect`, `age_sum` (uint32), `age_max` (uint8) and `print` (uint64); rows
    that are not alive hold 0.  `info` is the call's gsp_audit_info as a dict (tick, n, age_limit,
    alive, entries, kernel_ms)."""

    def __init__(self, tick, state, size, dead, suspect, age_sum, age_max, print, info=None):
        self.tick = int(tick)
        self.state = np.asarray(state, np.uint8)
        self.size = np.asarray(size, np.uint32)
        self.dead = np.asarray(dead, np.uint32)
        self.suspect = np.asarray(suspect, np.uint32)
        self.age_sum = np.asarray(age_sum, np.uint32)
        self.age_max = np.asarray(age_max, np.uint8)
        self.print = np.asarray(print, np.uint64)
        self.info = dict(info or {})

    def summary(self):
        """alive: observers alive at the tick.  classes: distinct prints among them,
        largest_class: the observers sharing the most common one.  exact: observers whose print
        equals the sum of fp over the alive nodes, the true view; converged: exact == alive.
        views_with_dead: observers listing at least one member that is not alive, dead_pairs:
        those entries (completeness: both reach 0).  missing_pairs: sum over alive r of alive -
        1 - (size - dead), the (alive observer, alive member) pairs not listed (meaningful for
        the full view, where a view holds every member).  suspect_pairs: alive members' entries
        at or past the age limit.  mean_age: age_sum over the alive members' entries, max_age:
        the oldest of them.  size_min / size_max: over the alive observers.

        A print is a sum mod 2^64 of 64-bit hashes, so two different views can collide:
        `classes`, `largest_class`, `exact` and `converged` are fingerprints, not proofs."""
        alive = self.state == ALIVE
        n_alive = int(alive.sum())
        size = self.size[alive].astype(np.int64)
        dead = self.dead[alive].astype(np.int64)
        live_entries = int((size - dead).sum())
        prints, counts = np.unique(self.print[alive], return_counts=True)
        with np.errstate(over="ignore"):
            truth = fp(np.nonzero(alive)[0]).sum(dtype=np.uint64) if n_alive else np.uint64(0)
        exact = int((self.print[alive] == truth).sum())
        age_sum = int(self.age_sum[alive].sum(dtype=np.int64))
        return {
            "tick": self.tick,
            "alive": n_alive,
            "classes": int(prints.size),
            "largest_class": int(counts.max()) if counts.size else 0,
            "exact": exact,
            "converged": exact == n_alive,
            "views_with_dead": int((dead > 0).sum()),
            "dead_pairs": int(dead.sum()),
            "missing_pairs": int((n_alive - 1 - (size - dead)).sum()),
            "suspect_pairs": int(self.suspect[alive].sum(dtype=np.int64)),
            "mean_age": age_sum / live_entries if live_entries else 0.0,
            "max_age": int(self.age_max[alive].max()) if n_alive else 0,
            "size_min": int(size.min()) if n_alive else 0,
            "size_max": int(size.max()) if n_alive else 0,
        }


def run(fn, handle, n, age_limit, what):
    """Call gsp_scale_audit / gsp_pview_audit `fn` on an engine handle."""
    u32 = lambda: np.zeros(n, np.uint32)
    size, dead, suspect, age_sum = u32(), u32(), u32(), u32()
    age_max, state, prints = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    info = _lib.GspAuditInfo()
    P32, P8 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    check(fn(handle, age_limit, size.ctypes.data_as(P32), dead.ctypes.data_as(P32),
             suspect.ctypes.data_as(P32), age_sum.ctypes.data_as(P32), age_max.ctypes.data_as(P8),
             prints.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), state.ctypes.data_as(P8),
             ctypes.byref(info)), what)
    return Audit(info.tick, state, size, dead, suspect, age_sum, age_max, prints,
                 {k: getattr(info, k) for k, _ in info._fields_})
