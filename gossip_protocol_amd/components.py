"""Overlay components of the scale engines (gsp_scale_components / gsp_pview_components in
include/gossip/gossip.h): the exact weakly or strongly connected components of the graph of
reach.py at the engine's current tick.  Every alive node is labelled with the smallest id of its
component, so two results can be compared for equality whatever layout produced them.

After a mass failure this is the figure the peer-sampling literature reports: into how many
clusters the overlay has fallen and how large the largest one is.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .census import ALIVE

WEAK, STRONG = _lib.COMPONENTS_WEAK, _lib.COMPONENTS_STRONG
KINDS = {"weak": WEAK, "strong": STRONG}
DEFAULT_SWEEPS = _lib.COMPONENTS_DEFAULT_SWEEPS


class Components:
    """One components call: `tick`, `kind` ("weak" / "strong"), per node `label` (int32: the
    smallest id of the node's component, -1 for a node that is not alive) and `state` (uint8, as
    in census.Census), and `info`, the call's gsp_components_info as a dict.  `converged` is False
    when max_sweeps ended the call early; the labels then mean nothing."""

    def __init__(self, tick, kind, label, state, info=None, converged=True):
        self.tick = int(tick)
        self.kind = kind
        self.label = np.asarray(label, np.int32)
        self.state = np.asarray(state, np.uint8)
        self.info = dict(info or {})
        self.converged = bool(converged)

    def _need(self):
        if not self.converged:
            raise ValueError("the components call did not converge (max_sweeps too small)")

    def sizes(self):
        """(labels, sizes): every component's label and node count as int64 arrays, the largest
        first and equal sizes by ascending label."""
        self._need()
        labels, counts = np.unique(self.label[self.label >= 0], return_counts=True)
        order = np.lexsort((labels, -counts))
        return labels[order].astype(np.int64), counts[order].astype(np.int64)

    def of(self, x):
        """The ids of x's component, ascending; empty for a node that is not alive."""
        self._need()
        lab = int(self.label[int(x)])
        return np.nonzero(self.label == lab)[0] if lab >= 0 else np.zeros(0, np.int64)

    def summary(self):
        """components; giant (size of the largest) and giant_share of the alive nodes (NaN with
        none); giant_label; singletons; nontrivial (components of two nodes or more); histogram,
        a list whose entry k counts the components of 2^k .. 2^(k+1) - 1 nodes.  Raises ValueError
        when the call did not converge."""
        labels, sizes = self.sizes()
        alive = int((self.state == ALIVE).sum())
        hist = np.bincount(np.floor(np.log2(sizes)).astype(np.int64)).tolist() if sizes.size else []
        return {
            "tick": self.tick,
            "kind": self.kind,
            "alive": alive,
            "components": int(sizes.size),
            "giant": int(sizes[0]) if sizes.size else 0,
            "giant_label": int(labels[0]) if sizes.size else -1,
            "giant_share": float(sizes[0] / alive) if alive else float("nan"),
            "singletons": int((sizes == 1).sum()),
            "nontrivial": int((sizes >= 2).sum()),
            "histogram": hist,
        }


def nesting(strong, weak):
    """How the strong components sit inside the weak ones: (labels, counts) with, per weak
    component (by ascending label), the number of strong components inside it.  Raises ValueError
    if a strong component straddles two weak ones, which no graph allows."""
    strong._need()
    weak._need()
    live = strong.label >= 0
    if not np.array_equal(live, weak.label >= 0):
        raise ValueError("the two results are not of the same nodes")
    pairs = np.unique(np.stack([strong.label[live], weak.label[live]], axis=1), axis=0)
    if np.unique(pairs[:, 0]).size != pairs.shape[0]:
        raise ValueError("a strong component lies in two weak components")
    labels, counts = np.unique(pairs[:, 1], return_counts=True)
    return labels.astype(np.int64), counts.astype(np.int64)


Components.nesting = staticmethod(nesting)


def run(fn, handle, n, kind, age_limit, max_sweeps, what):
    """Call gsp_scale_components / gsp_pview_components `fn` on an engine handle."""
    code = KINDS.get(kind, kind)
    label, state = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    info = _lib.GspComponentsInfo()
    check(fn(handle, int(code), int(age_limit), int(max_sweeps), label.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
             state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(info)), what)
    name = {WEAK: "weak", STRONG: "strong"}[info.kind]
    return Components(info.tick, name, label, state, {f: getattr(info, f) for f, _ in info._fields_},
                      bool(info.converged))
