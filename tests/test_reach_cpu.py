"""Overlay reach without a GPU: the struct mirror, the exported names, the declarations in
gossip.h, and Reach.level_sizes() / summary() on hand-made hops arrays."""
import ctypes
import os

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.census import ALIVE, CRASHED, NOT_STARTED
from gossip_protocol_amd.reach import FROM, TO, Reach

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reach_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_reach_info") == ctypes.sizeof(_lib.GspReachInfo)
    assert ctypes.sizeof(_lib.GspReachInfo) == 56


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    for name in ("gsp_scale_reach", "gsp_pview_reach"):
        assert name in _lib.SIGNATURES
        rc = getattr(L, name)(None, 0, 9, None, 0, None, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for decl in ("int gsp_scale_reach(gsp_scale *s, int32_t direction, int32_t age_limit",
                 "int gsp_pview_reach(gsp_pview *s, int32_t direction, int32_t age_limit",
                 "#define GSP_REACH_FROM 0", "#define GSP_REACH_TO   1", "} gsp_reach_info;"):
        assert decl in text, decl


def test_all_unreached():
    state = np.array([ALIVE, ALIVE, CRASHED, NOT_STARTED], np.uint8)
    r = Reach(5, np.full(4, -1), state, {"direction": FROM})
    assert r.level_sizes().size == 0 and r.hops.dtype == np.int32
    assert r.summary() == {"tick": 5, "direction": "from", "alive": 2, "sources": 0, "reached": 0,
                           "unreached": 2, "depth": -1, "mean_hops": 0.0, "level_sizes": []}


def test_single_source_alone():
    r = Reach(0, np.array([-1, 0, -1]), np.array([CRASHED, ALIVE, CRASHED], np.uint8), {"direction": TO})
    assert r.level_sizes().tolist() == [1]
    assert r.summary() == {"tick": 0, "direction": "to", "alive": 1, "sources": 1, "reached": 1,
                           "unreached": 0, "depth": 0, "mean_hops": 0.0, "level_sizes": [1]}


def test_unreachable_alive_nodes():
    # node:           0  1  2  3   4       5   6
    hops = np.array([0, 1, 1, 3, -1, -1, 2])
    state = np.array([ALIVE, ALIVE, ALIVE, ALIVE, ALIVE, CRASHED, ALIVE], np.uint8)
    r = Reach(12, hops, state, {"direction": FROM, "reached": 5})
    assert r.level_sizes().tolist() == [1, 2, 1, 1]
    s = r.summary()
    assert s == {"tick": 12, "direction": "from", "alive": 6, "sources": 1, "reached": 5,
                 "unreached": 1, "depth": 3, "mean_hops": (1 + 1 + 3 + 2) / 5,
                 "level_sizes": [1, 2, 1, 1]}
