"""Multi-source reach without a GPU: the struct mirror, the exported names, the declarations in
gossip.h, and ReachMulti.summary() / bowtie() and tests/reach_multi_oracle.py on a hand-made graph.

The graph, nodes 0..7 (7 crashed), r -> x meaning "r lists x":
    0 -> 1 -> 2 -> 0     a cycle: one strongly connected component
    3 -> 0               3 is source-only: nobody lists it
    2 -> 4               4 is sink-only: it lists nobody
    5 <-> 6              a second component, apart from the first
"""
import ctypes
import os

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.census import ALIVE, CRASHED
from gossip_protocol_amd.reach import FROM, TO
from gossip_protocol_amd.reach_multi import ReachMulti, bowtie
from tests import reach_multi_oracle as rm
from tests import reach_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 8
EDGES = np.array([(0, 1), (1, 2), (2, 0), (3, 0), (2, 4), (5, 6), (6, 5)], np.int32)
STATE = np.array([ALIVE] * 7 + [CRASHED], np.uint8)
SOURCES = [0, 3, 4, 5, 7, 0]                 # 7 is not alive; 0 stands under two bits


def _expected(direction, level_cap=8):
    r, x = EDGES[:, 0], EDGES[:, 1]
    adj = ro.csr(N, r, x) if direction == FROM else ro.csr(N, x, r)
    return rm.expected(N, 4, STATE, adj, 9, direction, SOURCES, level_cap)


def _result(e):
    return ReachMulti(e["info"]["tick"], SOURCES, e["seen"], e["hops"], e["reached"], e["ecc"],
                      e["sum_hops"], e["level_sizes"], STATE, e["info"])


def test_reach_multi_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_reach_multi_info") == ctypes.sizeof(_lib.GspReachMultiInfo)
    assert ctypes.sizeof(_lib.GspReachMultiInfo) == 64
    assert _lib.REACH_MAX_SOURCES == 64


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    for name in ("gsp_scale_reach_multi", "gsp_pview_reach_multi"):
        assert name in _lib.SIGNATURES
        rc = getattr(L, name)(None, 0, 9, None, 0, None, None, None, None, None, None, 0, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for decl in ("int gsp_scale_reach_multi(gsp_scale *s, int32_t direction, int32_t age_limit",
                 "int gsp_pview_reach_multi(gsp_pview *s, int32_t direction, int32_t age_limit",
                 "#define GSP_REACH_MAX_SOURCES 64", "} gsp_reach_multi_info;", " * Multi-source reach:"):
        assert decl in text, decl
    assert text.index(" * Overlay reach:") < text.index(" * Multi-source reach:") < text.index(" * Rumor trace:")


def test_oracle_on_the_hand_made_graph():
    f, t = _expected(FROM), _expected(TO)
    assert f["hops"].tolist() == [[0, 1, 2, -1, 3, -1, -1, -1], [1, 2, 3, 0, 4, -1, -1, -1],
                                  [-1, -1, -1, -1, 0, -1, -1, -1], [-1, -1, -1, -1, -1, 0, 1, -1],
                                  [-1] * 8, [0, 1, 2, -1, 3, -1, -1, -1]]
    assert t["hops"].tolist() == [[0, 2, 1, 1, -1, -1, -1, -1], [-1, -1, -1, 0, -1, -1, -1, -1],
                                  [3, 2, 1, 4, 0, -1, -1, -1], [-1, -1, -1, -1, -1, 0, 1, -1],
                                  [-1] * 8, [0, 2, 1, 1, -1, -1, -1, -1]]
    assert f["reached"].tolist() == [4, 5, 1, 2, 0, 4] and f["ecc"].tolist() == [3, 4, 0, 1, -1, 3]
    assert f["sum_hops"].tolist() == [6, 10, 0, 1, 0, 6]
    assert f["seen"].tolist() == [0b100011, 0b100011, 0b100011, 0b000010, 0b100111, 0b001000, 0b001000, 0]
    assert f["level_sizes"][1].tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and not f["level_sizes"][4].any()
    assert _expected(FROM, 2)["level_sizes"].tolist() == [[1, 1], [1, 1], [1, 0], [1, 1], [0, 0], [1, 1]]
    assert f["info"] == {"tick": 4, "n": 8, "age_limit": 9, "direction": FROM, "alive": 7, "n_sources": 6,
                         "alive_sources": 5, "depth": 4, "levels": 5, "reserved": 0, "pairs": 16,
                         "sum_hops": 23}
    assert t["info"]["pairs"] == 4 + 1 + 5 + 2 + 4 and t["info"]["depth"] == 4
    assert rm.distinct_sets(f) == 4 and rm.component_sizes(f, t).tolist() == [3, 1, 1, 2, 0, 3]


def test_summary():
    s = _result(_expected(FROM)).summary()
    assert s == {"tick": 4, "direction": "from", "alive": 7, "sources": 6, "alive_sources": 5,
                 "mean_hops": 23 / 16, "diameter_bound": 4, "reached_min": 1, "reached_median": 4.0,
                 "reached_max": 5, "distinct_sets": 4}
    e = _expected(TO)
    none = ReachMulti(4, [7], np.zeros(N, np.uint64), None, [0], [-1], [0], np.zeros((1, 4)), STATE,
                      {"direction": TO})
    assert none.summary() == {"tick": 4, "direction": "to", "alive": 7, "sources": 1, "alive_sources": 0,
                              "mean_hops": 0.0, "diameter_bound": -1, "reached_min": 0,
                              "reached_median": 0.0, "reached_max": 0, "distinct_sets": 0}
    assert _result(e).summary()["distinct_sets"] == 4


def test_bowtie():
    frm, to = _result(_expected(FROM)), _result(_expected(TO))
    b = bowtie(frm, to)
    assert b["scc"].tolist() == [3, 1, 1, 2, 0, 3]
    assert b["downstream"].tolist() == [1, 4, 0, 0, 0, 1]        # 4 below the cycle; all below 3
    assert b["upstream"].tolist() == [1, 0, 4, 0, 0, 1]          # 3 above the cycle; all above 4
    assert b["neither"].tolist() == [2, 2, 2, 5, 7, 2]
    same = b["same"]
    assert same[0, 5] and same[5, 0] and same[3, 3]              # the two bits of node 0; 5 with itself
    assert not same[0, 1] and not same[0, 2] and not same[0, 3] and not same[4].any()
    for bad in ((to, frm), (frm, frm)):
        try:
            bowtie(*bad)
        except ValueError:
            continue
        raise AssertionError("bowtie accepted two results of the wrong directions")
