"""Overlay clustering without a GPU: the struct mirror, the exported names, the declarations in
gossip.h; tests/cluster_oracle.py and cluster.Cluster on hand-made graphs (a complete digraph, a
directed 3-cycle, a star, one reciprocated pair); the closed forms of tick 0 from the C oracle's
rows; summary() and overlap() on hand-made arrays, the NaN handling below two neighbours included.
"""
import ctypes
import math
import os

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.census import ALIVE, CRASHED
from gossip_protocol_amd.cluster import Cluster
from tests import cluster_oracle as co
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle, ScaleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(n, edges, observers, dead=()):
    """expected() of a hand-made edge list (r, x): the entries of dead rows and for dead members
    are dropped the way reach_oracle.edges_at drops them."""
    state = np.full(n, ALIVE, np.uint8)
    state[list(dead)] = CRASHED
    e = np.array([(r, x) for r, x in edges if state[r] == ALIVE and state[x] == ALIVE], np.int32).reshape(-1, 2)
    a = co.adjacency(n, ro.csr(n, e[:, 0], e[:, 1]))
    want = co.expected(n, 4, state, a, co.counts(a), 9, observers)
    return want, Cluster(4, observers, want["member"], want["degree"], want["links"], want["mutual"], state,
                         want["info"])


def test_cluster_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_cluster_info") == ctypes.sizeof(_lib.GspClusterInfo)
    assert ctypes.sizeof(_lib.GspClusterInfo) == 64
    assert _lib.CLUSTER_MAX_OBSERVERS == 64
    assert [f for f, _ in _lib.GspClusterInfo._fields_ if f != "kernel_ms"] == list(co.INFO)


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    for name in ("gsp_scale_cluster", "gsp_pview_cluster"):
        assert name in _lib.SIGNATURES
        rc = getattr(L, name)(None, 9, None, 0, None, None, None, None, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for decl in ("int gsp_scale_cluster(gsp_scale *s, int32_t age_limit, const int32_t *observers",
                 "int gsp_pview_cluster(gsp_pview *s, int32_t age_limit, const int32_t *observers",
                 "#define GSP_CLUSTER_MAX_OBSERVERS 64", "} gsp_cluster_info;", " * Overlay clustering:"):
        assert decl in text, decl
    assert text.index(" * Multi-source reach:") < text.index(" * Overlay clustering:") < text.index(" * Rumor trace:")


def test_complete_digraph():
    n = 6
    want, c = _graph(n, [(r, x) for r in range(n) for x in range(n) if r != x], list(range(n)))
    assert want["degree"].tolist() == [5] * n and want["links"].tolist() == [20] * n      # k (k - 1)
    assert want["mutual"].tolist() == [5] * n
    assert want["member"].tolist() == [0b111111 & ~(1 << x) for x in range(n)]
    assert c.coefficient.tolist() == [1.0] * n
    s = c.summary()
    assert s["density"] == 1.0 and s["transitivity"] == 1.0 and s["reciprocity"] == 1.0
    assert s["mean_clustering"] == 1.0 and s["clustering_over_density"] == 1.0
    assert want["info"]["rows"] == n and want["info"]["sum_links"] == 120


def test_directed_three_cycle():
    want, c = _graph(3, [(0, 1), (1, 2), (2, 0)], [0, 1, 2])
    assert want["degree"].tolist() == [1, 1, 1] and want["links"].tolist() == [0, 0, 0]
    assert want["mutual"].tolist() == [0, 0, 0]
    assert want["member"].tolist() == [0b100, 0b001, 0b010]
    assert np.isnan(c.coefficient).all()                       # k < 2 everywhere
    s = c.summary()
    assert math.isnan(s["mean_clustering"]) and math.isnan(s["transitivity"])
    assert math.isnan(s["clustering_over_density"])
    assert s["reciprocity"] == 0.0 and s["mean_degree"] == 1.0 and s["density"] == 0.5


def test_star_and_its_closed_rim():
    # the hub 0 lists 1..4 and nobody lists anybody else: a lattice-like zero
    want, c = _graph(5, [(0, x) for x in range(1, 5)], [0, 1])
    assert want["degree"].tolist() == [4, 0] and want["links"].tolist() == [0, 0]
    assert want["mutual"].tolist() == [0, 0]
    assert c.coefficient[0] == 0.0 and math.isnan(c.coefficient[1])
    # the rim closed into a directed ring, 1 listing the hub back: 4 of the hub's 12 ordered
    # pairs, 1 mutual; node 1 lists 2 and the hub, and the hub lists 2: 1 of its 2 pairs
    rim = [(1, 2), (2, 3), (3, 4), (4, 1), (1, 0)]
    want, c = _graph(5, [(0, x) for x in range(1, 5)] + rim, [0, 1, 0])
    assert want["degree"].tolist() == [4, 2, 4] and want["links"].tolist() == [4, 1, 4]
    assert want["mutual"].tolist() == [1, 1, 1]
    assert want["member"].tolist() == [0b010, 0b101, 0b111, 0b101, 0b101]
    assert c.coefficient.tolist() == [4 / 12, 0.5, 4 / 12]
    assert want["info"]["rows"] == 5 and want["info"]["sum_degree"] == 10


def test_reciprocated_pair_and_a_dead_observer():
    # 0 <-> 1; 2 is crashed: its row and the entries for it are no edges, its bit is set nowhere
    want, c = _graph(4, [(0, 1), (1, 0), (2, 0), (0, 2), (3, 0)], [0, 1, 2, 3], dead=[2])
    assert want["degree"].tolist() == [1, 1, 0, 1] and want["links"].tolist() == [0, 0, 0, 0]
    assert want["mutual"].tolist() == [1, 1, 0, 0]
    assert want["member"].tolist() == [0b1010, 0b0001, 0, 0]
    assert want["info"]["alive_observers"] == 3 and want["info"]["alive"] == 3 and want["info"]["rows"] == 2
    s = c.summary()
    assert s["observers"] == 3 and s["reciprocity"] == 2 / 3 and s["mean_degree"] == 1.0
    assert s["density"] == 0.5 and math.isnan(s["mean_clustering"])


def test_edge_set_of_a_hand_made_graph():
    # 0: no neighbour; 1: one; 2 lists 3, 4, 5 who list each other; 6 crashed
    tri = [(3, 4), (4, 5), (5, 3), (4, 3)]
    state = np.array([ALIVE] * 6 + [CRASHED] + [ALIVE], np.uint8)
    e = np.array([(1, 2), (2, 3), (2, 4), (2, 5)] + tri, np.int32)
    a = co.adjacency(8, ro.csr(8, e[:, 0], e[:, 1]))
    ids, slots = co.edge(8, state, co.counts(a))
    assert (ids, slots) == ([0, 1, 2, 6, 2, 7], ["empty", "single", "top", "dead", "again", "last"])


def test_tick_zero_closed_forms_from_the_c_oracle():
    # the partial view starts as a lattice of stride n / V = 128 > 1: no two neighbours of a node
    # are 128 k apart from a neighbour's neighbour, and 1 is no multiple of the stride
    n, view = 4096, 32
    orc = PviewOracle(n, view=view, fanout=3, inbox=7, tremove=9, fail_mode=1, fail_tick=2, fail_ppm=50000,
                      seed=4128)
    state = ro.states(orc, n, 0)
    a = co.adjacency(n, ro.graph(n, 0, ro.edges_at(orc, n, state, True), 32, ro.FROM))
    orc.close()
    degree, links, mutual = co.counts(a)
    assert (degree == view).all() and not links.any() and not mutual.any()
    assert co.mean_clustering(state, (degree, links, mutual))[0] == 0.0
    # the full view starts complete
    n = 600
    orc = ScaleOracle(n, fanout=3, tremove=9, fail_mode=1, fail_tick=2, fail_ppm=20000, seed=600)
    state = ro.states(orc, n, 0)
    a = co.adjacency(n, ro.graph(n, 0, ro.edges_at(orc, n, state, False), 32, ro.FROM))
    orc.close()
    degree, links, mutual = co.counts(a)
    assert (degree == n - 1).all() and (links == (n - 1) * (n - 2)).all() and (mutual == n - 1).all()
    want = co.expected(n, 0, state, a, (degree, links, mutual), 32, [0, n - 1])
    assert want["info"]["rows"] == n and want["info"]["sum_links"] == 2 * (n - 1) * (n - 2)
    assert want["member"][0] == 2 and want["member"][n - 1] == 1 and (want["member"][1:n - 1] == 3).all()


def test_summary_on_hand_made_arrays():
    state = np.array([ALIVE] * 9 + [CRASHED], np.uint8)
    member = np.zeros(10, np.uint64)
    # observers 0 (k = 4, 6 links, 2 mutual), 1 (k = 1), 9 (crashed), 2 (k = 2, 2 links, 1 mutual)
    c = Cluster(7, [0, 1, 9, 2], member, [4, 1, 0, 2], [6, 0, 0, 2], [2, 0, 0, 1], state)
    assert c.live.tolist() == [True, True, False, True]
    coef = c.coefficient
    assert coef[0] == 0.5 and math.isnan(coef[1]) and math.isnan(coef[2]) and coef[3] == 1.0
    assert coef.dtype == np.float64
    s = c.summary()
    assert s == {"tick": 7, "alive": 9, "observers": 3, "mean_degree": 7 / 3, "density": 7 / 3 / 8,
                 "mean_clustering": 0.75, "transitivity": 8 / 14, "reciprocity": 3 / 7,
                 "clustering_over_density": 0.75 / (7 / 3 / 8)}
    none = Cluster(7, [9], member, [0], [0], [0], state).summary()
    assert none["observers"] == 0 and all(math.isnan(none[f]) for f in (
        "mean_degree", "density", "mean_clustering", "transitivity", "reciprocity", "clustering_over_density"))
    big = Cluster(0, [0], member, [65535], [65535 * 65534], [0], state)      # links past 2^32
    assert big.links.dtype == np.uint64 and big.coefficient[0] == 1.0 and big.summary()["transitivity"] == 1.0


def test_overlap_on_hand_made_arrays():
    state = np.array([ALIVE] * 7 + [CRASHED], np.uint8)
    # bit 0 (node 0): {1, 2, 3}; bit 1 (node 4): {2, 3, 5}; bit 2 (node 7, crashed): nothing;
    # bit 3 (node 0 again): {1, 2, 3}; bit 4 (node 6): nothing
    member = np.array([0, 0b01001, 0b01011, 0b01011, 0, 0b00010, 0, 0], np.uint64)
    c = Cluster(3, [0, 4, 7, 0, 6], member, [3, 3, 0, 3, 0], [0] * 5, [0] * 5, state)
    inter, jac = c.overlap()
    assert inter.tolist() == [[3, 2, 0, 3, 0], [2, 3, 0, 2, 0], [0] * 5, [3, 2, 0, 3, 0], [0] * 5]
    # distinct alive pairs with a non-empty union: (0,1) 2/4, (0,4) 0/3, (1,3) 2/4, (1,4) 0/3, (3,4) 0/3
    assert jac == (0.5 + 0 + 0.5 + 0 + 0) / 5
    _, lone = Cluster(3, [0, 7], member, [3, 0], [0, 0], [0, 0], state).overlap()
    assert math.isnan(lone)
