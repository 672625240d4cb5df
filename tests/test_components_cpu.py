"""Overlay components without a GPU: the struct mirror, the exported names, the declarations in
gossip.h; tests/components_oracle.py on hand-made graphs (two cycles joined by one edge, a
descending chain, an isolated node, a dead node between two parts) and, where scipy is installed,
against scipy.sparse.csgraph on the C oracle's rows; components.Components on fixed label arrays.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from gossip_protocol_amd import _lib
from gossip_protocol_amd import components as comps
from gossip_protocol_amd.census import ALIVE, CRASHED
from gossip_protocol_amd.components import Components
from tests import components_oracle as co
from tests import reach_oracle as ro
from tests.oracle_binding import PviewOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(n, edges, dead=()):
    """(weak, strong) expected() of a hand-made edge list (r, x), all entries stamped at the
    tick: the entries of dead rows and for dead members are dropped as reach_oracle.edges_at
    drops them."""
    state = np.full(n, ALIVE, np.uint8)
    state[list(dead)] = CRASHED
    e = np.array([(r, x) for r, x in edges if state[r] == ALIVE and state[x] == ALIVE], np.int32).reshape(-1, 2)
    packed = (e[:, 0], e[:, 1], np.full(e.shape[0], 4, np.int32), 0)
    return tuple(co.expected(n, 4, state, packed, 1, kind) for kind in (co.WEAK, co.STRONG)) + (packed,)


def test_components_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_components_info") == ctypes.sizeof(_lib.GspComponentsInfo)
    assert ctypes.sizeof(_lib.GspComponentsInfo) == 56
    assert (_lib.COMPONENTS_WEAK, _lib.COMPONENTS_STRONG) == (0, 1) == (co.WEAK, co.STRONG)
    fields = [f for f, _ in _lib.GspComponentsInfo._fields_]
    assert [f for f in fields if f not in ("kernel_ms", "sweeps", "rounds")] == list(co.INFO)
    assert fields[-1] == "kernel_ms" and fields[9:11] == ["sweeps", "rounds"]


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    for name in ("gsp_scale_components", "gsp_pview_components"):
        assert name in _lib.SIGNATURES
        rc = getattr(L, name)(None, 1, 9, 0, None, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for decl in ("int gsp_scale_components(gsp_scale *s, int32_t kind, int32_t age_limit, int32_t max_sweeps",
                 "int gsp_pview_components(gsp_pview *s, int32_t kind, int32_t age_limit, int32_t max_sweeps",
                 "#define GSP_COMPONENTS_WEAK   0", "#define GSP_COMPONENTS_STRONG 1",
                 "#define GSP_COMPONENTS_DEFAULT_SWEEPS %d" % _lib.COMPONENTS_DEFAULT_SWEEPS,
                 "} gsp_components_info;", " * Overlay components:", "#define GSP_ABI_VERSION 7"):
        assert decl in text, decl
    assert text.index(" * Overlay clustering:") < text.index(" * Overlay components:") < text.index(" * Rumor trace:")


def test_two_cycles_joined_by_one_edge():
    # 5 -> 6 -> 7 -> 5 and 1 -> 2 -> 3 -> 1, joined by 7 -> 1 alone; 0 and 4 list nobody
    weak, strong, packed = _graph(8, [(5, 6), (6, 7), (7, 5), (1, 2), (2, 3), (3, 1), (7, 1)])
    assert weak["label"].tolist() == [0, 1, 1, 1, 4, 1, 1, 1]
    assert strong["label"].tolist() == [0, 1, 1, 1, 4, 5, 5, 5]
    assert weak["info"]["components"] == 3 and weak["info"]["largest"] == 6 and weak["info"]["singletons"] == 2
    assert strong["info"]["components"] == 4 and strong["info"]["largest"] == 3
    assert strong["info"]["largest_label"] == 1                       # the smaller label of the two 3s
    assert co.depth(8, 4, packed, 1, strong["label"]) == 2


def test_descending_chain():
    n = 7
    weak, strong, packed = _graph(n, [(x, x - 1) for x in range(n - 1, 0, -1)])
    assert weak["label"].tolist() == [0] * n
    assert strong["label"].tolist() == list(range(n)) and strong["info"]["singletons"] == n
    assert co.depth(n, 4, packed, 1, strong["label"]) == n
    # closed into a ring it is one strong component
    _, ring, packed = _graph(n, [(x, x - 1) for x in range(n - 1, 0, -1)] + [(0, n - 1)])
    assert ring["label"].tolist() == [0] * n and co.depth(n, 4, packed, 1, ring["label"]) == 1


def test_isolated_node_and_self_loop():
    weak, strong, _ = _graph(4, [(0, 1), (1, 0), (3, 3)])
    assert weak["label"].tolist() == [0, 0, 2, 3] == strong["label"].tolist()
    assert weak["info"]["singletons"] == 2 and weak["info"]["largest_label"] == 0


def test_dead_node_between_two_parts():
    # 0 <-> 1 <-> 2 <-> 3 <-> 4 with 2 crashed: its row and the entries for it are no edges
    ring = [(x, x + 1) for x in range(4)] + [(x + 1, x) for x in range(4)]
    weak, strong, _ = _graph(5, ring, dead=[2])
    assert weak["label"].tolist() == [0, 0, -1, 3, 3] == strong["label"].tolist()
    assert weak["info"]["alive"] == 4 and weak["info"]["components"] == 2
    alive, _, _ = _graph(5, ring)
    assert alive["label"].tolist() == [0] * 5
    none, _, _ = _graph(3, [(0, 1)], dead=[0, 1, 2])
    assert none["label"].tolist() == [-1] * 3
    assert none["info"]["components"] == 0 and none["info"]["largest"] == 0 and none["info"]["largest_label"] == -1


def test_age_limit_is_the_reach_rule():
    """(t - ts) mod 32 < age_limit, past the wrap too."""
    state = np.full(3, ALIVE, np.uint8)
    edges = (np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([33, 30], np.int32), 0)
    assert co.expected(3, 33, state, edges, 1, co.WEAK)["label"].tolist() == [0, 0, 2]
    assert co.expected(3, 33, state, edges, 3, co.WEAK)["label"].tolist() == [0, 0, 2]
    assert co.expected(3, 33, state, edges, 4, co.WEAK)["label"].tolist() == [0, 0, 0]
    assert co.expected(3, 33 + 32, state, edges, 4, co.WEAK)["label"].tolist() == [0, 0, 0]


def test_oracle_against_scipy_on_a_fragmented_overlay():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    n, t = 512, 3
    orc = PviewOracle(n, view=8, fanout=1, inbox=0, tremove=9, fail_mode=2, fail_tick=0, fail_ppm=100000, seed=77)
    for _ in range(t):
        orc.step()
    state = ro.states(orc, n, t)
    edges = ro.edges_at(orc, n, state, True)
    orc.close()
    r, x = co.pairs(t, edges, 1)
    g = sparse.csr_matrix((np.ones(r.size), (r, x)), shape=(n, n))
    live = state == ALIVE
    for kind, conn in ((co.WEAK, "weak"), (co.STRONG, "strong")):
        want = co.expected(n, t, state, edges, 1, kind)
        _, lab = csgraph.connected_components(g, directed=True, connection=conn)
        smallest = np.full(lab.max() + 1, n)
        np.minimum.at(smallest, lab[live], np.nonzero(live)[0])
        assert np.array_equal(want["label"][live], smallest[lab[live]]), conn
        assert (want["label"][~live] == -1).all()
        assert want["info"]["components"] > 20, conn                 # it does fragment


def _fixed():
    #        0  1  2   3  4  5  6  7  8  9
    state = np.array([1, 1, 1, 2, 1, 1, 1, 1, 0, 1], np.uint8)
    strong = np.array([0, 0, 2, -1, 2, 5, 6, 0, -1, 9], np.int32)
    weak = np.array([0, 0, 0, -1, 0, 5, 5, 0, -1, 9], np.int32)
    return Components(7, "strong", strong, state), Components(7, "weak", weak, state)


def test_sizes_of_and_summary():
    strong, weak = _fixed()
    labels, sizes = strong.sizes()
    assert labels.tolist() == [0, 2, 5, 6, 9] and sizes.tolist() == [3, 2, 1, 1, 1]
    assert strong.of(7).tolist() == [0, 1, 7] and strong.of(4).tolist() == [2, 4]
    assert strong.of(3).size == 0 and strong.of(8).size == 0          # crashed, not started
    s = strong.summary()
    assert (s["components"], s["giant"], s["giant_label"], s["singletons"], s["nontrivial"]) == (5, 3, 0, 3, 2)
    assert s["alive"] == 8 and s["giant_share"] == 3 / 8 and s["histogram"] == [3, 2] and s["kind"] == "strong"
    w = weak.summary()
    assert (w["components"], w["giant"], w["singletons"], w["nontrivial"], w["histogram"]) == (3, 5, 1, 2, [1, 1, 1])
    empty = Components(0, "weak", np.full(3, -1, np.int32), np.zeros(3, np.uint8)).summary()
    assert empty["components"] == 0 and empty["giant"] == 0 and math.isnan(empty["giant_share"])
    assert empty["histogram"] == []


def test_not_converged_raises():
    c = Components(3, "strong", np.arange(4, dtype=np.int32), np.ones(4, np.uint8), {"converged": 0}, converged=False)
    for call in (c.summary, c.sizes, lambda: c.of(0)):
        with pytest.raises(ValueError, match="did not converge"):
            call()


def test_nesting():
    strong, weak = _fixed()
    labels, counts = comps.nesting(strong, weak)
    assert labels.tolist() == [0, 5, 9] and counts.tolist() == [2, 2, 1]
    assert Components.nesting(strong, weak)[1].tolist() == [2, 2, 1]
    with pytest.raises(ValueError, match="two weak"):
        comps.nesting(weak, strong)                                   # a "strong" part across two "weak" ones
    other = Components(7, "weak", np.where(weak.label >= 0, 0, -1).astype(np.int32), weak.state)
    assert comps.nesting(strong, other)[1].tolist() == [5]
    shifted = Components(7, "weak", np.roll(weak.label, 1), weak.state)
    with pytest.raises(ValueError, match="same nodes"):
        comps.nesting(strong, shifted)
