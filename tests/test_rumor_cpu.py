"""Rumor trace without a GPU: the struct mirror, the exported names, the declarations in
gossip.h, Rumor.summary() on hand-made arrays, and the numpy rule (tests/rumor_oracle.py) on a
hand-made 6-node message list that shows each clause of the rule by itself."""
import ctypes
import os

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.census import ALIVE, CRASHED, NOT_STARTED
from gossip_protocol_amd.rumor import Rumor
from tests import rumor_oracle as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [e + "_rumor_" + f for e in ("gsp_scale", "gsp_pview") for f in ("open", "seed", "get", "close")]
NEVER = 2 ** 31 - 1


def test_rumor_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_rumor_info") == ctypes.sizeof(_lib.GspRumorInfo)
    assert ctypes.sizeof(_lib.GspRumorInfo) == 48


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    assert len(NAMES) == 8
    for name in NAMES:
        assert name in _lib.SIGNATURES
        args = {"open": (1,), "seed": (0, None, 0), "get": (0, None, None, None, 0, None),
                "close": ()}[name.rsplit("_", 1)[1]]
        rc = getattr(L, name)(None, *args)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for e in ("scale", "pview"):
        for decl in ("int gsp_%s_rumor_open(gsp_%s *s, int32_t rumors);",
                     "int gsp_%s_rumor_seed(gsp_%s *s, int32_t rumor, const int32_t *sources, int32_t n_sources);",
                     "int gsp_%s_rumor_get(gsp_%s *s, int32_t rumor, int32_t *heard, uint8_t *state,",
                     "int gsp_%s_rumor_close(gsp_%s *s);"):
            assert decl % (e, e) in text, decl % (e, e)
    assert "} gsp_rumor_info;" in text
    assert "#define GSP_ABI_VERSION 7" in text


def test_summary_nobody_heard():
    state = np.array([ALIVE, ALIVE, CRASHED, NOT_STARTED], np.uint8)
    r = Rumor(5, np.full(4, -1), state, np.zeros(6), {"seed_tick": -1, "sources": 0})
    assert r.heard.dtype == np.int32 and r.known.dtype == np.int32
    assert r.summary() == {"tick": 5, "seed_tick": -1, "sources": 0, "alive": 2, "known": 0,
                           "known_alive": 0, "unknown_alive": 2, "last_heard": -1,
                           "latency_p50": None, "latency_p90": None, "latency_max": None}
    assert r.coverage().tolist() == [0] * 6


def test_summary_latencies():
    # seeded at tick 2 at node 0; node 4 heard and then crashed, node 5 is alive and never heard
    heard = np.array([2, 3, 3, 4, 5, -1, 9, -1])
    state = np.array([ALIVE] * 4 + [CRASHED, ALIVE, ALIVE, NOT_STARTED], np.uint8)
    known = np.bincount(heard[heard >= 0], minlength=11)
    r = Rumor(10, heard, state, known, {"seed_tick": 2, "sources": 1})
    # latencies 0 1 1 2 3 7: p50 = 3rd of 6 = 1, p90 = 6th of 6 = 7
    assert r.summary() == {"tick": 10, "seed_tick": 2, "sources": 1, "alive": 6, "known": 6,
                           "known_alive": 5, "unknown_alive": 1, "last_heard": 9,
                           "latency_p50": 1, "latency_p90": 7, "latency_max": 7}
    assert r.coverage().tolist() == [0, 0, 1, 3, 4, 5, 5, 5, 5, 6, 6]
    # of the 6 alive now, 5 heard (at 2 3 3 4 9): half by tick 3, 80 % by 9, all never
    assert (r.ticks_to(0.5), r.ticks_to(0.8), r.ticks_to(0.99), r.ticks_to(1.0)) == (1, 7, None, None)


# ---- the rule, 6 nodes ----
START = np.array([0, 0, 0, 0, 0, 3], np.int64)        # node 5 starts at tick 3
FAIL = np.array([NEVER, NEVER, NEVER, 1, NEVER, NEVER], np.int64)   # node 3 runs ticks 0, 1


def _know(**bits):
    k = np.zeros(6, np.uint32)
    for node, mask in bits.items():
        k[int(node[1:])] = mask
    return k


def test_no_second_hop_within_a_tick():
    # 0 -> 1 and 1 -> 2 both merged at tick 1: 2 reads 1's word of tick 0, which is empty
    know, rec = ru.advance(_know(n0=1), 1, [0, 1], [1, 2], [], START, FAIL, 0)
    assert know.tolist() == [1, 1, 0, 0, 0, 0]
    know, _ = ru.advance(know, 2, [1], [2], [], START, FAIL, 0)
    assert know.tolist() == [1, 1, 1, 0, 0, 0]
    assert rec == {"longest": 1, "cut_withheld": 0, "joinrep_carried": 0}


def test_crashed_and_unstarted_receivers_keep_their_mask():
    # node 3 is alive at tick 1 (its crash tick) and not at 2; node 5 has not started at 2
    know, _ = ru.advance(_know(n0=1, n3=2), 1, [0], [3], [], START, FAIL, 0)
    assert know[3] == 3
    know, rec = ru.advance(_know(n0=1, n3=2), 2, [0, 0], [3, 5], [], START, FAIL, 0)
    assert know.tolist() == [1, 0, 0, 2, 0, 0]
    assert rec["cut_withheld"] == 0                  # a dead receiver is no withheld bit


def test_joinrep_sorts_first_and_takes_the_last_inbox_slot():
    # tick 3: node 5 starts and is sent a JOINREP (node 0's word: bit 0) and GOSSIP from 1
    # (bit 1) and 2 (bit 2).  Inbox 2 keeps the JOINREP and sender 1; inbox 1 the JOINREP alone.
    prev = _know(n0=1, n1=2, n2=4)
    know, rec = ru.advance(prev, 3, [2, 1], [5, 5], [5], START, FAIL, 2)
    assert know[5] == 3
    assert rec == {"longest": 3, "cut_withheld": 1, "joinrep_carried": 1}
    know, rec = ru.advance(prev, 3, [2, 1], [5, 5], [5], START, FAIL, 1)
    assert know[5] == 1 and rec["cut_withheld"] == 1
    know, rec = ru.advance(prev, 3, [2, 1], [5, 5], [5], START, FAIL, 0)
    assert know[5] == 7 and rec["cut_withheld"] == 0
    # without the JOINREP inbox 1 keeps sender 1: the JOINREP did take the slot
    know, _ = ru.advance(prev, 3, [2, 1], [5, 5], [], START, FAIL, 1)
    assert know[5] == 2
    # a JOINREP from a node 0 that knows nothing carries nothing
    _, rec = ru.advance(_know(n1=2), 3, [], [], [5], START, FAIL, 0)
    assert rec["joinrep_carried"] == 0


def test_duplicate_and_dead_seeds():
    tr = ru.Trace(6, 2, START, FAIL, 0)
    tr.seed(0, [1, 1, 5])                            # a duplicate; node 5 has not started
    h, state, known, info = tr.snapshot(0)
    assert h.tolist() == [-1, 0, -1, -1, -1, -1] and known.tolist() == [1]
    assert (info["seed_tick"], info["sources"], info["known"], info["alive"]) == (0, 1, 1, 5)
    assert state.tolist() == [ALIVE] * 5 + [NOT_STARTED]
    tr.seed(1, [5])                                  # no alive source: never seeded
    assert tr.snapshot(1)[3]["seed_tick"] == -1 and tr.snapshot(1)[3]["sources"] == 0
    tr.tick([1], [2], [])
    tr.tick([2], [4], [])
    tr.seed(0, [3, 1, 0])                            # tick 2: 3 has crashed, 1 knows already
    h, state, known, info = tr.snapshot(0)
    assert h.tolist() == [2, 0, 1, -1, 2, -1] and known.tolist() == [1, 1, 2]
    assert (info["seed_tick"], info["sources"], info["known"], info["known_alive"]) == (0, 2, 4, 4)
    assert (info["last_heard"], info["ticks_traced"], info["tick"]) == (2, 2, 2)
    assert state[3] == CRASHED
