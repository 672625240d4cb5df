"""The view audit without a GPU: the struct mirror, the argument checks that run before any
device call, and Audit.summary() on hand-made arrays."""
import ctypes

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.audit import Audit, fp
from gossip_protocol_amd.census import ALIVE, CRASHED, NOT_STARTED

KEYS = {"tick", "alive", "classes", "largest_class", "exact", "converged", "views_with_dead",
        "dead_pairs", "missing_pairs", "suspect_pairs", "mean_age", "max_age", "size_min", "size_max"}


def _fp(x):
    """splitmix64 finaliser of one id in Python integers."""
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _print(ids):
    return sum(_fp(x) for x in ids) & ((1 << 64) - 1)


def test_audit_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_audit_info") == ctypes.sizeof(_lib.GspAuditInfo)
    assert ctypes.sizeof(_lib.GspAuditInfo) == 32


def test_null_handle_is_invalid_and_named():
    L = _lib.lib()
    for name in ("gsp_scale_audit", "gsp_pview_audit"):
        rc = getattr(L, name)(None, 9, None, None, None, None, None, None, None, None)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name


def test_fp_is_the_splitmix64_finaliser():
    ids = [0, 1, 2, 3000, 65535, 1048575]
    assert [int(v) for v in fp(np.array(ids))] == [_fp(x) for x in ids]
    assert _fp(0) == 0xE220A8397B1DCDAF          # splitmix64's first output from state 0


def test_summary_two_classes():
    # observer:          0      1      2        3            4
    state = np.array([ALIVE, ALIVE, ALIVE, CRASHED, NOT_STARTED], np.uint8)
    # 0 and 1 hold the true view {0, 1, 2}; 2 still lists the crashed 3 and misses 1
    prints = np.array([_print([0, 1, 2]), _print([0, 1, 2]), _print([0, 2, 3]), 0, 0], np.uint64)
    a = Audit(11, state, size=[2, 2, 2, 0, 0], dead=[0, 0, 1, 0, 0], suspect=[1, 0, 0, 0, 0],
              age_sum=[5, 2, 3, 0, 0], age_max=[4, 2, 3, 0, 0], print=prints,
              info={"tick": 11, "alive": 3})
    assert a.tick == 11 and a.info["alive"] == 3
    s = a.summary()
    assert set(s) == KEYS
    assert s == {"tick": 11, "alive": 3, "classes": 2, "largest_class": 2, "exact": 2,
                 "converged": False, "views_with_dead": 1, "dead_pairs": 1,
                 "missing_pairs": (2 - 2) + (2 - 2) + (2 - 1), "suspect_pairs": 1,
                 "mean_age": (5 + 2 + 3) / 5, "max_age": 4, "size_min": 2, "size_max": 2}
    assert a.print.dtype == np.uint64 and a.age_max.dtype == np.uint8 and a.size.dtype == np.uint32


def test_summary_converged():
    n = 4
    full = Audit(0, np.full(n, ALIVE, np.uint8), np.full(n, 3), np.zeros(n), np.zeros(n), np.zeros(n),
                 np.zeros(n), np.full(n, _print(range(n)), np.uint64))
    assert full.summary() == {"tick": 0, "alive": 4, "classes": 1, "largest_class": 4, "exact": 4,
                              "converged": True, "views_with_dead": 0, "dead_pairs": 0,
                              "missing_pairs": 0, "suspect_pairs": 0, "mean_age": 0.0, "max_age": 0,
                              "size_min": 3, "size_max": 3}


def test_summary_ignores_rows_that_are_not_alive_and_survives_none():
    # a crashed row's arrays are 0 by contract; a nonzero print there must not make a class
    state = np.array([ALIVE, CRASHED], np.uint8)
    a = Audit(3, state, [0, 7], [0, 7], [0, 0], [0, 0], [0, 0],
              np.array([_print([0]), 12345], np.uint64))
    s = a.summary()
    assert s["classes"] == 1 and s["exact"] == 1 and s["converged"] and s["dead_pairs"] == 0
    assert s["size_min"] == 0 and s["size_max"] == 0 and s["mean_age"] == 0.0
    none = Audit(0, np.zeros(3, np.uint8), *([np.zeros(3)] * 6)).summary()
    assert set(none) == KEYS and none["alive"] == 0 and none["classes"] == 0 and none["converged"]
