"""Detection ledger without a GPU: the struct mirror, the exported names, the declarations in
gossip.h, Detect.summary() on hand-made arrays, and the numpy rule (tests/detect_oracle.py) on a
hand-made record list that shows each clause of the rule by itself."""
import ctypes
import os

import numpy as np

from gossip_protocol_amd import _lib
from gossip_protocol_amd.detect import Detect
from tests import detect_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [e + "_detect_" + f for e in ("gsp_scale", "gsp_pview") for f in ("open", "get", "close")]
NEVER = 2 ** 31 - 1


def test_detect_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_detect_info") == ctypes.sizeof(_lib.GspDetectInfo)
    assert ctypes.sizeof(_lib.GspDetectInfo) == 88


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    assert len(NAMES) == 6
    for name in NAMES:
        assert name in _lib.SIGNATURES
        args = (None,) * 9 + (0, None) if name.endswith("_get") else ()
        rc = getattr(L, name)(None, *args)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for e in ("scale", "pview"):
        for decl in ("int gsp_%s_detect_open(gsp_%s *s);",
                     "int gsp_%s_detect_get(gsp_%s *s, int32_t *first_remove, int32_t *last_remove,",
                     "int gsp_%s_detect_close(gsp_%s *s);"):
            assert decl % (e, e) in text, decl % (e, e)
    assert "} gsp_detect_info;" in text
    assert "#define GSP_ABI_VERSION 7" in text


def _detect(tick, crash, **kw):
    n = len(crash)
    arr = dict(first_remove=np.full(n, -1), last_remove=np.full(n, -1), removers=np.zeros(n),
               false_removes=np.zeros(n), first_false=np.full(n, -1), revivals=np.zeros(n),
               evicts=np.zeros(n))
    info = kw.pop("info", None)
    arr.update(kw)
    return Detect(tick, crash, info=info, **arr)


def test_summary_nobody_crashed():
    d = _detect(20, [NEVER] * 4, false_removes=[0, 2, 0, 1], first_false=[-1, 7, -1, 9])
    assert d.first_remove.dtype == np.int32 and d.removers.dtype == np.uint32
    assert d.summary() == {
        "tick": 20, "crashed_nodes": 0, "crashed_nodes_detected": 0, "removes_per_detected_node": 0.0,
        "removes_of_live_nodes": 3, "first_detection_latency_ticks": None,
        "full_detection_latency_ticks": None, "revived_nodes": 0, "revivals": 0,
        "falsely_removed_nodes": 2, "lost": 0}


def test_summary_nothing_detected():
    # 1 and 2 crashed before tick 12 and nobody has removed them yet; 3 crashes at 12 (not < 12)
    d = _detect(12, [NEVER, 5, 9, 12], false_removes=[0, 1, 0, 4], info={"lost": 7})
    s = d.summary()
    assert (s["crashed_nodes"], s["crashed_nodes_detected"]) == (2, 0)
    assert s["removes_per_detected_node"] == 0.0 and s["first_detection_latency_ticks"] is None
    assert s["full_detection_latency_ticks"] is None
    assert s["removes_of_live_nodes"] == 4           # member 3 only: 1 crashed before the tick
    assert s["falsely_removed_nodes"] == 2 and s["lost"] == 7


def test_summary_latencies():
    # crash 4: removed at 13..16 by 5; crash 6: removed at 16..20 by 3 and revived twice; member 3
    # crashed at 30, after the tick: its removes do not count as detection
    d = _detect(25, [NEVER, 4, 6, 30], first_remove=[-1, 13, 16, -1], last_remove=[-1, 16, 20, -1],
                removers=[0, 5, 3, 0], false_removes=[1, 0, 2, 6], revivals=[0, 0, 2, 0])
    assert d.summary() == {
        "tick": 25, "crashed_nodes": 2, "crashed_nodes_detected": 2, "removes_per_detected_node": 4.0,
        "removes_of_live_nodes": 7,
        "first_detection_latency_ticks": {"min": 9, "mean": 9.5, "max": 10},
        "full_detection_latency_ticks": {"min": 12, "mean": 13.0, "max": 14},
        "revived_nodes": 1, "revivals": 2, "falsely_removed_nodes": 3, "lost": 0}


def _led(crash, span=12, kinds=14):
    n = len(crash)
    return do.Ledger(n, np.zeros(n), crash, span, kinds=kinds)


def test_rule_remove_at_the_crash_tick_is_false():
    led = _led([5, NEVER])
    led.fold([2, 2], [5, 6], [0, 0])                 # t == crash: alive; crash + 1: true
    s = led.snapshot(6)
    assert (s["false_removes"][0], s["first_false"][0]) == (1, 5)
    assert (s["removers"][0], s["first_remove"][0], s["last_remove"][0]) == (1, 6, 6)
    assert s["by_tick"][5].tolist() == [0, 1, 0, 0] and s["by_tick"][6].tolist() == [1, 0, 0, 0]
    assert s["first_remove"][1] == -1 and s["first_false"][1] == -1 and s["last_remove"][1] == -1
    assert s["state"].tolist() == [2, 1]


def test_rule_revival_and_evict():
    led = _led([3, NEVER, NEVER])
    led.fold([1, 1, 1, 3, 3], [3, 4, 4, 4, 9], [0, 0, 1, 2, 2])
    s = led.snapshot(9)
    assert s["revivals"].tolist() == [1, 0, 0]       # the join at t == crash is no revival
    assert s["evicts"].tolist() == [0, 0, 2]
    assert s["by_tick"][4].tolist() == [0, 0, 1, 1] and s["by_tick"][9].tolist() == [0, 0, 0, 1]
    assert (s["info"]["joins"], s["info"]["revivals"], s["info"]["evicts"], s["info"]["records"]) == (3, 1, 2, 5)


def test_rule_first_and_last_with_repeats():
    led = _led([2, 8])
    led.fold([2] * 7, [9, 7, 7, 11, 9, 4, 3], [0, 0, 0, 0, 0, 1, 1])
    s = led.snapshot(11)
    assert (s["first_remove"][0], s["last_remove"][0], s["removers"][0]) == (7, 11, 5)
    assert (s["first_false"][1], s["false_removes"][1], s["removers"][1]) == (3, 2, 0)
    led.fold([2], [5], [0])                          # a later fold lowers first, keeps last
    s = led.snapshot(11)
    assert (s["first_remove"][0], s["last_remove"][0], s["removers"][0]) == (5, 11, 6)
    assert s["info"]["true_removes"] == 6 and s["info"]["false_removes"] == 2


def test_rule_unrecorded_kinds_count_nothing():
    led = _led([2, NEVER], kinds=4)                  # removes only
    led.fold([1, 2, 3], [5, 5, 5], [0, 0, 1])
    s = led.snapshot(5)
    assert (s["info"]["records"], s["info"]["joins"], s["info"]["evicts"], s["info"]["revivals"]) == (1, 0, 0, 0)
    assert s["removers"].tolist() == [1, 0]


def test_pack_matches_split_events():
    rec = do.pack([2, 3], [7, 1000], [5, 2 ** 21 - 1], [9, 2 ** 21 - 1])
    k, t, r, x = _lib.split_events(rec)
    assert (k.tolist(), t.tolist(), r.tolist(), x.tolist()) == ([2, 3], [7, 1000], [5, 2 ** 21 - 1], [9, 2 ** 21 - 1])
