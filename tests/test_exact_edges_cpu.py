"""The exact-engine edge workloads reach their edges (CPU only: the restatement alone).

tests/test_exact_edges_gpu.py compares the engine with the restatement's record of every workload
of tests/exact_edges.py.  That says nothing unless the record really contains the edge the
workload is named for; each test here proves one from the restatement's own output -- and, for
the MSG_DROP_PROB edges, from the reference's fixtures.  Nothing here runs the engine.
"""
import math
import re

import pytest

from tests import exact_edges as xe
from tests.oracle_binding import golden_edge

ORACLE_SECONDS = 5.0     # the bound the scale engines' edge workloads keep


def _names(prefix):
    return [n for n in xe.WORKLOADS if n.startswith(prefix)]


@pytest.mark.parametrize("name", list(xe.WORKLOADS))
def test_oracle_run_is_quick(name):
    ref = xe.reference(name)
    print("%s: restatement %.2f s, %d merges" % (name, ref["seconds"], ref["merges"]))
    assert ref["seconds"] < ORACLE_SECONDS, "%s: %.1f s" % (name, ref["seconds"])


@pytest.mark.parametrize("name", list(xe.WORKLOADS))
def test_workload_lies_inside_the_admitted_box(name):
    """Every parameter a workload sets is one gsp_create admits (include/gossip/gossip.h)."""
    w = xe.WORKLOADS[name]
    assert 1 <= xe.nodes(name) <= 1024 and 1 <= w["ticks"] <= 3600
    assert 0 <= w.get("intro_list", 0) <= 16
    for field, value in w["params"].items():
        lo, hi = xe.BOX[field]
        assert math.isfinite(value) and lo <= value <= hi, (field, value)
    with open(xe.conf_file(name)) as f:
        prob = float(re.search(r"MSG_DROP_PROB: (\S+)", f.read()).group(1))
    assert 0.0 <= prob <= 1.0


@pytest.mark.parametrize("name", _names("nofilter_"))
def test_nofilter_lists_fill_and_shrink(name):
    """With the payload filter lifted some node holds all the other N - 1 nodes, and entries are
    removed after the failure."""
    ref = xe.reference(name)
    assert max(xe.list_lengths(xe.read(ref, "state.txt")).values()) == ref["n"] - 1
    assert xe.log_lines(xe.read(ref, "dbg.log"), b"removed")


def test_n129_buf_fills_the_buffer():
    assert xe.reference("nofilter_n129_buf")["buffer_full_rejects"] > 0


@pytest.mark.parametrize("name", _names("tr"))
def test_small_tremove_removes_again_and_again(name):
    ref = xe.reference(name)
    assert len(xe.log_lines(xe.read(ref, "dbg.log"), b"removed")) > ref["n"]


@pytest.mark.parametrize("name", _names("buf"))
def test_small_buffer_rejects_from_the_first_ticks(name, tmp_path):
    """Buffer-full rejections before t = 10: counted over a run of the same workload that ends
    there (ticks 0..9)."""
    w = xe.WORKLOADS[name]
    _, _, rejects, _ = xe.run_restatement(xe.conf_file(name), w["seed"], w["mode"], str(tmp_path),
                                          10, **w["params"])
    assert rejects > 0
    assert xe.reference(name)["buffer_full_rejects"] > rejects


def test_msg56_rejects_every_send_and_msg57_none(tmp_path):
    r56, r57 = xe.reference("msg56_n10"), xe.reference("msg57_n10")
    mc = xe.read(r56, "msgcount.log").decode()
    assert [int(x) for x in re.findall(r"sent_total\s+(\d+)", mc)] == [0] * 10
    assert not xe.log_lines(xe.read(r56, "dbg.log"), b"joined")
    assert r56["buffer_full_rejects"] == 0       # the size rule is not a buffer-full rejection
    w = xe.WORKLOADS["msg57_n10"]
    paths, _, _, _ = xe.run_restatement(xe.conf_file("msg57_n10"), w["seed"], w["mode"],
                                        str(tmp_path), w["ticks"])     # max_msg_size 4000
    with open(paths["dbg.log"], "rb") as f:
        assert f.read() == xe.read(r57, "dbg.log")
    assert xe.log_lines(xe.read(r57, "dbg.log"), b"joined")


@pytest.mark.parametrize("name", _names("step0_"))
def test_step0_introducer_answers_everyone_in_one_tick(name):
    ref = xe.reference(name)
    assert xe.sent_per_tick(xe.read(ref, "msgcount.log"), 1)[1] >= ref["n"] - 1
    assert set(xe.log_lines(xe.read(ref, "dbg.log"), b"Trying to join")) == {0}


def test_step_rates_past_the_reference():
    """step1_n40: node i starts at t = i, one join in every tick 1..39 (its last at t = 39, so
    step_rate 1.0 cannot put a join of 40 nodes after the failure).  step3_n40: node i starts at
    t = 3 i, with joins later than the failure at t = 100."""
    joins = xe.log_lines(xe.read(xe.reference("step1_n40"), "dbg.log"), b"Trying to join")
    assert sorted(joins) == list(range(1, 40))
    joins = xe.log_lines(xe.read(xe.reference("step3_n40"), "dbg.log"), b"Trying to join")
    assert sorted(joins) == list(range(3, 120, 3)) and max(joins) > 100


def test_n1024_default_joins_fails_and_removes():
    ref = xe.reference("n1024_default")
    dbg = xe.read(ref, "dbg.log")
    assert max(xe.log_lines(dbg, b"Trying to join")) == 255
    assert len(xe.log_lines(dbg, b"Node failed at time")) == 512
    # the victims' entries leave from t = 120 on (dropped messages remove a few earlier)
    removed = xe.log_lines(dbg, b"removed")
    assert sum(t >= 120 for t in removed) > 512
    # ids past the reference's MAX_NODES are in the run
    assert b" 0.4.0.0:0 [255] Trying to join..." in dbg


def test_drop100_drops_every_send_of_the_window():
    """From the reference's own fixture: MSG_DROP_PROB 1.0 gives the threshold 100, so no send
    of ticks 51..300 is admitted."""
    for mode in ("glibc", "philox"):
        mc = golden_edge(mode, "n10_drop100", 3, "msgcount.log")
        for node in range(1, 11):
            sent = xe.sent_per_tick(mc, node)
            assert len(sent) == 700 and sum(sent[51:301]) == 0 and sum(sent[:51]) > 0
    mc0 = golden_edge("glibc", "n10_drop0", 3, "msgcount.log")
    assert all(sum(xe.sent_per_tick(mc0, node)[51:301]) > 0 for node in range(1, 11))


@pytest.mark.parametrize("mode", ["glibc", "philox"])
def test_drop029_truncates_to_28(tmp_path, mode):
    """(int)(0.29 * 100) is 28 (EmulNet.cpp:92).  Checked against the reference's fixture at
    0.29: dbg.log and msgcount.log equal the restatement's run at 0.28 (threshold 28) byte for
    byte, and msgcount.log differs from its runs at 0.295 (threshold 29, what rounding 0.29 up
    would give) and at 0.30 (threshold 30)."""
    want = {f: golden_edge(mode, "n10_drop029", 3, f) for f in ("dbg.log", "msgcount.log")}
    got = {}
    for prob in ("0.28", "0.295", "0.30"):
        conf = xe.write_conf("n10_drop" + prob.replace(".", ""), (10, 1, 1, prob))
        paths, _, _, _ = xe.run_restatement(conf, 3, mode, str(tmp_path / prob), 700)
        got[prob] = {}
        for f in want:
            with open(paths[f], "rb") as fh:
                got[prob][f] = fh.read()
    assert got["0.28"] == want
    assert got["0.295"]["msgcount.log"] != want["msgcount.log"]
    assert got["0.30"]["msgcount.log"] != want["msgcount.log"]


def test_n513_alias_takes_messages_that_lingered(tmp_path):
    """n513_multi: id 256 fails at t = 100 while id 512, its strcmp() alias (EmulNet.cpp:154),
    starts only at t = 127; from t = 128 node 512 takes the messages that lingered for 256 since
    t = 100 -- GOSSIPs whose senders have changed their lists many times since.  The engine has to
    merge the list as it was sent; read from the restatement's handling-order trace."""
    from tests.oracle_binding import load_oracle
    w = xe.WORKLOADS["n513_multi"]
    L = load_oracle()
    trace = str(tmp_path / "trace.txt")
    L.gsp_oracle_mp1_set_queue_trace(trace.encode())
    try:
        xe.run_restatement(xe.conf_file("n513_multi"), w["seed"], w["mode"], str(tmp_path),
                           w["ticks"])
    finally:
        L.gsp_oracle_mp1_set_queue_trace(None)
    late = set()
    with open(trace) as f:
        for line in f:
            t, receiver, _, kind, sent = map(int, line.split())
            if kind == 3 and sent < t - 1:
                late.add((t, receiver))
    assert late == {(128, 512)}
