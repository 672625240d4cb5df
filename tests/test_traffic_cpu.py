"""Traffic ledger without a GPU: the struct mirror, the exported names and their argument errors,
the declarations in gossip.h, the numpy rule (tests/traffic_oracle.py) on a hand-made case that
shows each clause by itself, the five per-tick identities on every oracle run the GPU tests use
(the oracle alone satisfies them before the GPU is asked), Traffic.summary() on hand-made arrays,
and the msgcount.log writer against every golden file the reference wrote."""
import ctypes
import glob
import gzip
import os
import re

import numpy as np
import pytest

from gossip_protocol_amd import _lib, traffic
from tests import traffic_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [e + "_traffic_" + f for e in ("gsp_scale", "gsp_pview") for f in ("open", "get", "close")]
NEVER = 2 ** 31 - 1


def test_traffic_info_layout():
    assert _lib.lib().gsp_struct_size(b"gsp_traffic_info") == ctypes.sizeof(_lib.GspTrafficInfo)
    assert ctypes.sizeof(_lib.GspTrafficInfo) == 88


def test_names_are_in_signatures_and_exported():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        args = (None,) * 11 + (0, None) if name.endswith("_get") else (None, 0) if name.endswith("_open") else ()
        rc = getattr(L, name)(None, *args)
        assert rc == -1, name
        assert name.encode() in L.gsp_last_error(), name
    assert "gsp_traffic_write_msgcount" in _lib.SIGNATURES
    assert L.gsp_abi_version() == 7


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "gossip", "gossip.h")).read()
    for e in ("scale", "pview"):
        for decl in ("int gsp_%s_traffic_open(gsp_%s *s, const int32_t *watch, int32_t n_watch);",
                     "int gsp_%s_traffic_get(gsp_%s *s, uint32_t *sent, uint32_t *recv, uint32_t *merged,",
                     "int gsp_%s_traffic_close(gsp_%s *s);"):
            assert decl % (e, e) in text, decl % (e, e)
    assert "} gsp_traffic_info;" in text
    assert "int gsp_traffic_write_msgcount(const char *path, const int32_t *sent, const int32_t *recv," in text
    assert "#define GSP_ABI_VERSION 7" in text
    assert "#define GSP_TRAFFIC_BUCKETS %d" % traffic.BUCKETS in text
    assert "#define GSP_TRAFFIC_MAX_WATCH %d" % traffic.MAX_WATCH in text


def test_writer_argument_errors(tmp_path):
    L = _lib.lib()
    one = (ctypes.c_int32 * 1)(0)
    assert L.gsp_traffic_write_msgcount(None, one, one, 1, 1) == -1
    assert L.gsp_traffic_write_msgcount(str(tmp_path / "x").encode(), None, one, 1, 1) == -1
    assert L.gsp_traffic_write_msgcount(str(tmp_path / "x").encode(), one, one, -1, 1) == -1
    assert L.gsp_traffic_write_msgcount(str(tmp_path / "no" / "dir").encode(), one, one, 1, 1) != 0
    assert b"gsp_traffic_write_msgcount" in L.gsp_last_error()


def test_buckets():
    k = [0, 1, 2, 3, 4, 7, 8, 65535, 65536, 131071, 131072, 10 ** 9]
    want = [0, 1, 2, 2, 3, 3, 4, 16, 17, 17, 17, 17]
    assert to.bucket_of(k).tolist() == want
    assert traffic.bucket_of(k).tolist() == want


# Six nodes, inbox 2, intro_list 3.  Node 2 crashes at tick 1 (alive at 1, not at 2); node 5 starts
# at tick 2.  size: what a GOSSIP of each sender carries.
START = np.array([0, 0, 0, 0, 0, 2])
FAIL = np.array([NEVER, NEVER, 1, NEVER, NEVER, NEVER])
SIZE = {0: 5, 1: 4, 2: 3, 3: 2, 4: 1}


def _hand():
    led = to.Ledger(6, START, FAIL, 2, 3, 4, watch=(3, 2, 5))
    # tick 1: 3 is sent four messages (inbox cut: senders 0 and 1 merge), 2 one while still alive,
    # 5 one before it has started (lost); the JOINREP for 5 leaves node 0 at tick 1
    arr = to.arrivals(1, [4, 1, 0, 2, 0, 1], [3, 3, 3, 3, 2, 5], [], START, FAIL, 2)
    led.tick(arr, SIZE, [0, 0, 1, 1, 3], 1)
    # tick 2: the JOINREP reaches 5 (first in its inbox, then sender 0; sender 1 is cut), crashed 2
    # is sent two messages (lost), 3 none
    arr = to.arrivals(2, [1, 0, 3, 1], [5, 5, 2, 2], [5], START, FAIL, 2)
    led.tick(arr, SIZE, [4], 0)
    return led


def test_rule_on_the_hand_made_case():
    s = _hand().snapshot()
    assert s["sent"].tolist() == [3, 2, 0, 1, 1, 0]            # node 0: two GOSSIPs and the JOINREP
    assert s["recv"].tolist() == [0, 0, 1, 4, 0, 3]
    assert s["merged"].tolist() == [0, 0, 1, 2, 0, 2]
    assert s["lost"].tolist() == [0, 0, 2, 0, 0, 1]
    # 3 merges senders 0, 1: (1 + 5) + (1 + 4); 2 merges sender 0: 1 + 5; 5 the JOINREP and 0:
    # (1 + min(3, 5)) + (1 + 5)
    assert s["entries_in"].tolist() == [0, 0, 6, 11, 0, 10]
    assert s["peak_recv"].tolist() == [0, 0, 1, 4, 0, 3]
    assert s["peak_tick"].tolist() == [-1, -1, 1, 1, -1, 2]
    assert s["state"].tolist() == [1, 1, 2, 1, 1, 1]
    assert s["by_tick"].tolist() == [[0] * 6, [6, 5, 3, 1, 17, 4], [1, 3, 2, 2, 10, 3]]
    # tick 1: alive 0..4 -- 0, 1, 4 none, 2 one, 3 four; tick 2: alive 0, 1, 3, 4, 5 -- 5 three
    assert s["fanin"][1].tolist()[:4] == [3, 1, 0, 1] and s["fanin"][2].tolist()[:4] == [4, 0, 1, 0]
    assert s["fanin"].sum() == 10
    assert s["watch"].tolist() == [[[0, 0], [1, 4], [0, 0]], [[0, 0], [0, 1], [0, 0]], [[0, 0], [0, 0], [0, 3]]]
    i = s["info"]
    assert (i["sent"], i["recv"], i["merged"], i["lost"], i["entries"], i["overflow"]) == (7, 8, 5, 3, 27, 3)
    assert (i["max_fanin"], i["max_fanin_node"], i["ticks_counted"], i["n_watch"]) == (4, 3, 2, 3)


def test_rule_ties_keep_the_first_tick_and_the_smallest_id():
    led = to.Ledger(3, np.zeros(3), np.full(3, NEVER), 0, 0, 4)
    led.tick(to.arrivals(1, [0, 0], [1, 2], [], led.start, led.fail, 0), {0: 1}, [], 0)
    led.tick(to.arrivals(2, [0, 0], [1, 2], [], led.start, led.fail, 0), {0: 1}, [], 0)
    s = led.snapshot()
    assert s["peak_tick"].tolist() == [-1, 1, 1] and s["info"]["max_fanin_node"] == 1
    assert s["merged"].tolist() == s["recv"].tolist() == [0, 2, 2]     # K = 0: everything merges


def test_summary():
    s = _hand().snapshot()
    tr = traffic.Traffic(2, s["sent"], s["recv"], s["merged"], s["lost"], s["entries_in"], s["peak_recv"],
                         s["peak_tick"], s["state"], s["by_tick"], s["fanin"], [3, 2, 5], s["watch"], s["info"])
    assert tr.sent.dtype == np.uint32 and tr.entries_in.dtype == np.uint64 and tr.peak_tick.dtype == np.int32
    m = tr.summary(top=2)
    assert (m["sent"], m["recv"], m["merged"], m["lost"], m["entries"], m["overflow"]) == (7, 8, 5, 3, 27, 3)
    assert m["alive_node_rounds"] == 10
    assert m["messages_per_alive_node_round"] == 0.8 and m["entries_per_alive_node_round"] == 2.7
    assert m["lost_share"] == 3 / 11 and m["overflow_share"] == 3 / 8
    assert m["hubs"] == [(3, 4, 1), (5, 3, 2)]
    # recv over the nodes that took anything or are alive: 0, 0, 1, 4, 0, 3
    assert m["recv_max_over_mean"] == 4 / (8 / 6)
    v = np.array([0, 0, 0, 1, 3, 4.0])
    gini = 2 * (np.arange(1, 7) * v).sum() / (6 * v.sum()) - 7 / 6
    assert abs(m["recv_gini"] - gini) < 1e-12 and 0 < gini < 1


@pytest.mark.parametrize("kind,name", sorted(to.WORKLOADS))
def test_oracle_runs_satisfy_the_identities(kind, name):
    """Per tick, against the oracle's digest: sends, merged messages, merged entries, the inbox
    overflow, and conservation from one tick to the next."""
    w = to.WORKLOADS[kind, name]
    ref = to.reference(kind, name)
    bt, dig = ref["ledger"].by_tick, ref["digest"]
    for t in range(1, w["ticks"] + 1):
        d = dig[t]
        assert bt[t][0] == d["sent"] - d["dropped"], (t, "sent")
        assert bt[t][2] == d["delivered"], (t, "merged")
        assert bt[t][4] == d["merges"], (t, "entries")
        if kind == "pview":
            assert bt[t][1] - bt[t][2] == d["overflow"], (t, "overflow")
        else:
            assert bt[t][1] == bt[t][2], (t, "the full view merges everything")
        if t < w["ticks"]:
            assert bt[t][0] == bt[t + 1][1] + bt[t + 1][3], (t, "conservation")
    snap = ref["ledger"].snapshot()
    assert snap["info"]["sent"] == bt[:, 0].sum() and snap["info"]["lost"] > 0


def _parse_msgcount(text):
    """(sent, recv) [nodes][ticks] of a msgcount.log, either row layout."""
    sent, recv = [], []
    blocks = re.split(rb"\nnode +\d+ sent_total +\d+  recv_total +\d+\n\n", text)
    assert blocks[-1] == b""
    for i, blk in enumerate(blocks[:-1]):
        head = b"node %3d " % (i + 1)
        assert blk.startswith(head), (i, blk[:20])
        body = blk[len(head):]
        if i + 1 == 67:
            rows = re.findall(rb"special +(\d+) +(-?\d+) +(-?\d+)\n", body)
            assert [int(r[0]) for r in rows] == list(range(len(rows)))
            pairs = [(r[1], r[2]) for r in rows]
        else:
            pairs = re.findall(rb" \( *(-?\d+), *(-?\d+)\)", body)
        sent.append([int(a) for a, _ in pairs])
        recv.append([int(b) for _, b in pairs])
    return np.array(sent, np.int32), np.array(recv, np.int32)


GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "**", "msgcount.log.gz"), recursive=True))


def test_writer_reproduces_every_golden_msgcount(tmp_path):
    """Parse the reference's own files into count arrays and write them back: identical bytes."""
    assert len(GOLDEN) >= 80
    nodes = set()
    out = str(tmp_path / "msgcount.log")
    for path in GOLDEN:
        with gzip.open(path, "rb") as f:
            want = f.read()
        sent, recv = _parse_msgcount(want)
        assert sent.ndim == 2 and sent.shape == recv.shape and sent.shape[1] > 0, path
        nodes.add(sent.shape[0])
        traffic.write_msgcount(out, sent, recv)
        with open(out, "rb") as f:
            assert f.read() == want, path
    assert 1 in nodes and 1000 in nodes and sum(1 for x in nodes if x >= 70) >= 4, sorted(nodes)


def test_writer_of_no_rows(tmp_path):
    out = str(tmp_path / "empty.log")
    traffic.write_msgcount(out, np.zeros((0, 5), np.int32), np.zeros((0, 5), np.int32))
    assert open(out, "rb").read() == b""
    traffic.write_msgcount(out, np.zeros((2, 0), np.int32), np.zeros((2, 0), np.int32))
    assert open(out, "rb").read() == (b"node   1 \nnode   1 sent_total      0  recv_total      0\n\n"
                                      b"node   2 \nnode   2 sent_total      0  recv_total      0\n\n")
