"""Workloads at the exact engine's size and parameter edges, and their CPU-oracle record.

The exact engine (gsp_create / gsp_tick_process) picks a block of 64, 128, 256, 512 or 1024
lanes by N, sorts each list in that block, sends from one block of 1024 lanes, and reads
tremove, id_filter_limit, en_buff_size, max_msg_size, step_rate and msg_drop_prob from
gsp_params.  Each workload below puts one of those on an end of its range, or N on a block
boundary; tests/test_exact_edges_cpu.py proves from the record that the workload reaches the
edge it is named for, tests/test_exact_edges_gpu.py compares the engine with the record byte for
byte.

The reference is the parametric restatement (oracle/mp1_oracle.c): at the reference's own
parameter values it is pinned to the reference itself over the full 700 ticks at every size used
here up to 1000 (tests/test_oracle_golden.py, tests/golden/ref_edge), and each parameter changes
one cited line of it.  The reference's arrays stop at MAX_NODES = 1000 (EmulNet.h:10), so for
N = 1024 the restatement is the only reference.  Nothing in a record comes from the engine.

reference(name) runs the restatement once per process and keeps the output files on disk (a
state dump with full lists is tens of MB) together with its merge count, its buffer-full
rejections and the seconds it took.
"""
import atexit
import functools
import os
import re
import shutil
import tempfile
import time

from tests.oracle_binding import EDGE_CONFS, FILES, conf_path, load_oracle, run_oracle_mp1

# name: conf = (MAX_NNB, SINGLE_FAILURE, DROP_MSG, MSG_DROP_PROB) or the name of a ref_edge
# testcase, params = gsp_params / gsp_oracle_mp1_params overrides, ticks, rng mode, seed.
WORKLOADS = {
    # no payload filter: every list grows to N - 1 entries -- the sort and rank write, the removal
    # order and the send list at N equal to the block (64) and at block / 2 + 1 (65 of 128)
    "nofilter_n64": dict(conf=(64, 0, 1, "0.1"), params=dict(id_filter_limit=65), ticks=160,
                         mode="glibc", seed=3),
    "nofilter_n65": dict(conf=(65, 0, 1, "0.1"), params=dict(id_filter_limit=66), ticks=160,
                         mode="philox", seed=3),
    # the 256-lane block with full lists; once the t = 100 victims' messages linger the
    # 30,000-message buffer fills every tick until the victims are removed, so buff_room is smaller
    # than the batch's sends and admission follows call order
    "nofilter_n129_buf": dict(conf=(129, 0, 1, "0.1"), params=dict(id_filter_limit=130), ticks=160,
                              mode="glibc", seed=3),
    "nofilter_intro16_n64": dict(conf=(64, 0, 1, "0.1"), params=dict(id_filter_limit=65),
                                 intro_list=16, ticks=160, mode="philox", seed=3),
    # tremove at its small end: entries are removed and re-added every few ticks
    "tr1_n10": dict(conf=(10, 1, 1, "0.1"), params=dict(tremove=1), ticks=150, mode="glibc", seed=3),
    "tr2_n10": dict(conf=(10, 0, 1, "0.1"), params=dict(tremove=2), ticks=150, mode="philox", seed=3),
    "tr3_nofilter_n65": dict(conf=(65, 0, 1, "0.1"), params=dict(tremove=3, id_filter_limit=66),
                             ticks=150, mode="glibc", seed=7),
    # a buffer smaller than one node's gossip list
    "buf1_n10": dict(conf=(10, 1, 0, "0.1"), params=dict(en_buff_size=1), ticks=150,
                     mode="philox", seed=3),
    "buf7_n10": dict(conf=(10, 0, 1, "0.1"), params=dict(en_buff_size=7), ticks=150,
                     mode="glibc", seed=3),
    "buf50_n40": dict(conf=(40, 1, 1, "0.1"), params=dict(en_buff_size=50), ticks=150,
                      mode="philox", seed=3),
    # every send is 40 + 16 bytes: max_msg_size 56 rejects all of them, 57 none (EmulNet.cpp:92)
    "msg56_n10": dict(conf=(10, 1, 0, "0.1"), params=dict(max_msg_size=56), ticks=60,
                      mode="glibc", seed=3),
    "msg57_n10": dict(conf=(10, 1, 0, "0.1"), params=dict(max_msg_size=57), ticks=60,
                      mode="glibc", seed=3),
    # step_rate 0: all nodes start at t = 0 and the introducer answers N - 1 JOINREQs in one
    # batch position at t = 1; at N = 1024 the send kernel's batch is its whole block
    "step0_n257": dict(conf=(257, 1, 0, "0.1"), params=dict(step_rate=0.0), ticks=140,
                       mode="philox", seed=3),
    "step0_n1024": dict(conf=(1024, 0, 1, "0.1"), params=dict(step_rate=0.0), ticks=40,
                        mode="glibc", seed=3),
    # one join per tick (node i starts at t = i, the last at t = 39)
    "step1_n40": dict(conf=(40, 0, 1, "0.1"), params=dict(step_rate=1.0), ticks=200,
                      mode="philox", seed=3),
    # one join every third tick: node i starts at t = 3 i, so joins still arrive after the
    # failure at t = 100 (the last at t = 117), which step_rate 1.0 cannot give 40 nodes
    "step3_n40": dict(conf=(40, 0, 1, "0.1"), params=dict(step_rate=3.0), ticks=200,
                      mode="glibc", seed=3),
    # the engine's largest N with every parameter at the reference's value: the last join at
    # t = 255, the failure at 100, removals from 120
    "n1024_default": dict(conf=(1024, 0, 1, "0.1"), params={}, ticks=300, mode="philox", seed=3),
    # the sizes of tests/golden/ref_edge, where the restatement is pinned to the reference over
    # 700 ticks; here the engine against the restatement over the first 300
    "n64_multi": dict(conf="n64_multi", params={}, ticks=300, mode="glibc", seed=3),
    "n128_multi": dict(conf="n128_multi", params={}, ticks=300, mode="philox", seed=3),
    "n129_single": dict(conf="n129_single", params={}, ticks=300, mode="glibc", seed=3),
    "n256_multi": dict(conf="n256_multi", params={}, ticks=300, mode="philox", seed=3),
    "n257_single": dict(conf="n257_single", params={}, ticks=300, mode="glibc", seed=3),
    "n513_multi": dict(conf="n513_multi", params={}, ticks=300, mode="philox", seed=3),
    "n1000_multidrop": dict(conf="n1000_multidrop", params={}, ticks=300, mode="glibc", seed=3),
}

# ref_edge runs cheap enough for the engine to repeat over all 700 ticks against the fixture
SMALL_EDGE_CONFS = ["n1_single", "n2_multi", "n10_drop0", "n10_drop029", "n10_drop100"]

# the box gsp_create admits (include/gossip/gossip.h): every workload lies inside it
BOX = dict(tremove=(1, 2**31 - 1), id_filter_limit=(0, 2**31 - 1), en_buff_size=(0, 2**20 - 1),
           max_msg_size=(0, 2**31 - 1), step_rate=(0.0, float("inf")), msg_drop_prob=(0.0, 1.0))

_tmp = tempfile.mkdtemp(prefix="exact_edges_")
atexit.register(shutil.rmtree, _tmp, ignore_errors=True)


def write_conf(name, fields):
    """A .conf of our own in the scratch directory; returns its path."""
    path = os.path.join(_tmp, name + ".conf")
    with open(path, "w") as f:
        f.write("MAX_NNB: %d\nSINGLE_FAILURE: %d\nDROP_MSG: %d\nMSG_DROP_PROB: %s\n" % fields)
    return path


def conf_file(name):
    """Path of the workload's .conf: a committed ref_edge testcase, or one written here."""
    c = WORKLOADS[name]["conf"]
    if isinstance(c, str):
        assert c in EDGE_CONFS
        return conf_path(c)
    return write_conf(name, c)


def nodes(name):
    c = WORKLOADS[name]["conf"]
    if isinstance(c, str):
        return int(re.match(r"n(\d+)_", c).group(1))
    return c[0]


def run_restatement(conf_file_path, seed, mode, out_dir, ticks, intro_list=0, **params):
    """run_oracle_mp1 on a .conf anywhere: it resolves names under tests/golden, and an absolute
    path without its extension resolves to itself.  Returns (paths, merges, buffer-full
    rejections, seconds)."""
    assert os.path.isabs(conf_file_path) and conf_file_path.endswith(".conf")
    t0 = time.perf_counter()
    paths = run_oracle_mp1(conf_file_path[:-len(".conf")], seed, mode, out_dir, ticks=ticks,
                           intro_list=intro_list, **params)
    seconds = time.perf_counter() - t0
    L = load_oracle()
    return paths, L.gsp_oracle_mp1_merges(), L.gsp_oracle_mp1_buffer_full_rejects(), seconds


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's record of workload `name` (one run per process)."""
    w = WORKLOADS[name]
    paths, merges, rejects, seconds = run_restatement(
        conf_file(name), w["seed"], w["mode"], os.path.join(_tmp, name), w["ticks"],
        intro_list=w.get("intro_list", 0), **w["params"])
    return {"name": name, "w": w, "n": nodes(name), "paths": paths, "merges": merges,
            "buffer_full_rejects": rejects, "seconds": seconds}


def read(ref, name):
    with open(ref["paths"][name], "rb") as f:
        return f.read()


# ---- readers of the reference's file formats ----
def list_lengths(state_bytes):
    """{(tick, node id): list length} of a state dump ("t id inited in_group failed hb nlist ...")."""
    out = {}
    for line in state_bytes.splitlines():
        f = line.split(b" ", 7)
        out[(int(f[0]), int(f[1]))] = int(f[6])
    return out


_LINE_TICK = re.compile(rb"\[(\d+)\] (.*)$")


def log_lines(dbg_bytes, word):
    """Ticks of the dbg.log lines whose text contains `word` (bytes)."""
    return [int(m.group(1)) for m in map(_LINE_TICK.search, dbg_bytes.split(b"\n"))
            if m and word in m.group(2)]


def sent_per_tick(msgcount_bytes, node_id):
    """msgcount.log's per-tick sent counts of one node (EmulNet.cpp:184-220; not node 67, whose
    layout differs)."""
    assert node_id != 67
    text = msgcount_bytes.decode()
    start = text.index("node %3d " % node_id)
    end = text.index("node %3d sent_total" % node_id)
    return [int(a) for a, _ in re.findall(r"\(\s*(\d+),\s*(\d+)\)", text[start:end])]


__all__ = ["WORKLOADS", "SMALL_EDGE_CONFS", "BOX", "FILES", "reference", "read", "conf_file",
           "nodes", "run_restatement", "write_conf", "list_lengths", "log_lines", "sent_per_tick"]
