"""EXACT mode at its size and parameter edges: the engine against the restatement, byte for byte.

Every workload of tests/exact_edges.py runs through exact.run_application (the HIP kernels do
every merge / sort / removal / send list / draw / admission) with the same gsp_params overrides
and tick count as the restatement's record, and dbg.log, msgcount.log, the end-of-tick state of
every node and the driver's stdout lines must be the same bytes; so must the merge counts.
tests/test_exact_edges_cpu.py proves that each record reaches the edge the workload is named for.

The restatement is pinned to the reference at every size up to 1000 (tests/golden/ref_edge).
The reference's own arrays stop at MAX_NODES = 1000, so for step0_n1024 and n1024_default the
restatement is the only reference.  The small ref_edge runs are cheap over all 700 ticks and are
compared with the reference's fixtures directly.
"""
import pytest

from gossip_protocol_amd import exact
from tests import exact_edges as xe
from tests.oracle_binding import (BIG_FILES, EDGE_RUNS, FILES, conf_path, golden_edge,
                                  outputs_for_big)

pytestmark = pytest.mark.gpu


def _same(name, got, want):
    if got != want:
        gl, wl = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
        pytest.fail("%s differs at line %d:\n got: %s\nwant: %s" % (
            name, first, gl[first][:300] if first < len(gl) else "<eof>",
            wl[first][:300] if first < len(wl) else "<eof>"))


@pytest.mark.parametrize("name", list(xe.WORKLOADS))
def test_exact_edge_vs_restatement(tmp_path, name):
    ref = xe.reference(name)
    w = ref["w"]
    out = exact.run_application(xe.conf_file(name), w["seed"], w["mode"], str(tmp_path),
                                ticks=w["ticks"], intro_list=w.get("intro_list", 0),
                                params=w["params"])
    for f in FILES:
        with open(out[f], "rb") as fh:
            _same(f, fh.read(), xe.read(ref, f))
    assert out["stats"].merges == ref["merges"]
    assert out["stats"].batches == w["ticks"]


@pytest.mark.parametrize("conf,seed,mode", [r for r in EDGE_RUNS if r[0] in xe.SMALL_EDGE_CONFS],
                         ids=lambda x: str(x))
def test_exact_bitexact_vs_reference_edge(tmp_path, conf, seed, mode):
    """N = 1 and 2 (the failure draws rand() % 1 and rand() % 2 / 2) and MSG_DROP_PROB 0, 0.29
    (threshold (int)(0.29 * 100) = 28) and 1 against the reference's own outputs over all 700
    ticks (tests/golden/ref_edge)."""
    got = outputs_for_big(exact.run_application(conf_path(conf), seed, mode, str(tmp_path)))
    for f in BIG_FILES:
        _same(f, got[f], golden_edge(mode, conf, seed, f))
