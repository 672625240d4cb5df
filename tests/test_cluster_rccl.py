"""Overlay clustering of engines with a communicator: each rank ORs its shards' share of the
observers' rows into its member words, the words are all-reduced over RCCL on the engine's stream
(SUM, exact: no two ranks write the same bit), each rank adds its share of the links and the
counters are all-reduced, so every rank's result equals the numpy counts over the oracle's rows.

Each case launches tests/cluster_ranks.py under torch.distributed.run, one fresh child process per
GPU (this process makes no GPU call for it), as tests/test_reach_multi_rccl.py does.  With one rank
everywhere (the communicator path with a world of one); with two ranks where two GPUs are visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_cluster_one_rank(case):
    for r in ranks_common.launch("cluster_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_cluster_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("cluster_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
