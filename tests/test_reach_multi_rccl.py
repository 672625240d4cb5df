"""Multi-source reach of engines with a communicator: per level each rank ORs its shards' share
into its next frontier, the frontiers are all-gathered over RCCL on the engine's stream and ORed
down by one small kernel, so every rank's result equals the stack of numpy BFS over the oracle's
rows.

Each case launches tests/reach_multi_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_reach_rccl.py does.  With one rank
everywhere (the communicator path with a world of one); with two ranks where two GPUs are visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_reach_multi_one_rank(case):
    for r in ranks_common.launch("reach_multi_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_reach_multi_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("reach_multi_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
