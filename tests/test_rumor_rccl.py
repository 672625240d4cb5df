"""Rumor trace of engines with a communicator: column shards compute the whole map on every rank,
row shards all-reduce know each tick (MAX) and heard / known at a get (MIN / SUM) over RCCL on the
engine's stream, so every rank's result equals the numpy rule over the oracle's messages.

Each case launches tests/rumor_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_reach_rccl.py does.  With one
rank everywhere (the communicator path with a world of one); with two ranks where two GPUs are
visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_rumor_one_rank(case):
    for r in ranks_common.launch("rumor_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_rumor_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("rumor_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
