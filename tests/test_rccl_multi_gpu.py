"""RCCL with more than one rank: the sharded engines' collectives --
the count all-gather and picks all-reduce MAX of column shards, the grouped ncclSend /
ncclRecv of row shards (full view and partial view), the count broadcasts and node 0's row
broadcast -- run between real ranks, and the job's results are checked against the oracle
(the behaviour is EmulNet::ENsend / ENrecv across shards, EmulNet.cpp:87-177).

Each case launches tests/rccl_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it: the device count comes from torch, which does
not initialise the GPU to count).  Skips where fewer than two GPUs are visible -- the
one-GPU boxes this build is developed on; the driver's 8-GPU node runs it.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["columns_tiled", "rows", "pview_rows", "pview_capacity",
                                  "rows_capacity", "pview_burst", "rows_burst"])
def test_two_ranks_match_the_oracle(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("rccl_ranks.py", case, 2):
        assert r["bad"] == [] and ("capacity" in case or r["xgmi"] > 0), r


def test_rank_program_one_rank():
    """The same child program with one rank (the one-GPU boxes): every check but the xGMI
    bytes, so the multi-GPU test's own logic is exercised wherever a GPU exists."""
    for case in ("columns_tiled", "rows", "pview_rows", "pview_capacity", "rows_capacity",
                 "pview_burst", "rows_burst"):
        for r in ranks_common.launch("rccl_ranks.py", case, 1):
            assert r["bad"] == [], (case, r)
