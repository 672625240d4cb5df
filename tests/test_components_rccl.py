"""Overlay components of engines with a communicator: each rank sweeps its shards, the label
arrays are all-reduced over RCCL on the engine's stream after every sweep (MIN for the weak
labels, MAX for the colours and the trim flags: every word only moves one way, so the reduced
word is what one rank sweeping all shards would hold) and the n-length kernels run on the reduced
arrays, so every rank's labels of both kinds equal tests/components_oracle.py's.

Each case launches tests/components_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_cluster_rccl.py does.  With one
rank everywhere (the communicator path with a world of one); with two ranks where two GPUs are
visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_components_one_rank(case):
    for r in ranks_common.launch("components_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_components_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("components_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
