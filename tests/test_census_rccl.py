"""The census of engines with a communicator: each rank accumulates its shards' share and the
arrays are all-reduced over RCCL on the engine's stream (SUM for listed / fresh, MAX for max_hb),
so every rank's census equals the oracle's.

Each case launches tests/census_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_rccl_multi_gpu.py does.  With
one rank everywhere (the communicator path with a world of one); with two ranks where two GPUs
are visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_census_one_rank(case):
    for r in ranks_common.launch("census_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_census_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("census_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
