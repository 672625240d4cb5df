"""Traffic ledger of engines with a communicator: column ranks count the whole job from the one
receiver CSR, row ranks count their own rows and a get all-reduces the buffers (SUM; MAX for the
peaks) over RCCL on the engine's stream into staging, so every rank's result equals the numpy rule
over the oracle.

Each case launches tests/traffic_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_detect_rccl.py does.  With one
rank everywhere (the communicator path with a world of one); with two ranks where two GPUs are
visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows", "pview_tfail"]


@pytest.mark.parametrize("case", CASES)
def test_traffic_one_rank(case):
    for r in ranks_common.launch("traffic_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_traffic_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("traffic_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
