"""Detection ledger of engines with a communicator: every rank folds the records of its own
columns or rows and a get all-reduces the arrays (MIN / MAX / SUM) over RCCL on the engine's stream
into a staging buffer, so every rank's result equals the numpy rule over the oracle's events.

Each case launches tests/detect_ranks.py under torch.distributed.run, one fresh child process
per GPU (this process makes no GPU call for it), as tests/test_rumor_rccl.py does.  With one
rank everywhere (the communicator path with a world of one); with two ranks where two GPUs are
visible.
"""
import pytest

from tests import ranks_common

pytestmark = pytest.mark.gpu
CASES = ["columns_tiled", "rows", "pview_rows"]


@pytest.mark.parametrize("case", CASES)
def test_detect_one_rank(case):
    for r in ranks_common.launch("detect_ranks.py", case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_detect_two_ranks(case):
    if ranks_common.gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % ranks_common.gpus())
    for r in ranks_common.launch("detect_ranks.py", case, 2):
        assert r["bad"] == [], (case, r)
