"""The view audit of engines with a communicator: each rank accumulates its shards' share and
the arrays are all-reduced over RCCL on the engine's stream (SUM for the counts and the wrapping
64-bit print, MAX for age_max), so every rank's audit equals the oracle's.

Each case launches tests/audit_ranks.py under torch.distributed.run, one fresh child process per
GPU (this process makes no GPU call for it), as tests/test_census_rccl.py does.  With one rank
everywhere (the communicator path with a world of one); with two ranks where two GPUs are
visible.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["columns_tiled", "rows", "pview_rows"]


def _gpus():
    import torch
    return torch.cuda.device_count()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(case, world):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "tests", "audit_ranks.py"), case]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, "rc %d\n%s\n%s" % (p.returncode, p.stdout[-3000:],
                                                          p.stderr[-3000:])
    res = json.loads(lines[-1])
    assert res["world"] == world and len(res["ranks"]) == world
    return res["ranks"]


@pytest.mark.parametrize("case", CASES)
def test_audit_one_rank(case):
    for r in _launch(case, 1):
        assert r["bad"] == [], (case, r)


@pytest.mark.parametrize("case", CASES)
def test_audit_two_ranks(case):
    if _gpus() < 2:
        pytest.skip("needs two GPUs (%d visible)" % _gpus())
    for r in _launch(case, 2):
        assert r["bad"] == [], (case, r)
