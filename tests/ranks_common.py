"""The harness the rank tests share: tests/test_*rccl*.py (parent side) launch a tests/*_ranks.py
program (child side) under torch.distributed.run, one fresh child process per GPU.

Parent side: the pytest process makes no GPU call for a case -- the device count comes from torch,
which does not initialise the GPU to count.  Child side: torch.distributed (gloo) carries only the
RCCL id and the verdicts; rank 0 prints one JSON line, and exit status 0 means parity.
"""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpus():
    import torch
    return torch.cuda.device_count()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(script, case, world):
    """Run tests/<script> <case> on `world` ranks; the per-rank verdicts of its JSON line."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "tests", script), case]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, "rc %d\n%s\n%s" % (p.returncode, p.stdout[-3000:],
                                                          p.stderr[-3000:])
    res = json.loads(lines[-1])
    assert res["world"] == world and len(res["ranks"]) == world
    return res["ranks"]


def start():
    """A rank program's prologue: (dist, rank, world, device, the job's RCCL id)."""
    import torch.distributed as dist
    from gossip_protocol_amd.dist import broadcast_bytes
    from gossip_protocol_amd.scale import nccl_unique_id
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    device = int(os.environ.get("LOCAL_RANK", "0"))
    return dist, rank, world, device, broadcast_bytes(nccl_unique_id() if rank == 0 else None)


def finish(dist, case, rank, world, bad, **extra):
    """A rank program's epilogue: gather every rank's verdict (`bad`, and `extra` fields), print
    rank 0's JSON line; the exit status."""
    res = [None] * world
    dist.all_gather_object(res, dict(rank=rank, bad=[str(b)[:300] for b in bad], **extra))
    if rank == 0:
        print(json.dumps({"case": case, "world": world, "ranks": res}), flush=True)
    dist.destroy_process_group()
    return 0 if not any(r["bad"] for r in res) else 1
