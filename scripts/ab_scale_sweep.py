#!/usr/bin/env python3
"""The headline as bench.py measures it (a plain run, default arguments) under library /
environment variants, each run a child process of its own, interleaved; per variant and run:
ms_per_step and roofline.kernel_ms_per_tick of bench.py's line.  Stops at the first child
that fails (nothing more is started on the GPU after a fault).
    python scripts/ab_scale_sweep.py [reps] parent:GSP_LIB_VARIANT=parent sweep512:
    python scripts/ab_scale_sweep.py 3 block:GSP_TEST_SCALE_SWEEP=0 \\
        w512:GSP_TEST_SCALE_SWEEP=512 w1024t:GSP_TEST_SCALE_SWEEP=1024,GSP_TEST_SCALE_POLICY=4
GSP_TEST_SCALE_POLICY bit 0 makes the sweep's stores of the new table non-temporal.
AB_BENCH_ARGS (environment): further bench.py arguments, e.g. "--no-events".
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args.pop(0)) if args and args[0].isdigit() else 3
    extra = os.environ.get("AB_BENCH_ARGS", "").split()
    for rep in range(reps):
        for spec in args:
            name, _, envs = spec.partition(":")
            env = dict(os.environ)
            for kv in filter(None, envs.split(",")):
                k, _, v = kv.partition("=")
                env[k] = v
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env,
                               capture_output=True, text=True,
                               timeout=int(os.environ.get("AB_TIMEOUT", 240)))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                print(name, "failed (exit %d)" % r.returncode, r.stderr[-800:], flush=True)
                sys.exit(1)
            j = json.loads(lines[-1])
            print(json.dumps({"variant": name, "rep": rep, "ms_per_step": j["ms_per_step"],
                              "kernel_ms_per_tick": j["roofline"]["kernel_ms_per_tick"],
                              "frac": j["roofline"]["frac"]}), flush=True)
