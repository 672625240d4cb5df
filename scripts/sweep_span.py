#!/usr/bin/env python3
"""Per tick of a rocprofv3 --kernel-trace CSV of bench.py: the summed scale_sweep_kernel time,
the number of sweep launches, and the span from the first sweep start to the end of the tick's
scale_long_kernel (what the launch structure of a tick costs beyond the kernels themselves).
A tick is closed by its scale_long_kernel; ticks without a sweep launch (the init tick) are
skipped.  Prints the mean over the last `window` ticks (default 20: bench.py --steps 20).
    python scripts/sweep_span.py <..._kernel_trace.csv> [window]
"""
import csv
import sys


def main():
    path = sys.argv[1]
    window = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    ticks, first, total, launches = [], None, 0, 0
    for start, end, name in rows:
        if "scale_sweep_kernel" in name:
            if first is None:
                first = start
            total += end - start
            launches += 1
        elif "scale_long_kernel" in name:
            if first is not None:
                ticks.append((total, end - first, launches, end - start))
            first, total, launches = None, 0, 0
    ticks = ticks[-window:]
    n = len(ticks)
    if not n:
        print("no sweep tick in", path)
        sys.exit(1)
    print("ticks %d  sweep launches/tick %.1f" % (n, sum(t[2] for t in ticks) / n))
    print("sweep kernels, summed   %.4f ms/tick" % (sum(t[0] for t in ticks) / n / 1e6))
    print("first sweep -> long end %.4f ms/tick" % (sum(t[1] for t in ticks) / n / 1e6))
    print("scale_long_kernel       %.4f ms/tick" % (sum(t[3] for t in ticks) / n / 1e6))


if __name__ == "__main__":
    main()
