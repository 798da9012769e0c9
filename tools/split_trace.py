#!/usr/bin/env python3
"""Split decode in a kernel trace: rocprofv3 --kernel-trace --output-format csv of `bench.py --sample-steps N`.
Finds the sampler kernels (one per chain and iteration), takes the last N per queue as the timed decode, and prints per iteration
the wall time between the points where every chain has finished it (device timestamps), and how much of that window has kernels of
two queues running at once.

    python tools/split_trace.py <dir or kernel_trace.csv> N
"""
import csv
import glob
import os
import sys


def main():
    path, n = sys.argv[1], int(sys.argv[2])
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "0"), r["Kernel_Name"]))
    rows.sort()
    samplers = {}
    for s, e, q, name in rows:
        if "sampler_kernel" in name or "sampler_rows4_kernel" in name:
            samplers.setdefault(q, []).append(e)
    chains = {q: v[-n:] for q, v in samplers.items() if len(v) >= n}
    done = [max(v[k] for v in chains.values()) for k in range(n)]         # every chain has finished iteration k
    print(f"{os.path.basename(path)}: {len(chains)} chain(s), {n} iterations")
    for k in range(1, n):
        t0, t1 = done[k - 1], done[k]
        active = [(max(s, t0), min(e, t1), q) for s, e, q, _ in rows if e > t0 and s < t1 and q in chains]
        ev = sorted([(s, 1, q) for s, e, q in active] + [(e, -1, q) for s, e, q in active])
        live, both, busy, last = {}, 0, 0, t0
        for t, d, q in ev:
            nq = sum(1 for c in live.values() if c > 0)
            busy += (t - last) if nq >= 1 else 0
            both += (t - last) if nq >= 2 else 0
            last = t
            live[q] = live.get(q, 0) + d
        print(f"  iteration {k}: {(t1 - t0) / 1e6:.3f} ms wall, {busy / 1e6:.3f} ms with a kernel running, {both / 1e6:.3f} ms with kernels of two queues")


if __name__ == "__main__":
    main()
