#!/usr/bin/env python3
"""What K samples per image cost, on the full x-param U-Net at 256 x 256, 20 steps, gamma = 0.8, eta = 0.5,
synthetic weights, device tensors:

  - ms per sample-iteration (wall time of the decodes / (B K steps)) of `decompress(samples=8)` in ONE library call against eight
    calls of one sample per image (`sample_chunk=1`), for B = 1 and B = 4;
  - GB/s of the three kernels of csrc/sample_kernels.hip at 32 x 3 x 256^2 with K = 8, counting the bytes each has to move
    (repeat: B images read, B K written; moments: B K read, mean and m2 written; select: B images read, B written).

--parent-tree DIR: a built checkout of the parent commit.  Three alternating plain `bench.py --gpus 1` runs of that tree and of this
one are recorded below the table; this tree's mean must lie inside the parent's own min .. max spread widened by 0.2 % (no default
path executes new code: a check that nothing moved, not a speed claim).

    timeout -k 10 900 python tools/samples_time.py --out profiles/samples_time.txt [--parent-tree DIR]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import _lib, synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))


def decode_table(diff, dev, S, steps, K, rounds):
    lines = []
    gen = torch.Generator(device=dev).manual_seed(77)
    for B in (1, 4):
        ctx = [torch.randn((B, c, S >> l, S >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
        args = dict(samples=K, seed=1000, gamma=0.8, eta=0.5, sample_steps=steps)
        row = {}
        for chunk in (K, 1):
            diff.decompress(ctx, sample_chunk=chunk, **dict(args, sample_steps=2))          # launch programs, code pages
            torch.cuda.synchronize()
            ts = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                out = diff.decompress(ctx, sample_chunk=chunk, **args)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / (B * K * steps))
            assert tuple(out.shape) == (B, K, 3, S, S) and bool(torch.isfinite(out).all().item())
            row[chunk] = ts
        med = statistics.median
        lines.append(f"B = {B}, K = {K}: one call of {B * K:2d} rows  median {med(row[K]):7.4f}  min {min(row[K]):7.4f}  max {max(row[K]):7.4f}   |   "
                     f"{K} calls of {B} row(s)  median {med(row[1]):7.4f}  min {min(row[1]):7.4f}  max {max(row[1]):7.4f}   "
                     f"ms per sample-iteration   ratio {med(row[1]) / med(row[K]):5.2f} x   n = {rounds}")
    return lines


def kernel_table(un, dev, B, S, K, reps):
    L, h = _lib.lib(), un._handle()
    per = 3 * S * S
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.randn((B, per), device=dev)
    smp = torch.empty((B * K, per), device=dev)
    mean, m2, best = (torch.empty((B, per), device=dev) for _ in range(3))
    pick = (ctypes.c_int * B)(*[b % K for b in range(B)])
    D = _lib.CDC_MEM_DEVICE
    calls = {
        "repeat_images (float32)": (lambda: L.cdc_repeat_images(h, src.data_ptr(), smp.data_ptr(), B, K, per, 4, D, st), 4 * per * B * (1 + K)),
        "sample_moments (mean, m2)": (lambda: L.cdc_sample_moments(h, smp.data_ptr(), B, K, per, 0, mean.data_ptr(), m2.data_ptr(), 1, D, st), 4 * per * B * (K + 2)),
        "sample_moments (mean only)": (lambda: L.cdc_sample_moments(h, smp.data_ptr(), B, K, per, 0, mean.data_ptr(), None, 0, D, st), 4 * per * B * (K + 1)),
        "sample_select": (lambda: L.cdc_sample_select(h, smp.data_ptr(), pick, best.data_ptr(), B, K, per, D, st), 4 * per * B * 2),
    }
    lines = []
    for name, (call, nbytes) in calls.items():
        _lib.check(h, call())
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(h, call())
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        lines.append(f"{name:<27s} {nbytes / 1e6:8.1f} MB   best {min(ms) * 1e3:7.1f} us  median {statistics.median(ms) * 1e3:7.1f} us   "
                     f"{nbytes / (min(ms) * 1e-3) / 1e9:7.1f} GB/s (best)   n = {reps}")
    assert torch.equal(best[1], smp[K + 1]) and bool(torch.isfinite(mean).all().item())
    return lines


def bench_ab(parent, runs, steps, warmup):
    """Alternating plain bench.py runs, parent tree first -> (lines, ok)."""
    vals = {"parent": [], "head": []}
    for _ in range(runs):
        for tag, tree in (("parent", parent), ("head", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=tree, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"bench.py of the {tag} tree failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            res = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1]
            vals[tag].append(float(res["value"]))
    lo, hi = min(vals["parent"]) * (1 - 0.002), max(vals["parent"]) * (1 + 0.002)
    mean = statistics.mean(vals["head"])
    ok = lo <= mean <= hi
    fmt = lambda v: " ".join(f"{x:.4f}" for x in v)      # noqa: E731
    return [f"plain bench.py --gpus 1 --steps {steps} --warmup {warmup}, images/s, {runs} alternating runs (parent, head, parent, ...):",
            f"parent  {fmt(vals['parent'])}   min {min(vals['parent']):.4f}  max {max(vals['parent']):.4f}",
            f"head    {fmt(vals['head'])}   mean {mean:.4f}",
            f"head's mean inside the parent's spread widened by 0.2 % [{lo:.4f}, {hi:.4f}]: {'yes' if ok else 'NO'}"], ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sample-steps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    S, K = a.size, a.samples
    lines = [f"K samples per image: decompress(samples={K}) on the full x-param U-Net, {S} x {S}, {a.sample_steps} steps, gamma 0.8, eta 0.5, "
             "synthetic weights, device tensors",
             f"device: {torch.cuda.get_device_name(0)}; {_lib.lib().cdc_version().decode()}; kernels {_lib.kernel_source_hash()}"]
    lines += decode_table(diff, dev, S, a.sample_steps, K, a.rounds)
    lines.append(f"handle after the runs: {un.status()}")
    lines.append(f"the kernels of sample_kernels.hip at {32} x 3 x {S}^2 float32, K = {K} (bytes each has to move; event time of one call):")
    lines += kernel_table(un, dev, 32, S, K, 20)
    ok = True
    if a.parent_tree:
        del diff, un
        torch.cuda.empty_cache()
        more, ok = bench_ab(os.path.abspath(a.parent_tree), 3, a.bench_steps, a.bench_warmup)
        lines += more
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        sys.exit("the head's bench mean left the parent's spread")


if __name__ == "__main__":
    main()
