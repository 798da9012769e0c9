#!/usr/bin/env python3
"""Parallel-in-time decode against the sequential decode: sweeps, wall time and the deviation of the picture, over a grid
of windows and tolerances (profiles/parallel_decode.md).  BASELINE's x-param network with SYNTHETIC weights, 256 x 256, B = 1, device
tensors.  Sweep counts depend on the network: these figures say what the machinery costs, not what a trained model converges like.

Two modes, so that the sequential baseline can come from another checkout of the project (the commit before the feature):

    python tools/parallel_time.py seq --tree <checkout> --out DIR       # sequential decodes: DIR/seq_<steps>.npy, DIR/seq.json
    python tools/parallel_time.py par --ref DIR --out DIR               # the grid, against DIR's pictures and times; DIR/par.json
    python tools/parallel_time.py ops --tree <checkout> --out FILE      # the op labels of a plain decode (cdc_prof_op), one per line
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["seq", "par", "ops"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", required=True)
ap.add_argument("--ref", default=None)
ap.add_argument("--steps", type=int, nargs="+", default=[500, 65])
ap.add_argument("--windows", type=int, nargs="+", default=[8, 16, 32])
ap.add_argument("--tols", type=float, nargs="+", default=[1e-4, 1e-3, 1e-2])
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
A = ap.parse_args()
sys.path.insert(0, os.path.abspath(A.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import _lib, synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))
S, DEV = A.size, torch.device("cuda", 0)


def model():
    un = cdc.Unet(**KW, device=0)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    g = torch.Generator(device=DEV).manual_seed(1256)
    init = torch.randn((1, 3, S, S), generator=g, device=DEV) * 0.8
    ctx = [torch.randn((1, c, S >> l, S >> l), generator=g, device=DEV) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
    return un, diff, init, ctx


def timed(fn, rounds):
    ts, res = [], None
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), sorted(ts)[len(ts) // 2], res


def op_table(un):
    L, h = _lib.lib(), un._handle()
    out = []
    for i in range(L.cdc_prof_num_ops(h)):
        lab, ms, n, fl = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(h, L.cdc_prof_op(h, i, ctypes.byref(lab), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        out.append((lab.value.decode(), ms.value, n.value))
    return out


def main():
    un, diff, init, ctx = model()
    shape = (1, 3, S, S)
    if A.mode == "ops":
        _lib.check(un._handle(), _lib.lib().cdc_prof_enable(un._handle(), 1))
        diff.decompress(ctx, shape, sample_steps=3, init=init)
        with open(A.out, "w") as f:
            f.write("".join(f"{lab}  n={n}\n" for lab, _, n in op_table(un)))
        return
    os.makedirs(A.out, exist_ok=True)
    diff.decompress(ctx, shape, sample_steps=2, init=init)                 # code objects, the program
    if A.mode == "seq":
        res = {}
        for steps in A.steps:
            lo, med, rec = timed(lambda: diff.decompress(ctx, shape, sample_steps=steps, init=init), A.rounds)
            np.save(os.path.join(A.out, f"seq_{steps}.npy"), rec.cpu().numpy())
            res[str(steps)] = dict(ms_min=lo, ms_median=med, ms_per_step=lo / steps)
            print(f"sequential {steps} steps: {lo:.1f} ms (median {med:.1f}), {lo / steps:.3f} ms / step", flush=True)
        json.dump(res, open(os.path.join(A.out, "seq.json"), "w"), indent=1)
        return
    seq = json.load(open(os.path.join(A.ref, "seq.json")))
    rows = []
    for steps in A.steps:
        ref = np.load(os.path.join(A.ref, f"seq_{steps}.npy")).astype(np.float64)
        here, _, rec = timed(lambda: diff.decompress(ctx, shape, sample_steps=steps, init=init), 1)
        same = bool(np.array_equal(rec.cpu().numpy(), ref.astype(np.float32)))
        print(f"{steps} steps: this checkout's sequential decode {here:.1f} ms, bit-equal to the reference picture: {same}", flush=True)
        for p in A.windows:
            # what a sweep of p rows costs in sequential steps: a p-row sequential decode of a few steps, per step
            few = 4
            c = [t.repeat(p, 1, 1, 1) for t in ctx]
            diff.decompress(c, (p, 3, S, S), sample_steps=2, init=init.repeat(p, 1, 1, 1))
            rows_ms, _, _ = timed(lambda: diff.decompress(c, (p, 3, S, S), sample_steps=few, init=init.repeat(p, 1, 1, 1)), A.rounds)
            sweep_cost = rows_ms / few / seq[str(steps)]["ms_per_step"]
            for tol in A.tols:
                diff.decompress(ctx, shape, sample_steps=2, init=init, parallel=2, parallel_tol=tol)
                lo, med, (rec, info) = timed(lambda: diff.decompress(ctx, shape, sample_steps=steps, init=init, parallel=p, parallel_tol=tol,
                                                                      return_info=True), A.rounds if steps < 200 else 1)
                got = rec.cpu().numpy().astype(np.float64)
                relerr = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
                mse = float((((np.clip(got, -1, 1) - np.clip(ref, -1, 1)) / 2) ** 2).mean())
                psnr = float("inf") if mse == 0 else 10 * math.log10(1.0 / mse)
                row = dict(steps=steps, window=p, tol=tol, sweeps=info["sweeps"], mean_stride=steps / info["sweeps"], max_stride=info["max_stride"],
                           sweep_cost_in_steps=sweep_cost, ms=lo, seq_ms=seq[str(steps)]["ms_min"], speedup=seq[str(steps)]["ms_min"] / lo,
                           relerr=relerr, psnr=psnr, max_residual=info["max_residual"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    # the update kernel (with its residual kernel, one op) against its bytes at the copy rate of this process
    L, h = _lib.lib(), un._handle()
    per = 3 * S * S
    kern = []
    for p in A.windows:
        _lib.check(h, L.cdc_prof_reset(h))
        _lib.check(h, L.cdc_prof_enable(h, 1))
        diff.decompress(ctx, shape, sample_steps=max(A.steps), init=init, parallel=p, parallel_tol=0.0)
        _lib.check(h, L.cdc_prof_enable(h, 0))
        upd = [(ms / n, n) for lab, ms, n in op_table(un) if lab.startswith("window update") and n]
        nbytes = 12 * p * per + 12 * per                    # per live row: model output and old guess read, new guess written; y_w, `last`
        rate = ctypes.c_double()
        assert L.cdc_probe_hbm_copy(0, max(nbytes, 1 << 20), 20, ctypes.byref(rate)) == 0
        big = ctypes.c_double()
        assert L.cdc_probe_hbm_copy(0, 1 << 30, 5, ctypes.byref(big)) == 0
        k = dict(window=p, update_us=upd[0][0] * 1e3 if upd else None, launches=upd[0][1] if upd else 0, bytes=nbytes,
                 copy_gbs_same_bytes=rate.value, copy_us_same_bytes=nbytes / rate.value * 1e-3, copy_gbs_1gib=big.value)
        kern.append(k)
        print(json.dumps(k), flush=True)
    json.dump(dict(rows=rows, kernel=kern), open(os.path.join(A.out, "par.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
