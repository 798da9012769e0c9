#!/usr/bin/env python3
"""Golden vectors of the second-order multistep sampler: tests/golden/solver_small.npz.

Like make_golden.py this runs only where the real reference is (it imports the reference's own Unet through make_golden's helpers and
holds none of its text); the sampler itself has no reference counterpart, so the update is stated here, in float64:

    x0     = the prediction of the DDIM step (pred_mode "x": fx; "v": sqrt_ac x - sqrt_1mac fx; "noise": sqrt_recip x - sqrt_recipm1 fx),
             clamped to [-1, 1] in the x tree (compress()'s clip_denoised=True); the eps tree runs clip_noise="none"
    x_next = a_i x + b_i x0 + c_i x0_prev,     x0_prev <- x0 (zeros before the first step)

over the float32 tables of cdc_compression_amd.schedule (the grid, the prediction's scalars, a / b / c).  The network is the
reference's float32 U-Net, as in the decode goldens; the image is fed back to it as float32 each step, the history stays float64.
Cases small_x, small_eps, odd_x and pred_mode "v" on small_x; 5 steps; spacing "index" and "logsnr".  Stored: data only -- each
run's grid, its a / b / c tables and the final image.

    python tests/golden/make_golden_solver.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from cdc_compression_amd import synth  # noqa: E402
from cdc_compression_amd.schedule import SampleSchedule  # noqa: E402

STEPS = 5
RUNS = [("small_x", "small_x", "x"), ("small_eps", "small_eps", "noise"), ("odd_x", "odd_x", "x"), ("small_x_v", "small_x", "v")]


def decode(net, sched, ctx, init, pred_mode, clip, tables):
    a, b, c = (t.astype(np.float64) for t in tables)
    d = lambda t: t.astype(np.float64)                                 # noqa: E731
    x = init.copy()
    prev = np.zeros(x.shape, np.float64)
    tctx = [torch.from_numpy(t) for t in ctx]
    for i in reversed(range(sched.steps)):
        time = np.full((x.shape[0], 1), sched.time_in[i], np.float32)
        with torch.no_grad():
            fx = net(torch.from_numpy(x), torch.from_numpy(time), tctx).numpy().astype(np.float64)
        x64 = x.astype(np.float64)
        if pred_mode == "x":
            x0 = fx
        elif pred_mode == "v":
            x0 = d(sched.sqrt_ac)[i] * x64 - d(sched.sqrt_one_minus_ac)[i] * fx
        else:
            x0 = d(sched.sqrt_recip)[i] * x64 - d(sched.sqrt_recipm1)[i] * fx
        if clip:
            x0 = np.clip(x0, -1.0, 1.0)
        x = (a[i] * x64 + b[i] * x0 + c[i] * prev).astype(np.float32)
        prev = x0
    return x


def main():
    out = {"steps": STEPS}
    for key, name, pred_mode in RUNS:
        tree, kw, ctxc, H, W, B = mg.CONFIGS[name]
        _, net, _, _ = mg.gen_unet(name, taps=False)
        ctx = synth.context_pyramid(ctxc, B, H, W, seed=3)
        init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
        T, vs = mg.DIFF[tree]["num_timesteps"], mg.DIFF[tree]["var_schedule"]
        for spacing in ("index", "logsnr"):
            sched = SampleSchedule(T, vs, "x" if tree == "xparam" else "eps", STEPS, spacing=spacing)
            tables = sched.solver()
            rec = decode(net, sched, ctx, init, pred_mode, tree == "xparam", tables)
            k = f"{key}_{spacing}"
            out[k + "_grid"] = sched.index
            out[k + "_a"], out[k + "_b"], out[k + "_c"] = tables
            out[k + "_rec"] = rec
            print(k, list(sched.index), "max |b|, |c| =", float(np.abs(tables[1]).max()), float(np.abs(tables[2]).max()),
                  "max |rec| =", float(np.abs(rec).max()))
    np.savez_compressed(os.path.join(HERE, "solver_small.npz"), **out)


if __name__ == "__main__":
    main()
