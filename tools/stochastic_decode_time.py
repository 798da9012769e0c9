#!/usr/bin/env python3
"""Time of the stochastic decode paths at BASELINE configs[1]'s shape (x-param, batch 32, 256 x 256, synthetic weights), in ms per
DDIM iteration over 50-step decodes:

  (a) cdc_decode                      eta = 0, the loop bench.py times
  (b) cdc_decode_seeded               eta = 0.5, noise from the generator inside the sampler kernel (csrc/rng.h)
  (c) host-driven loop, torch GPU     eta = 0.5 without a seed: cdc_ddim_step per step, torch.randn_like per step
  (d) host-driven loop, NumPy         the same with host arrays: np.random draw, image and noise over PCIe per step

(c) and (d) are the code `eta != 0` ran before the seeded loop existed and still runs without a seed.  One process; the variants
alternate inside every round, each decode ends in a device synchronise; the median over the rounds and the spread (min .. max)
are printed, and written to --out.  Run it under a `timeout` (about 3 minutes at the defaults):

    timeout -k 10 600 python tools/stochastic_decode_time.py --out profiles/stochastic_decode.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sample-steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the NumPy variant (d), the slow one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    B, S, steps = a.batch, a.size, a.sample_steps
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    gen = torch.Generator(device=dev).manual_seed(77)
    init = torch.randn((B, 3, S, S), generator=gen, device=dev) * 0.8
    ctx = [torch.randn((B, c, S >> l, S >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
    init_h, ctx_h = init.cpu().numpy(), [c.cpu().numpy() for c in ctx]
    shape = (B, 3, S, S)
    torch.manual_seed(1)
    np.random.seed(1)
    variants = {
        "a": ("cdc_decode, eta = 0", lambda n: diff.decompress(ctx, shape, sample_steps=n, init=init)),
        "b": ("cdc_decode_seeded, eta = 0.5", lambda n: diff.decompress(ctx, shape, sample_steps=n, init=init, eta=0.5, seed=1234)),
        "c": ("host-driven eta = 0.5, torch GPU tensors", lambda n: diff.decompress(ctx, shape, sample_steps=n, init=init, eta=0.5)),
        "d": ("host-driven eta = 0.5, NumPy arrays", lambda n: diff.decompress(ctx_h, shape, sample_steps=n, init=init_h, eta=0.5)),
    }
    for k in "abcd":                        # every shape and kernel of the timed windows once, untimed
        variants[k][1](2)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(a.rounds):
        for k in "abcd":
            if k == "d" and r >= a.host_rounds:
                continue
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = variants[k][1](steps)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) / steps * 1e3)
            assert bool(np.isfinite(out).all() if isinstance(out, np.ndarray) else torch.isfinite(out).all().item())
    st = un.status()
    lines = [f"stochastic decode, ms per DDIM iteration ({steps}-step decodes, batch {B}, {S} x {S}, x-param, synthetic weights)",
             f"device: {torch.cuda.get_device_name(0)}; {cdc._lib.lib().cdc_version().decode()}; kernels {cdc._lib.kernel_source_hash()}",
             f"handle after the runs: {st}"]
    for k in "abcd":
        v = ms[k]
        lines.append(f"({k}) {variants[k][0]:<42s} median {statistics.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}   n = {len(v)}")
    ma, mb = statistics.median(ms["a"]), statistics.median(ms["b"])
    lines.append(f"(b) / (a) = {mb / ma:.4f};  (c) / (b) = {statistics.median(ms['c']) / mb:.3f};  (d) / (b) = {statistics.median(ms['d']) / mb:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
