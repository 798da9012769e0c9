#!/usr/bin/env python3
"""Time of cdc_distortion (device pointers) at batch 32, 256 x 256 and 500 x 333, in microseconds per call, for PSNR alone and for
MS-SSIM alone -- the call as a user makes it: launches, the copy of the results to the host and the stream synchronisation it ends
in.  The operands are the ones evaluate() compares: the float32 padded decoder frame against the uint8 image.  Beside them: the
same run's cdc_probe_hbm_copy rate, the two operands' window bytes and the time those bytes take at that rate (what bounds the PSNR
pass), the launch-only time of an empty-ish call (1 x 1 PSNR: what bounds small calls), and the share of a 500-step decode (measured
here over a short decode of the full x-param model at the same shape).  Writes --out (profiles/metrics.md).  About a minute:

    timeout -k 10 600 python tools/metrics_time.py --out profiles/metrics.md
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import metrics, synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))


def timed(fn, reps, rounds=5):
    """Median over `rounds` of the mean time of `reps` calls (each call synchronises), in microseconds."""
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t) / reps * 1e6)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--decode-steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--notes", default=None, help="a text file appended to the report (the parity figures of the GPU tests)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    B = a.batch
    L = cdc._lib.lib()
    rate = ctypes.c_double()
    assert L.cdc_probe_hbm_copy(0, 1 << 28, 5, ctypes.byref(rate)) == 0
    gbs = rate.value
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    gen = torch.Generator(device=dev).manual_seed(5)
    lines = ["# cdc_distortion: time per call", "",
             f"device: {torch.cuda.get_device_name(0)}; {L.cdc_version().decode()}; kernels {cdc._lib.kernel_source_hash()}",
             f"cdc_probe_hbm_copy of this run: {gbs:.0f} GB/s (read + written bytes)", "",
             f"Batch {B}, device pointers, float32 padded frame against the uint8 image, median (min .. max) over 5 rounds of {a.reps} calls.",
             "A call ends in the copy of its results to the host and a stream synchronisation.", "",
             "| image (frame) | operand bytes in the window | those bytes at the copy rate | PSNR alone | MS-SSIM alone | both | ms per DDIM iteration | PSNR + MS-SSIM share of a 500-step decode |",
             "|---|---|---|---|---|---|---|---|"]
    tiny = torch.zeros((1, 3, 1, 1), device=dev)
    floor = timed(lambda: metrics.psnr(un, tiny, tiny), a.reps)
    for H, W in ((256, 256), (500, 333)):
        Hp, Wp = diff.padded_size(H, W)
        img = torch.randint(0, 256, (B, 3, H, W), generator=gen, device=dev, dtype=torch.uint8)
        rec = torch.zeros((B, 3, Hp, Wp), device=dev)
        rec[:, :, :H, :W] = img.float() / 255 * 2 - 1 + 0.05 * torch.randn((B, 3, H, W), generator=gen, device=dev)
        size = (H, W)
        ps = timed(lambda: metrics.psnr(un, rec, img, size=size), a.reps)
        ms = timed(lambda: metrics.ms_ssim(un, rec, img, size=size), a.reps)
        both = timed(lambda: metrics.distortion(un, rec, img, size=size), a.reps)
        nbytes = B * 3 * H * W * 5
        ctx = [torch.randn((B, c, Hp >> l, Wp >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
        init = torch.randn((B, 3, Hp, Wp), generator=gen, device=dev) * 0.8
        diff.decompress(ctx, (B, 3, Hp, Wp), sample_steps=2, init=init)
        torch.cuda.synchronize()
        t = time.perf_counter()
        diff.decompress(ctx, (B, 3, Hp, Wp), sample_steps=a.decode_steps, init=init)
        torch.cuda.synchronize()
        it_ms = (time.perf_counter() - t) / a.decode_steps * 1e3
        f = lambda v: f"{v[0]:.0f} us ({v[1]:.0f} .. {v[2]:.0f})"      # noqa: E731
        lines.append(f"| {H} x {W} ({Hp} x {Wp}) | {nbytes / 1e6:.1f} MB | {nbytes / gbs / 1e3:.1f} us | {f(ps)} | {f(ms)} | {f(both)} | "
                     f"{it_ms:.2f} | {both[0] / (500 * it_ms * 1e3) * 100:.4f} % |")
    lines += ["", f"Floor of a call (PSNR of one 1 x 1 image: two launches, the result copy, the synchronisation, the Python layer): {floor[0]:.0f} us "
              f"({floor[1]:.0f} .. {floor[2]:.0f})."]
    if a.notes and os.path.exists(a.notes):
        lines += ["", open(a.notes).read().rstrip()]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
