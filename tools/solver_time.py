#!/usr/bin/env python3
"""Per-iteration time of the multistep sampler kernel against the DDIM kernel's at BASELINE configs[1]'s shape (x-param, batch 32,
256 x 256, synthetic weights), from the library's own event timers (cdc_prof_*).

Both decodes run the same U-Net program; an iteration differs in its sampler kernel alone, which is timed in the "small" class with
the iteration's other small launches.  So the figure is the difference of that class's time per iteration between sampler="dpmpp_2m"
and sampler="ddim", beside the class totals and the whole iteration.  The expectation, not a measurement: 8 more bytes per element
(the history read and written), 0.05 GB at this shape.  The rounds alternate the two samplers; medians and spread are printed.

    timeout -k 10 300 python tools/solver_time.py --out profiles/solver_time.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import _lib, synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))


def class_ms(h):
    """{class name: (ms, launches)} since the last reset."""
    L, out = _lib.lib(), {}
    for c in range(L.cdc_prof_num_classes()):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        _lib.check(h, L.cdc_prof_get(h, c, ctypes.byref(ms), ctypes.byref(n), None, None))
        out[L.cdc_prof_name(c).decode()] = (ms.value, n.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sample-steps", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=5)
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
    L, h = _lib.lib(), un._handle()
    run = lambda sampler, n: diff.decompress(ctx, (B, 3, S, S), sample_steps=n, init=init, sampler=sampler, spacing="logsnr")   # noqa: E731
    for s in ("ddim", "dpmpp_2m"):
        run(s, 3)
    torch.cuda.synchronize()
    small, total = {"ddim": [], "dpmpp_2m": []}, {"ddim": [], "dpmpp_2m": []}
    for _ in range(a.rounds):
        for s in ("ddim", "dpmpp_2m"):
            L.cdc_prof_reset(h)
            L.cdc_prof_enable(h, 1)
            out = run(s, steps)
            torch.cuda.synchronize()
            cm = class_ms(h)
            L.cdc_prof_enable(h, 0)
            assert bool(torch.isfinite(out).all().item())
            # (the hoisted context convolutions run once per decode, unprofiled; every class here is per-iteration work)
            small[s].append(cm["small"][0] / steps)
            total[s].append(sum(v[0] for v in cm.values()) / steps)
    n = B * 3 * S * S
    med = statistics.median
    lines = [f"sampler kernel time from cdc_prof_*, ms per iteration ({steps}-step decodes on the logSNR grid, batch {B}, {S} x {S}, x-param, synthetic weights)",
             f"device: {torch.cuda.get_device_name(0)}; {L.cdc_version().decode()}; kernels {_lib.kernel_source_hash()}",
             f"handle after the runs: {un.status()}"]
    for s in ("ddim", "dpmpp_2m"):
        lines.append(f"{s:<9s} class \"small\" median {med(small[s]):7.4f}  min {min(small[s]):7.4f}  max {max(small[s]):7.4f}   "
                     f"all classes median {med(total[s]):8.4f}  min {min(total[s]):8.4f}  max {max(total[s]):8.4f}   n = {len(small[s])}")
    d = med(small["dpmpp_2m"]) - med(small["ddim"])
    lines.append(f"dpmpp_2m - ddim, class \"small\": {d * 1e3:+.1f} us per iteration "
                 f"({d / med(total['ddim']) * 100:+.3f} % of a DDIM iteration's kernel time); expected from 8 more bytes per element "
                 f"({8 * n / 1e9:.3f} GB): {8 * n / 4.0e12 * 1e6:.0f} us at 4 TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
