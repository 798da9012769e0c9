#!/usr/bin/env python3
"""Time of SimpleCompressor (the GDN context model of the epsilon tree) beside BigCompressor(vbr=False) with the same arguments:
`encode(images)` and `decode(q_latent)` at batch 32, 256 x 256, dim 64, device tensors, in milliseconds per call (each call
synchronises), and the GDN kernel's achieved bytes per second -- per layer, from the library's event timing of the launch
programs -- beside the same run's cdc_probe_hbm_copy rate.  No bar is set on these figures: BigCompressor's time is the yardstick
they are printed against.  Writes --out (profiles/simple_compressor.md).  Under a minute:

    timeout -k 10 300 python tools/simple_compressor_time.py --out profiles/simple_compressor.md
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import synth  # noqa: E402

KW = dict(dim=64, dim_mults=(1, 2, 3, 3), hyper_dims_mults=(3, 3, 3), channels=3, out_channels=3)


def timed(fn, reps, rounds=5):
    """Median over `rounds` of the mean time of `reps` calls, in milliseconds."""
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / reps * 1e3)
    return statistics.median(out), min(out), max(out)


def full_manifest(m):
    return m.encoder_manifest() + m.hyper_manifest() + m.manifest()


def gdn_ops(L, h):
    """[(label, ms per launch, launches)] of the GDN ops of a handle's current program."""
    out = []
    for i in range(L.cdc_prof_num_ops(h)):
        lab, ms, n = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        L.cdc_prof_op(h, i, ctypes.byref(lab), ctypes.byref(ms), ctypes.byref(n), None)
        if lab.value.decode().startswith("gdn") and n.value:
            out.append((lab.value.decode(), ms.value / n.value, n.value))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--notes", default=None, help="a text file appended to the report (the parity figures of the GPU tests)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    L = cdc._lib.lib()
    rate = ctypes.c_double()
    assert L.cdc_probe_hbm_copy(0, 1 << 28, 5, ctypes.byref(rate)) == 0
    gbs = rate.value
    simple = cdc.epsilonparam.SimpleCompressor(**KW)
    simple.load_state_dict(synth.simple_compressor_state_dict(full_manifest(simple), seed=1))
    big = cdc.BigCompressor(vbr=False, **KW)
    big.load_state_dict(synth.compressor_state_dict(full_manifest(big), seed=1))
    gen = torch.Generator(device=dev).manual_seed(5)
    x = (torch.rand((B, 3, S, S), generator=gen, device=dev) * 2 - 1).contiguous()
    n = len(KW["dim_mults"])
    q = torch.round(torch.randn((B, KW["dim"] * KW["dim_mults"][-1], S >> n, S >> n), generator=gen, device=dev) * 2).contiguous()
    lines = ["# SimpleCompressor beside BigCompressor: time per call", "",
             f"device: {torch.cuda.get_device_name(0)}; {L.cdc_version().decode()}; kernels {cdc._lib.kernel_source_hash()}",
             f"cdc_probe_hbm_copy of this run: {gbs:.0f} GB/s (read + written bytes)", "",
             f"Batch {B}, {S} x {S}, {KW}, device tensors, median (min .. max) over 5 rounds of {a.reps} calls.", "",
             "| call | SimpleCompressor | BigCompressor(vbr=False) |", "|---|---|---|"]
    f = lambda v: f"{v[0]:.2f} ms ({v[1]:.2f} .. {v[2]:.2f})"      # noqa: E731
    lines.append(f"| encode(images) | {f(timed(lambda: simple.encode(x), a.reps))} | {f(timed(lambda: big.encode(x), a.reps))} |")
    lines.append(f"| decode(q_latent) | {f(timed(lambda: simple.decode(q), a.reps))} | {f(timed(lambda: big.decode(q), a.reps))} |")
    # the GDN kernel, per layer: event time of the launch programs
    lines += ["", "GDN kernel per layer (event timing of the launch program; bytes = x read once + y written once):", "",
              "| program | layer | us per launch | GB/s | share of the copy rate | TFLOP/s on the fp32 matrix pipe |", "|---|---|---|---|---|---|"]
    for name, h, run in (("encoder", simple._enc_handle(), lambda: simple.analysis(x)), ("context decoder", simple._handle(), lambda: simple.decode(q))):
        L.cdc_prof_reset(h)
        L.cdc_prof_enable(h, 1)
        for _ in range(a.reps):
            run()
        torch.cuda.synchronize()
        for lab, ms, cnt in gdn_ops(L, h):
            parts = dict(p.split("=") for p in lab.split()[1:3])
            nbytes = 8.0 * B * int(parts["C"]) * int(parts["HW"])
            g = nbytes / (ms * 1e-3) / 1e9
            tf = 2.0 * B * int(parts["HW"]) * int(parts["C"]) ** 2 / (ms * 1e-3) / 1e12
            lines.append(f"| {name} | {lab} | {ms * 1e3:.1f} | {g:.0f} | {g / gbs * 100:.0f} % | {tf:.1f} |")
        L.cdc_prof_enable(h, 0)
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
