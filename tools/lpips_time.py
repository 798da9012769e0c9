#!/usr/bin/env python3
"""Time of cdc_lpips (device pointers) at batch 32, 256 x 256 and 500 x 333: milliseconds per call as a user makes it (the launches
of every chunk, the copy of the results to the host and the stream synchronisation it ends in), on the operands evaluate() compares
-- the float32 padded decoder frame against the uint8 image.  Beside it: the convolutions' executed flops and their rate, the
activation bytes of a pair and the chunking, a per-op table from the library's event pairs (cdc_prof_op: the op's kernels plus ~4 us
of the pair), and the time of one DDIM iteration of the full x-param model at the same shape, measured in the same run, so that the
call stands next to a 500-step decode.  Writes --out (profiles/lpips.md takes the tables).

    timeout -k 10 900 python tools/lpips_time.py --out lpips_time.md

--dump-ops FILE / --calls N: write the launch program's op labels of --size and make N calls and nothing else -- the workload of
    rocprofv3 --kernel-trace -- python tools/lpips_time.py --size 256x256 --calls 3 --dump-ops ops.txt
whose CSV tools/trace_by_op.py --start-kernel lpips_in_kernel turns into a per-op table (one segment per chunk)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))
BUDGET = 4096 << 20           # the chunk budget of cdc_lpips (include/cdc_hip.h)


def conv_flops(H, W):
    fl, h, w = 0.0, H, W
    for l, idx in enumerate(((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))):
        if l:
            h, w = h // 2, w // 2
        for i in idx:
            _, _, cin, cout = synth.LPIPS_VGG_CONVS[i]
            fl += 2.0 * 9 * cin * cout * h * w
    return fl


def pair_bytes(H, W):
    px, h, w = 3 * H * W, H, W
    for l, (n, c) in enumerate(zip((2, 2, 3, 3, 3), synth.LPIPS_VGG_TAP_CHANNELS)):
        if l:
            h, w = h // 2, w // 2
            px += synth.LPIPS_VGG_TAP_CHANNELS[l - 1] * h * w
        px += n * c * h * w
    px += 2 * 256 * (H // 4) * (W // 4)          # the two partial-sum buffers of the sliced layers
    return 2 * px * 4


def operands(B, H, W, Hp, Wp, dev, gen):
    img = torch.randint(0, 256, (B, 3, H, W), generator=gen, device=dev, dtype=torch.uint8)
    rec = torch.zeros((B, 3, Hp, Wp), device=dev)
    rec[:, :, :H, :W] = img.float() / 255 * 2 - 1 + 0.05 * torch.randn((B, 3, H, W), generator=gen, device=dev)
    return rec, img


def op_table(model):
    L, h = cdc._lib.lib(), model._ready()
    out = []
    for i in range(L.cdc_prof_num_ops(h)):
        label, ms, n, fl = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        L.cdc_prof_op(h, i, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
        out.append((label.value.decode(), ms.value, n.value, fl.value))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--decode-steps", type=int, default=4)
    ap.add_argument("--size", default=None, help="HxW: only this size")
    ap.add_argument("--calls", type=int, default=0, help="make this many calls and nothing else (the workload of a kernel trace)")
    ap.add_argument("--dump-ops", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    B = a.batch
    L = cdc._lib.lib()
    model = cdc.LpipsVGG().load_state_dict(synth.lpips_vgg_state_dict(seed=0))
    gen = torch.Generator(device=dev).manual_seed(5)
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else [(256, 256), (500, 333)]
    if a.calls:
        H, W = sizes[0]
        rec, img = operands(B, H, W, -(-H // 64) * 64, -(-W // 64) * 64, dev, gen)
        for _ in range(a.calls):
            model(rec, img, size=(H, W), as_saved=True)
        if a.dump_ops:
            with open(a.dump_ops, "w") as f:
                f.write("\n".join(lab for lab, _, _, _ in op_table(model)) + "\n")
        return
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    lines = ["# cdc_lpips: time per call", "",
             f"device: {torch.cuda.get_device_name(0)}; {L.cdc_version().decode()}; kernels {cdc._lib.kernel_source_hash()}", "",
             f"Batch {B}, device pointers, float32 padded frame (as saved) against the uint8 image, median (min .. max) of {a.reps} calls after a",
             "warm-up call.  A call ends in the copy of its results to the host and a stream synchronisation.", "",
             "| image (frame) | activations per pair | chunks x pairs | convolution work per call | call | convolution rate over the call | ms per DDIM iteration | share of a 500-step decode |",
             "|---|---|---|---|---|---|---|---|"]
    tables = []
    for H, W in sizes:
        Hp, Wp = diff.padded_size(H, W)
        rec, img = operands(B, H, W, Hp, Wp, dev, gen)
        fn = lambda: model(rec, img, size=(H, W), as_saved=True)          # noqa: E731
        fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        h = model._ready()
        L.cdc_prof_reset(h)
        L.cdc_prof_enable(h, 1)
        fn()
        ops = op_table(model)
        L.cdc_prof_enable(h, 0)
        tables.append((H, W, ops))
        ctx = [torch.randn((B, c, Hp >> l, Wp >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
        init = torch.randn((B, 3, Hp, Wp), generator=gen, device=dev) * 0.8
        diff.decompress(ctx, (B, 3, Hp, Wp), sample_steps=2, init=init)
        torch.cuda.synchronize()
        t = time.perf_counter()
        diff.decompress(ctx, (B, 3, Hp, Wp), sample_steps=a.decode_steps, init=init)
        torch.cuda.synchronize()
        it_ms = (time.perf_counter() - t) / a.decode_steps * 1e3
        del ctx, init
        pb = pair_bytes(H, W)
        max_pairs = max(1, min(B, BUDGET // pb))
        nch = -(-B // max_pairs)
        fl = conv_flops(H, W) * 2 * B
        lines.append(f"| {H} x {W} ({Hp} x {Wp}) | {pb / 1e9:.3f} GB | {nch} x {-(-B // nch)} | {fl / 1e12:.2f} TFLOP | {med:.1f} ms ({lo:.1f} .. {hi:.1f}) | "
                     f"{fl / med / 1e9:.0f} TFLOP/s | {it_ms:.2f} | {med / (500 * it_ms) * 100:.3f} % |")
    for H, W, ops in tables:
        tot = sum(ms for _, ms, _, _ in ops)
        lines += ["", f"## Per op, {H} x {W}, batch {B}: event pairs around every launch of one call (sum {tot:.1f} ms; launches = chunks)", "",
                  "| op | launches | ms per call | TFLOP/s |", "|---|---|---|---|"]
        for lab, ms, n, f in ops:
            lines.append(f"| `{lab}` | {n} | {ms:.3f} | {f * n / ms / 1e9:.0f} |" if f else f"| `{lab}` | {n} | {ms:.3f} | |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
