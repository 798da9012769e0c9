#!/usr/bin/env python3
"""What a decode trajectory costs: wall time of a whole decode (x-param, 256 x 256, synthetic weights, device tensors) without a
trace, with x0 of every 8th step (float32 and uint8 slots), with x0 of every step, with x_t of every 8th step, and the same x_t images
obtained the old way -- one cdc_ddim_step call per step from the host, cloning the state at the chosen steps (that path has no x0
at all).  Each figure is the median of `--rounds` runs, with min and max.  Beside them, from the library's event timers (cdc_prof_*)
on a short decode: the launch counts, and the tap kernel's own time per slot as the difference of the "small" class.

`--plain-only` times the plain decode alone; copied into a checkout of the parent commit (whose library has no trace: the script
then runs that arm only) it gives the parent's figures, which is how the "same launches, time inside the parent's own spread" claim is
checked: parent, this build, parent again, on the same box.  `--out` appends.

    timeout -k 10 900 python tools/trace_time.py --out profiles/trace_time.txt
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
from cdc_compression_amd import _lib, synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))


def class_table(h):
    """{class name: (ms, launches)} since the last reset."""
    L, out = _lib.lib(), {}
    for c in range(L.cdc_prof_num_classes()):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        _lib.check(h, L.cdc_prof_get(h, c, ctypes.byref(ms), ctypes.byref(n), None, None))
        out[L.cdc_prof_name(c).decode()] = (ms.value, n.value)
    return out


def stepped(diff, un, ctx, init, steps, every):
    """The old way: cdc_ddim_step per step on device tensors, the state cloned at the steps `trajectory=every` would record."""
    L, h = _lib.lib(), un._handle()
    B, _, H, W = init.shape
    ptrs = (ctypes.c_void_p * len(ctx))(*[c.data_ptr() for c in ctx])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = set(range(steps - 1, -1, -every)) | {0}
    img, out, slots = init, torch.empty_like(init), []
    for i in reversed(range(steps)):
        # (the context goes in with the first step only: the later calls keep what is staged, as a careful caller would)
        _lib.check(h, L.cdc_ddim_step(h, img.data_ptr(), i, ptrs if i == steps - 1 else None, len(ctx), None, 0.0, out.data_ptr(), B, H, W,
                                      _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, _lib.CDC_MEM_DEVICE, st))
        img, out = out, (torch.empty_like(init) if img is init else img)
        if i in keep:
            slots.append(img.clone())
    return img, torch.stack(slots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sample-steps", type=int, default=65)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prof-steps", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    S, steps, every = a.size, a.sample_steps, a.every
    L = _lib.lib()
    traced_build = hasattr(L, "cdc_set_trace")
    lines = [f"decode trajectory: wall ms per {steps}-step decode, median of {a.rounds} (min .. max); x-param, {S} x {S}, device tensors, synthetic weights",
             f"device: {torch.cuda.get_device_name(0)}; {L.cdc_version().decode()}; kernels {_lib.kernel_source_hash()}; library {os.path.basename(_lib.LIB_PATH)}"
             f"{'' if traced_build else ' (a build without the trace)'}"]
    for B in a.batches:
        un = cdc.Unet(**KW)
        un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
        diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
        gen = torch.Generator(device=dev).manual_seed(77)
        init = torch.randn((B, 3, S, S), generator=gen, device=dev) * 0.8
        ctx = [torch.randn((B, c, S >> l, S >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
        h = un._handle()
        dec = lambda n=steps, **kw: diff.decompress(ctx, (B, 3, S, S), sample_steps=n, init=init, **kw)   # noqa: E731
        arms = [("plain decode", lambda: dec())]
        if traced_build and not a.plain_only:
            arms += [(f"x0 every {every}th step, float32", lambda: dec(trajectory=every)),
                     (f"x0 every {every}th step, uint8", lambda: dec(trajectory=every, trajectory_dtype="uint8")),
                     ("x0 every step, float32", lambda: dec(trajectory=1)),
                     ("x0 every step, uint8", lambda: dec(trajectory=1, trajectory_dtype="uint8")),
                     (f"x_t every {every}th step, float32", lambda: dec(trajectory=every, trajectory_of="x_t"))]
        if not a.plain_only:
            diff.set_sample_schedule(steps)
            arms.append((f"x_t every {every}th step the old way (cdc_ddim_step per step)", lambda: stepped(diff, un, ctx, init, steps, every)))
        dec(3)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in arms}
        for _ in range(a.rounds):                      # the arms alternate inside a round
            for name, fn in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        lines.append(f"batch {B}:")
        base = statistics.median(times["plain decode"])
        for name, _ in arms:
            t = times[name]
            m = statistics.median(t)
            lines.append(f"  {name:<62s} {m:10.2f}  ({min(t):.2f} .. {max(t):.2f})  {m - base:+9.2f} ms  {(m / base - 1) * 100:+6.2f} %")
        # launches and the tap's own time, from the event timers, on a short decode
        n = a.prof_steps
        prof = {}
        for name, kw in [("plain", {})] + ([("x0 every step, float32", dict(trajectory=1)),
                                            ("x0 every step, uint8", dict(trajectory=1, trajectory_dtype="uint8"))]
                                           if traced_build and not a.plain_only else []):
            L.cdc_prof_reset(h)
            L.cdc_prof_enable(h, 1)
            dec(n, **kw)
            torch.cuda.synchronize()
            prof[name] = class_table(h)
            L.cdc_prof_enable(h, 0)
        p0 = prof["plain"]
        lines.append(f"  launches of a {n}-step plain decode (hoisted context part not counted): {sum(v[1] for v in p0.values())}  "
                     + " ".join(f"{k}={v[1]}" for k, v in p0.items() if v[1]))
        elems = B * 3 * S * S
        for name, tab in prof.items():
            if name == "plain":
                continue
            extra = sum(v[1] for v in tab.values()) - sum(v[1] for v in p0.values())
            us = (tab["small"][0] - p0["small"][0]) / n * 1e3
            nbytes = elems * (4 * 7 + 4 + (1 if "uint8" in name else 4))
            lines.append(f"  {name}: {extra:+d} launches over {n} steps; class \"small\" {us:+.1f} us per slot; the tap moves "
                         f"{nbytes / elems:.0f} bytes per element (7 planes + x read, the slot written) = {nbytes / 1e6:.1f} MB: "
                         f"{nbytes / max(us, 1e-9) / 1e3:.0f} GB/s")
        lines.append(f"  handle after the runs: {un.status()}")
        del un, diff, ctx, init
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
