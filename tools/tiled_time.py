#!/usr/bin/env python3
"""What the tiled decode costs, on the published x-param configuration with synthetic weights, device tensors:

  decode   one S x S image from its q_latent, 8 steps, seed / gamma 0.8: the whole frame against tile=256 and tile=512 (overlap 64),
           and a 512 x 512 region of each -- ms per iteration (wall time of a call that ends in a synchronise / steps) and the device
           memory in use after the call (hipMemGetInfo, total - free: the handles keep the activations of their launch programs, so
           this is the footprint of the weights and the programs of the call, not a sampled peak; every configuration runs on fresh
           handles).
           --sizes gives S (default 1024, 2048); the whole frame runs only up to --whole-max (default 1024).
  kernels  cdc_tile_gather and cdc_tile_blend for the 2048 x 2048 image at tile 256 / overlap 64 (event time of one call, bytes each
           has to move) against cdc_probe_hbm_copy of the same box.
  step     the DDIM update kernel at 32 x 3 x 256 x 256, eta 0.5: seeded (the image's own tensor indexes the draws) against framed
           (cdc_set_noise_frames), alternating, event time.  On a build without the framed entry points only the seeded one runs.

    timeout -k 10 900 python tools/tiled_time.py --out profiles/tiled_time.txt [--what decode,kernels,step]
"""
import argparse
import ctypes
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import _lib, synth  # noqa: E402

U64P = ctypes.POINTER(ctypes.c_uint64)


def model(dev):
    un = cdc.Unet(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    comp = cdc.ResnetCompressor(dim=64, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=64)
    comp.load_state_dict(synth.unet_state_dict(comp.manifest(), seed=15))
    return cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine"), un, comp


def used_gib():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 30


def decode_table(dev, sizes, whole_max, steps, reps):
    lines = []
    for S in sizes:
        region = (S // 2 - 256 + 32, S // 2 - 256 + 32, 512, 512)
        configs = [("whole frame", {})] if S <= whole_max else []
        for t in (256, 512):
            configs += [(f"tile {t} overlap 64", dict(tile=t, tile_overlap=64)), (f"tile {t} overlap 64, region 512 x 512", dict(tile=t, tile_overlap=64, region=region))]
        if S > whole_max:
            lines.append(f"S = {S}: whole frame not measured (--whole-max {whole_max})")
        for name, kw in configs:
            base = used_gib()
            diff, un, comp = model(dev)
            gen = torch.Generator(device=dev).manual_seed(77)
            q = torch.randint(-8, 9, (1, comp.reversed_dims[0], S // 16, S // 16), generator=gen, device=dev).float()
            args = dict(seed=1000, gamma=0.8, **kw)
            diff.decompress(q, sample_steps=2, **args)                              # launch programs, code pages
            torch.cuda.synchronize()
            ts, info = [], None
            for _ in range(reps):
                t0 = time.perf_counter()
                out = diff.decompress(q, sample_steps=steps, **args)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / steps)
            if "region" in kw:
                out, info = out
            assert bool(torch.isfinite(out).all().item()) and un.status()["range_faults"] == 0, un.status()
            mem = used_gib() - base
            tiles_txt = "" if info is None else f"   {info['tiles_decoded']} of {info['tiles']} tiles"
            lines.append(f"S = {S:4d}  {name:<38s} median {statistics.median(ts):9.2f}  min {min(ts):9.2f}  max {max(ts):9.2f} ms / iteration   "
                         f"{mem:6.2f} GiB in use after the call   n = {reps}{tiles_txt}")
            print(lines[-1], flush=True)
            del diff, un, comp, q, out
            gc.collect()
    return lines


def event_ms(call, reps):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def kernel_table(dev, reps):
    from cdc_compression_amd import tiles
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    h = un._handle()
    S = 2048
    plan = tiles.Plan(S, S, (256, 256), (64, 64))
    lat = torch.randn((1, 256, S // 16, S // 16), device=dev)
    img = torch.randn((1, 3, S, S), device=dev)
    dec = torch.randn((plan.T, 3, 256, 256), device=dev)
    lo = [(y // 16, x // 16) for y, x in plan.origins()]
    calls = {
        f"tile_gather latent 256 ch, {plan.T} tiles of 16 x 16": (lambda: tiles.gather(h, lat, lo, 16, 16, 0), 2 * 4 * plan.T * 256 * 16 * 16),
        f"tile_gather pixels 3 ch, {plan.T} tiles of 256 x 256": (lambda: tiles.gather(h, img, plan.origins(), 256, 256, 0), 2 * 4 * plan.T * 3 * 256 * 256),
        f"tile_blend {plan.T} tiles -> 3 x 2048 x 2048 float32": (lambda: tiles.blend(h, dec, plan, 1, 0), 4 * plan.T * 3 * 256 * 256 + 4 * 3 * S * S),
        f"tile_blend {plan.T} tiles -> 3 x 2048 x 2048 uint8": (lambda: tiles.blend(h, dec, plan, 1, 0, as_uint8=True), 4 * plan.T * 3 * 256 * 256 + 3 * S * S),
    }
    lines = []
    for name, (call, nbytes) in calls.items():
        ms = event_ms(call, reps)
        lines.append(f"{name:<58s} {nbytes / 1e6:8.1f} MB   best {min(ms) * 1e3:8.1f} us  median {statistics.median(ms) * 1e3:8.1f} us   "
                     f"{nbytes / (min(ms) * 1e-3) / 1e9:7.1f} GB/s (best)   n = {reps}   (the event pair spans the Python wrapper: allocation of the result included)")
    gbs = ctypes.c_double()
    assert _lib.lib().cdc_probe_hbm_copy(0, 256 << 20, 5, ctypes.byref(gbs)) == 0
    lines.append(f"cdc_probe_hbm_copy of the same box (256 MiB float4 copy, read + write): {gbs.value:.0f} GB/s")
    return lines


def step_table(dev, reps):
    L = _lib.lib()
    framed = hasattr(L, "cdc_set_noise_frames")
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    diff.set_sample_schedule(8)
    h = un._handle()
    B, S = 32, 256
    fx, x, out = (torch.randn((B, 3, S, S), device=dev) for _ in range(3))
    sd = np.arange(1000, 1000 + B, dtype=np.uint64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step():
        _lib.check(h, L.cdc_op_ddim_update(h, fx.data_ptr(), x.data_ptr(), None, sd.ctypes.data_as(U64P), 0.5, 3, out.data_ptr(), B, 3, S, S,
                                           _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, None, None, 0, 0, _lib.CDC_MEM_DEVICE, st))

    rows = {"seeded": [], "framed": []}
    frames = np.asarray([(2048, 2048, 192 * (b // 8), 192 * (b % 8)) for b in range(B)], np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    for _ in range(5):                                                  # alternating blocks: the spread of the yardstick is in the table
        rows["seeded"] += event_ms(step, reps)
        if framed:
            _lib.check(h, L.cdc_set_noise_frames(h, frames.ctypes.data_as(i32p), B))
            rows["framed"] += event_ms(step, reps)
            _lib.check(h, L.cdc_set_noise_frames(h, None, 0))
    lines = []
    for name, ms in rows.items():
        if ms:
            ms = sorted(ms)
            lines.append(f"ddim update {name:<7s} 32 x 3 x 256 x 256, eta 0.5: median {statistics.median(ms) * 1e3:7.1f} us  min {ms[0] * 1e3:7.1f}  "
                         f"p90 {ms[int(0.9 * len(ms))] * 1e3:7.1f} us   n = {len(ms)}   (event pair around one C call: staging of the seeds included)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="decode,kernels,step")
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--whole-max", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: a time measured elsewhere says nothing about this path")
    dev = torch.device("cuda", 0)
    what = a.what.split(",")
    lines = [f"device: {torch.cuda.get_device_name(0)}; {_lib.lib().cdc_version().decode()}; kernels {_lib.kernel_source_hash()}; library {_lib.LIB_PATH}"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if "step" in what:
        lines += step_table(dev, 40)
        flush()
    if "kernels" in what:
        lines += kernel_table(dev, 20)
        flush()
    if "decode" in what:
        lines.append(f"tiled decode of one S x S image, x-param published configuration, synthetic weights, {a.steps} steps, seed, gamma 0.8, device tensors:")
        lines += decode_table(dev, [int(s) for s in a.sizes.split(",")], a.whole_max, a.steps, a.reps)
        flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
