"""Timings of the rate-distortion optimised quantiser against cdc_bpp on the same shapes, and the default ladder on the small synthetic
model.  usage: python tools/rdo_time.py [reps] [out.txt]   (profiles/rdo_quant.md holds a run)

cdc_entropy_rate_sweep and cdc_entropy_encode are synchronous entry points (front end: hyper symbols, hyper_dec, then the kernels, then
the copy back): they are timed with a host clock around the call.  cdc_bpp is timed with device events, as tools/rd_maps_time.py does.
The kernels alone (rdo_sweep_kernel, latent_symbols_rdo_kernel, latent_symbols_kernel, rdo_quantize_kernel, bpp_kernel) come from a
kernel trace of this script, taken in a run of its own."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cdc_compression_amd as cdc                     # noqa: E402
import metrics_ref as M                               # noqa: E402
import rate_ref as R                                  # noqa: E402
from cdc_compression_amd import _lib, compressor as C, synth   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def host_timed(f, reps=REPS, warm=3):
    for _ in range(warm):
        f()
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        v.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def event_timed(f, reps=REPS, warm=5):
    st = torch.cuda.current_stream()
    for _ in range(warm):
        f()
    v = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); f(); b.record(st)
        b.synchronize()
        v.append(a.elapsed_time(b) * 1e3)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def shape(B, H, W):
    m = cdc.ResnetCompressor(dim=64)                       # the published x-param sizes: CH = CL = 256
    dims = tuple(m.reversed_hyper_dims)
    CH, CL = dims[0], dims[-1] // 2
    rng = np.random.default_rng(B * 1000 + H)
    mean_bias = (2.0 * rng.standard_normal(CL)).astype(np.float32)
    # hyper_dec with zero weights: mean and scale are its last bias (3.0: the `typical` class of tests/rate_ref.py)
    m.load_hyper_state_dict({**R.zero_weight_hyper_sd(mean_bias, np.full(CL, 3.0, np.float32), dims=dims), **R.prior_sd(C=CH),
                             "prior._medians": R.medians(CH)})
    hh, wh = H // 64, W // 64
    hyper = (R.medians(CH)[None, :, None, None] + rng.standard_normal((B, CH, hh, wh))).astype(np.float32)
    latent = (mean_bias[None, :, None, None] + 3.0 * rng.standard_normal((B, CL, 4 * hh, 4 * wh))).astype(np.float32)
    dl, dh = torch.from_numpy(latent).cuda(), torch.from_numpy(hyper).cuda()
    mus = C.RDO_LADDER
    say(f"batch {B} at {H} x {W}: latent {CL} x {4 * hh} x {4 * wh} ({latent[0].size} symbols an image), hyper {CH} x {hh} x {wh}")
    t = m._sweep(dl, dh, mus)
    say(f"    the ladder 2^-8 .. 2^8 on N(mean, 3) latents at scale 3: bits / symbol {t['bits'][0, 0] / latent[0].size:.3f} -> "
        f"{t['bits'][0, -1] / latent[0].size:.3f}, moved {t['moved'][0, 0]} -> {t['moved'][0, -1]}")
    r = host_timed(lambda: m._sweep(dl, dh, mus))
    say(f"    cdc_entropy_rate_sweep L = 17   median {r[0]:10.1f} us (p10 {r[1]:.1f}, p90 {r[2]:.1f}) whole call, host clock")
    r1 = host_timed(lambda: m._sweep(dl, dh, mus[:1]))
    say(f"    cdc_entropy_rate_sweep L = 1    median {r1[0]:10.1f} us (p10 {r1[1]:.1f}, p90 {r1[2]:.1f})")
    e0 = host_timed(lambda: m.latents_to_bytes(dl, dh))
    e1 = host_timed(lambda: m.latents_to_bytes(dl, dh, rdo=1.0))
    say(f"    latents_to_bytes plain          median {e0[0]:10.1f} us;  rdo=1.0 {e1[0]:10.1f} us (whole calls, coder and copies included)")
    q, qh = m.decompress_from_bytes(m.latents_to_bytes(dl, dh), like=dl, return_hyper=True)
    mean, scale = m.hyper_decode(qh)
    L, h = _lib.lib(), m._hyper_handle()
    bpp = torch.empty(B, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def f_bpp():
        assert L.cdc_bpp(h, qh.data_ptr(), q.data_ptr(), mean.data_ptr(), scale.data_ptr(), bpp.data_ptr(), B, hh, wh, H, W, 1, st) == 0
    b = event_timed(f_bpp)
    say(f"    cdc_bpp                         median {b[0]:10.1f} us (p10 {b[1]:.1f}, p90 {b[2]:.1f}) device events")
    o = host_timed(lambda: m.rdo_quantize(dl, mean, scale, 1.0))
    say(f"    cdc_op_rdo_quantize             median {o[0]:10.1f} us whole call (operand check, kernel, count read back)")
    torch.cuda.synchronize()
    ref = bpp.double().cpu().numpy() * (H * W)
    say(f"    sweep column mu = 2^-8 against cdc_bpp H W of the plain symbols: {float(np.abs(t['bits'][:, 0] / ref - 1).max()):.2e} relative "
        f"(moved {int(t['moved'][:, 0].max())})")


def small_model_ladder():
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest_vbr_small.json")))
    sd = synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"])
    comp = cdc.BigCompressor(vbr=False, **meta["kwargs"])
    comp.load_state_dict({k: v for k, v in sd.items() if not synth.is_vbr_key(k)})
    img = (2.0 * M.noisy(M.picture(3, 128, 192, seed=3), 0.08, 5) - 1.0).astype(np.float32)
    ladder = np.concatenate([np.zeros(1, np.float32), C.RDO_LADDER])
    t = comp.rate_sweep(img, ladder)
    say("the default ladder on the small synthetic BigCompressor (tests/golden/manifest_vbr_small.json), image 0 of a 3 x 128 x 192 batch, "
        f"{3072} latent symbols; stream bytes from an encode at that mu:")
    say("        mu    est. bpp   bits saved   moved   latent mse   stream bytes")
    for j, mu in enumerate(ladder):
        n = len(comp.compress_to_bytes(img[:1], rdo=float(mu))[0])
        say(f"    {mu:8.4f}  {t['bpp'][0, j]:8.4f}   {100 * (1 - t['bpp'][0, j] / t['bpp'][0, 0]):8.2f} %  {t['moved'][0, j]:6d}   {t['latent_mse'][0, j]:9.4f}   {n:8d}")


say(f"device: {torch.cuda.get_device_name(0)}")
for B, H, W in ((32, 256, 256), (1, 2048, 2048)):
    shape(B, H, W)
small_model_ladder()
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
