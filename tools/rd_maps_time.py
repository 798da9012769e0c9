"""Device-event timings of cdc_rate_map against cdc_bpp and of cdc_distortion_map against cdc_distortion(PSNR).
usage: python tools/rd_maps_time.py [reps] [out.txt]   (profiles/rd_maps.md holds a run)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cdc_compression_amd as cdc                     # noqa: E402
import rate_ref as R                                  # noqa: E402
from cdc_compression_amd import _lib, synth           # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
OUT = sys.argv[2] if len(sys.argv) > 2 else None

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps=REPS, warm=10, burst=20):
    """fns: {name: callable}; alternating, one event pair per call -> {name: (median, p10, p90) in us}; and per-call us of a burst."""
    st = torch.cuda.current_stream()
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st); f(); b.record(st)
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3)
    out = {}
    for k, f in fns.items():
        bursts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(burst):
                f()
            b.record(st)
            b.synchronize()
            bursts.append(a.elapsed_time(b) * 1e3 / burst)
        v = np.array(res[k])
        out[k] = (float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90)), float(np.median(bursts)))
    return out


def rate_side(B, H, W):
    m = cdc.ResnetCompressor(dim=64)                       # the published x-param sizes: CH = CL = 256
    CH, CL = m.reversed_hyper_dims[0], m.reversed_hyper_dims[-1] // 2
    man = m.hyper_manifest()
    m.load_hyper_state_dict({**synth.unet_state_dict(man, seed=7), **R.prior_sd(C=CH)})
    hh, wh = H // 64, W // 64
    rng = np.random.default_rng(B * 1000 + H)
    qh = (R.medians(CH)[None, :, None, None] + np.rint(rng.standard_normal((B, CH, hh, wh)))).astype(np.float32)
    mu = rng.standard_normal((B, CL, 4 * hh, 4 * wh)).astype(np.float32) * 2
    ql = (mu + np.rint(rng.standard_normal(mu.shape) * 3.0)).astype(np.float32)
    sc = np.full(mu.shape, 3.0, np.float32)
    d = [torch.from_numpy(a).cuda() for a in (qh, ql, mu, sc)]
    L, h = _lib.lib(), m._hyper_handle()
    nl, nh = 4 * hh * 4 * wh, hh * wh
    o = [torch.empty(n, dtype=torch.float32, device="cuda") for n in (B * nl, B * nh, B * nl, B * CL, B * CH)]
    bpp = torch.empty(B, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = [t.data_ptr() for t in d]

    def f_bpp():
        assert L.cdc_bpp(h, *p, bpp.data_ptr(), B, hh, wh, H, W, 1, st) == 0

    def f_cell():
        assert L.cdc_rate_map(h, *p, None, None, o[2].data_ptr(), None, None, B, hh, wh, 1, st) == 0

    def f_all():
        assert L.cdc_rate_map(h, *p, *[t.data_ptr() for t in o], B, hh, wh, 1, st) == 0

    r = timed({"cdc_bpp": f_bpp, "rate_map cell only": f_cell, "rate_map all five": f_all})
    torch.cuda.synchronize()
    tot = o[2].double().view(B, -1).sum(1).cpu().numpy()
    ref = bpp.double().cpu().numpy() * (H * W)
    say(f"rate side, batch {B} at {H} x {W} (latent {CL} x {4 * hh} x {4 * wh}, hyper {CH} x {hh} x {wh}); sum(cell) / (bpp H W) - 1 = {float(np.abs(tot / ref - 1).max()):.2e}")
    for k, (med, lo, hi, burst) in r.items():
        say(f"    {k:22s} median {med:9.1f} us  (p10 {lo:9.1f}, p90 {hi:9.1f}; {REPS} single calls)   {burst:9.1f} us per call in bursts of 20")


def error_side(B, H, W):
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    rng = np.random.default_rng(B * 1000 + H + 1)
    a = torch.from_numpy(rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)).cuda()
    u = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)).cuda()
    u2 = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)).cuda()
    L, h = _lib.lib(), un._handle()
    gh, gw = H // 16, W // 16
    sse = torch.empty(B * gh * gw, dtype=torch.float64, device="cuda")
    cnt = torch.empty(B * gh * gw, dtype=torch.int32, device="cuda")
    ps = (ctypes.c_double * B)()
    st = torch.cuda.current_stream().cuda_stream
    for tag, x, y, saved in (("float32 / uint8", a, u, 0), ("uint8 / uint8 (exact)", u, u2, 0)):
        va = _lib.ImageView(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, H, W, saved)
        vb = _lib.ImageView(y.data_ptr(), 1, H, W, 0)

        def f_psnr():
            assert L.cdc_distortion(h, ctypes.byref(va), ctypes.byref(vb), B, H, W, 1, ps, None, None, 1, st) == 0

        def f_map():
            assert L.cdc_distortion_map(h, ctypes.byref(va), ctypes.byref(vb), B, H, W, 16, gh, gw, sse.data_ptr(), cnt.data_ptr(), 1, st) == 0

        r = timed({"cdc_distortion(PSNR)": f_psnr, "cdc_distortion_map c=16": f_map})
        say(f"error side, batch {B} at {H} x {W}, {tag} (cdc_distortion synchronises and copies its result back inside the call)")
        for k, (med, lo, hi, burst) in r.items():
            say(f"    {k:24s} median {med:9.1f} us  (p10 {lo:9.1f}, p90 {hi:9.1f})   {burst:9.1f} us per call in bursts of 20")


say(f"device: {torch.cuda.get_device_name(0)}; device events around each call on the caller's stream, device-memory operands")
for B, H, W in ((32, 256, 256), (1, 2048, 2048)):
    rate_side(B, H, W)
for B, H, W in ((32, 256, 256), (1, 2048, 2048)):
    error_side(B, H, W)
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
