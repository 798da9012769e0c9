"""Timings and sizes of streams with a grouped hyper part (container versions 19 - 22) against the segmented ones (11 - 14), on
in-model symbols: the sibling of tools/segment_time.py, on its synthetic model.
usage: python tools/hyper_groups_time.py [reps] [out.txt] [base]   (profiles/hyper_groups.md holds a run)

cdc_entropy_encode, cdc_entropy_decode and cdc_entropy_decode_window are synchronous entry points (front end, hyper_dec, the coder's
kernels, the copy back): they are timed with a host clock around the call, on device tensors.  The kernels alone come from a kernel
trace of this script, taken in a run of its own.  `base`: the unsegmented and the segment=128 rows only -- what also runs on a build
without hyper groups, for the comparison against the parent commit; the sha256 printed for them names the bytes."""
import hashlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cdc_compression_amd as cdc                     # noqa: E402
import rate_ref as R                                  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
BASE = len(sys.argv) > 3 and sys.argv[3] == "base"
SEGMENT = 128
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def host_timed(f, reps=REPS, warm=2):
    for _ in range(warm):
        f()
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f})"


def shape(B, H, W, groups, region=None):
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
    say(f"batch {B} at {H} x {W}: latent {CL} x {4 * hh} x {4 * wh}, hyper {CH} x {hh} x {wh} ({hyper[0].size} symbols an image)")
    say("    segment   groups (channels)   encode ms (min .. max)        decode ms (min .. max)        bytes / image   over ungrouped   bound (8 + 12 n - 264 .. 8 + 276 n)")
    cell = m.rate_map_cell
    win = None if region is None else tuple(v // cell for v in region)
    rows = [(None, None), (SEGMENT, None)] + ([] if BASE else [(SEGMENT, G) for G in groups])
    ungrouped = q0 = None
    for segment, G in rows:
        kw = {} if segment is None else {"segment": segment}
        if G is not None:
            kw["hyper_groups"] = G
        streams = m.latents_to_bytes(dl, dh, **kw)
        cg, ng = m.hyper_groups_of(streams)[0] if hasattr(m, "hyper_groups_of") else (0, 1)
        e = host_timed(lambda: m.latents_to_bytes(dl, dh, **kw))
        d = host_timed(lambda: m.decompress_from_bytes(streams, like=dl))
        size = sum(len(s) for s in streams) / B
        q = m.decompress_from_bytes(streams, like=dl)
        q0 = q if q0 is None else q0
        assert torch.equal(q, q0)
        tag = f"{'none' if segment is None else segment:>7}   {'none' if G is None else f'{ng} ({cg})':>17}"
        if G is None:
            ungrouped = size
            say(f"    {tag}   {fmt(e)}   {fmt(d)}   {size:13.1f}   sha256 of the streams {hashlib.sha256(b''.join(streams)).hexdigest()[:16]}")
        else:
            over = size - ungrouped
            lo, hi = 8 + 12 * ng - 264, 8 + 276 * ng
            say(f"    {tag}   {fmt(e)}   {fmt(d)}   {size:13.1f}   {over:+14.1f}   {lo} .. {hi}  {'inside' if lo <= over <= hi else 'OUTSIDE'}")
        if win is not None and segment is not None:
            w = host_timed(lambda: m.decompress_from_bytes(streams, like=dl, window=win))
            _, counts = m.decompress_from_bytes(streams, like=dl, window=win, return_segments=True)
            say(f"              window {region} px = {win} latent positions: {counts[1]} of {counts[0]} segments, decode {fmt(w)} ms "
                f"against {d[0]:.2f} whole")


say(f"device: {torch.cuda.get_device_name(0)}; {REPS} timed calls each after 2 warm-up calls, median (min .. max), host clock around synchronous calls")
shape(1, 2048, 2048, (4, 16, 64), region=(512, 512, 512, 512))
shape(32, 256, 256, (4,))
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
