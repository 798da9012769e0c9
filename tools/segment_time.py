"""Timings and sizes of segmented streams (container versions 11 - 14) against the unsegmented ones, on in-model symbols.
usage: python tools/segment_time.py [reps] [out.txt] [plain]   (profiles/segmented_stream.md holds a run)

cdc_entropy_encode, cdc_entropy_decode and cdc_entropy_decode_window are synchronous entry points (front end, hyper_dec, the coder's
kernels, the copy back): they are timed with a host clock around the call, on device tensors.  The kernels alone come from a kernel
trace of this script, taken in a run of its own.  `plain`: the unsegmented rows only -- what also runs on a build without segments,
for the comparison against the parent commit; the sha256 printed for them names the bytes."""
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
PLAIN = len(sys.argv) > 3 and sys.argv[3] == "plain"
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


def shape(B, H, W, region=None):
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
    say(f"batch {B} at {H} x {W}: latent {CL} x {4 * hh} x {4 * wh} ({latent[0].size} symbols an image), hyper {CH} x {hh} x {wh}")
    say("    segment   segments   encode ms (min .. max)        decode ms (min .. max)        bytes / image   over plain   bound (8 + 12 n - 264 .. 8 + 276 n)")
    plain_bytes = None
    for segment in (None,) if PLAIN else (None, 512, 256, 128):
        kw = {} if segment is None else {"segment": segment}
        streams = m.latents_to_bytes(dl, dh, **kw)
        n_seg = 1 if segment is None else m.segments_of(streams)[0][1] * m.segments_of(streams)[0][2]
        e = host_timed(lambda: m.latents_to_bytes(dl, dh, **kw))
        d = host_timed(lambda: m.decompress_from_bytes(streams, like=dl))
        size = sum(len(s) for s in streams) / B
        if segment is None:
            plain_bytes = size
            q0 = m.decompress_from_bytes(streams, like=dl)
            say(f"    {'none':>7}   {1:8d}   {e[0]:8.2f} ({e[1]:.2f} .. {e[2]:.2f})   {d[0]:8.2f} ({d[1]:.2f} .. {d[2]:.2f})   {size:13.1f}"
                f"   sha256 of the streams {hashlib.sha256(b''.join(streams)).hexdigest()[:16]}")
            continue
        q = m.decompress_from_bytes(streams, like=dl)
        assert torch.equal(q, q0)
        over = size - plain_bytes
        lo, hi = 8 + 12 * n_seg - 264, 8 + 276 * n_seg
        say(f"    {segment:7d}   {n_seg:8d}   {e[0]:8.2f} ({e[1]:.2f} .. {e[2]:.2f})   {d[0]:8.2f} ({d[1]:.2f} .. {d[2]:.2f})   {size:13.1f}"
            f"   {over:+10.1f}   {lo} .. {hi}  {'inside' if lo <= over <= hi else 'OUTSIDE'}")
        if region is not None:
            cell = m.rate_map_cell
            win = tuple(v // cell for v in region)
            w = host_timed(lambda: m.decompress_from_bytes(streams, like=dl, window=win))
            _, counts = m.decompress_from_bytes(streams, like=dl, window=win, return_segments=True)
            say(f"              window {region} px = {win} latent positions: {counts[1]} of {counts[0]} segments, decode {w[0]:8.2f} ms "
                f"({w[1]:.2f} .. {w[2]:.2f}) against {d[0]:.2f} whole")


say(f"device: {torch.cuda.get_device_name(0)}; {REPS} timed calls each after 2 warm-up calls, median (min .. max), host clock around synchronous calls")
shape(1, 2048, 2048, region=(512, 512, 512, 512))
shape(32, 256, 256)
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
