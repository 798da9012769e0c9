"""What a partial decode costs, on the synthetic model and in-model symbols of tools/hyper_groups_time.py.
usage: python tools/partial_time.py [reps] [out.txt] [base | sampler]      (profiles/partial_decode.md holds a run)

  (a) one 2048 x 2048 image at segment=128, hyper_groups=16: cdc_entropy_decode, and cdc_entropy_decode_partial at full length;
  (b) the same stream cut after 25 / 50 / 75 % of its segments, and whole with one damaged segment;
  (c) a batch of 32 256 x 256 images at segment=128, whole and every image cut after half of its segments;
  (d) `sampler`: decompress(tile=512, region="present") of the 2048 x 2048 stream at a 25 % prefix against the tiled decode of the
      same region of the whole stream, 8 steps, published x-param U-Net with synthetic weights.
`base`: the plain decodes only -- what also runs on a build without the partial entry points, for the comparison against the parent
commit; the sha256 printed names the decoded bits.  The entry points are synchronous: a host clock around the call, device tensors.
The conceal kernel's own time comes from a kernel trace of this script, taken in a run of its own."""
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
from cdc_compression_amd import synth                 # noqa: E402
import rate_ref as R                                  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"
SEGMENT, GROUPS = 128, 16
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
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def fmt(t):
    return f"{t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f})"


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def coder(B, H, W, with_decoder=False):
    """The compressor, its in-model latents on the device, and the streams at segment=128 / hyper_groups=16."""
    m = cdc.ResnetCompressor(dim=64, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=64)
    if with_decoder:
        m.load_state_dict(synth.unet_state_dict(m.manifest(), seed=15))
    dims = tuple(m.reversed_hyper_dims)
    CH, CL = dims[0], dims[-1] // 2
    rng = np.random.default_rng(B * 1000 + H)
    mean_bias = (2.0 * rng.standard_normal(CL)).astype(np.float32)
    m.load_hyper_state_dict({**R.zero_weight_hyper_sd(mean_bias, np.full(CL, 3.0, np.float32), dims=dims), **R.prior_sd(C=CH),
                             "prior._medians": R.medians(CH)})
    hh, wh = H // 64, W // 64
    hyper = (R.medians(CH)[None, :, None, None] + rng.standard_normal((B, CH, hh, wh))).astype(np.float32)
    latent = (mean_bias[None, :, None, None] + 3.0 * rng.standard_normal((B, CL, 4 * hh, 4 * wh))).astype(np.float32)
    dl, dh = torch.from_numpy(latent).cuda(), torch.from_numpy(hyper).cuda()
    return m, dl, m.latents_to_bytes(dl, dh, segment=SEGMENT, hyper_groups=GROUPS)


def entropy(B, H, W, fractions):
    m, dl, streams = coder(B, H, W)
    say(f"batch {B} at {H} x {W}, segment={SEGMENT}, hyper_groups={GROUPS}: {sum(len(s) for s in streams) / B:.0f} bytes an image")
    q = m.decompress_from_bytes(streams, like=dl)
    d = host_timed(lambda: m.decompress_from_bytes(streams, like=dl))
    say(f"    cdc_entropy_decode                         {fmt(d)} ms   sha256 of q_latent {sha(q)}")
    if MODE == "base":
        return
    ends = [m.segment_ends(s) for s in streams]
    S = len(ends[0])
    qp, status = m.decompress_from_bytes(streams, like=dl, partial=True, return_status=True)
    assert torch.equal(qp, q) and not status.any()
    p = host_timed(lambda: m.decompress_from_bytes(streams, like=dl, partial=True, return_status=True))
    say(f"    cdc_entropy_decode_partial, full length    {fmt(p)} ms   sha256 of q_latent {sha(qp)}   {S} of {S} segments an image")
    for f in fractions:
        k = int(S * f)
        cut = [s[: e[k - 1]] for s, e in zip(streams, ends)]
        _, status = m.decompress_from_bytes(cut, like=dl, partial=True, return_status=True)
        assert int((status == 0).sum()) == B * k
        t = host_timed(lambda: m.decompress_from_bytes(cut, like=dl, partial=True, return_status=True))
        say(f"    cdc_entropy_decode_partial, {100 * f:3.0f} % prefix    {fmt(t)} ms   {k} of {S} segments an image, {sum(len(c) for c in cut) / B:.0f} bytes")
    bad = bytearray(streams[0])
    bad[(ends[0][S // 2 - 1] + ends[0][S // 2]) // 2] ^= 0x10          # the middle of segment S / 2
    dam = [bytes(bad)] + list(streams[1:])
    _, status = m.decompress_from_bytes(dam, like=dl, partial=True, return_status=True)
    assert int((status == 2).sum()) == 1 and int((status == 0).sum()) == B * S - 1
    t = host_timed(lambda: m.decompress_from_bytes(dam, like=dl, partial=True, return_status=True))
    say(f"    cdc_entropy_decode_partial, one damaged    {fmt(t)} ms   (seg_conceal_kernel runs: one pair)")


def sampler():
    m, dl, streams = coder(1, 2048, 2048, with_decoder=True)
    un = cdc.Unet(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, m, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    ends = m.segment_ends(streams[0])
    prefix = [streams[0][: ends[len(ends) // 4 - 1]]]
    args = dict(sample_steps=8, seed=1000, gamma=0.8, tile=512, tile_overlap=64)
    a, ia = diff.decompress(prefix, partial=True, region="present", **args)
    b, ib = diff.decompress(streams, region=ia["present_region"], **args)
    same = np.array_equal(a, b)          # (a tile that reaches below the prefix's last row of segments sees the mean there)
    say(f"2048 x 2048 stream, 25 % prefix ({len(prefix[0])} of {len(streams[0])} bytes): present_region {ia['present_region']}, "
        f"{ia['tiles_decoded']} of {ia['tiles']} tiles, {ia['segments_decoded']} of {ia['segments']} segments; the window "
        f"{'equals' if same else 'differs from'} the whole stream's")
    reps = max(2, REPS // 3)
    tp = host_timed(lambda: diff.decompress(prefix, partial=True, region="present", **args), reps, 1)
    tw = host_timed(lambda: diff.decompress(streams, region=ia["present_region"], **args), reps, 1)
    say(f"    decompress(prefix, partial=True, tile=512, region=\"present\"), 8 steps   {fmt(tp)} ms")
    say(f"    decompress(whole stream, tile=512, region=that tuple), 8 steps           {fmt(tw)} ms")


say(f"device: {torch.cuda.get_device_name(0)}; {REPS} timed calls each after 2 warm-up calls, median (min .. max), host clock around synchronous calls")
if MODE == "sampler":
    sampler()
else:
    entropy(1, 2048, 2048, (0.25, 0.5, 0.75))
    entropy(32, 256, 256, (0.5,))
if OUT:
    open(OUT, "w").write("\n".join(lines) + "\n")
