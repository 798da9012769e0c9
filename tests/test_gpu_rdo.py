"""Rate-distortion optimised quantisation on the GPU: cdc_op_rdo_quantize against the float64 decision of tests/rdo_ref.py on hand-made
operands, cdc_entropy_rate_sweep against the coder itself (an encode with cdc_set_rdo, decoded) and against float64 sums, and the Python
surface: compress_to_bytes(rdo= / target_bpp= / max_bytes=), encode / forward(rdo=), GaussianDiffusion.compress_to_bytes(target_bpp=).

The model is the small four-level BigCompressor of tests/golden/manifest_vbr_small.json without its VBR sites (frame multiple 64, 32
latent channels: a 64 x 64 image has 512 latent symbols, a 128 x 192 one 3072, two workgroups of the sweep).  tests/test_rdo_host.py
asserts on the CPU what the op-level cases rest on: the band and the share of undecided symbols."""
import functools
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
import metrics_ref as M
import rate_ref as RR
import rdo_ref as R
from cdc_compression_amd import _lib, compressor as C, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _model():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_small.json")))
    sd = synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"])
    sd = {k: v for k, v in sd.items() if not synth.is_vbr_key(k)}
    comp = cdc.BigCompressor(vbr=False, **meta["kwargs"])
    comp.load_state_dict(sd)
    assert comp.frame_multiple == 64
    return comp, {k: v for k, v in sd.items() if k.startswith("prior.affine.") or k.startswith("prior.a.")}


@functools.lru_cache(maxsize=None)
def _images(B, H, W):
    img = (2.0 * M.noisy(M.picture(B, H, W, seed=3), 0.08, 5) - 1.0).astype(np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _analysed(B, H, W):
    """(latent, hyper) of the batch, and per image what the coder codes with: the plain streams, their decoded symbols, and mean / scale
    of hyper_decode at batch 1 (the coder's plan)."""
    comp, _ = _model()
    latent, hyper = comp.analysis(_images(B, H, W))
    streams = comp.latents_to_bytes(latent, hyper)
    q0, qh = comp.decompress_from_bytes(streams, return_hyper=True)
    ms = [comp.hyper_decode(qh[b:b + 1]) for b in range(B)]
    mean, scale = np.concatenate([a for a, _ in ms]), np.concatenate([b for _, b in ms])
    for a in (latent, hyper, q0, qh, mean, scale):
        a.setflags(write=False)
    return latent, hyper, tuple(streams), q0, qh, mean, scale


# ---- op level ---------------------------------------------------------------------------------------------------------------------------

def _check_op(per_image, q, moved, y, m, s):
    band, worst = R.method_band(y, m, s, R.MUS)
    t = R.terms64(y, m, s)
    und_total = 0
    for b, mu in enumerate(R.MUS):
        tb = {k: v[b] for k, v in t.items()}
        is0, is1 = _bits32(q[b]) == _bits32(tb["x0"]), _bits32(q[b]) == _bits32(tb["x1"])
        assert np.all(is0 | is1), (per_image, b)                         # every output symbol is k0 or k1
        took1 = ~is0
        if mu == 0:
            assert not took1.any()
        assert not np.any(took1 & (tb["k0"] == 0))
        assert np.all(np.abs(q[b].astype(np.float64) - y[b].astype(np.float64)) <= 1.5 + np.spacing(np.abs(y[b]).astype(np.float32)))
        assert moved[b] == int(took1.sum()), (per_image, b, moved[b], int(took1.sum()))
        want = R.decide64(tb, mu)
        und = R.undecided(tb, mu, band)
        und_total += int(und.sum())
        wrong = (took1 != want) & ~und
        off = np.abs(R.margin64(tb, mu))[took1 != want]
        print(f"[rdo] per_image {per_image} mu {mu}: moved {moved[b]}, undecided {int(und.sum())}, differing from float64 {int((took1 != want).sum())}"
              f" (largest float64 margin among them {off.max() if off.size else 0.0:.3g}), band {band:.3g} = 10 x {worst:.3g}")
        assert not wrong.any(), (per_image, b, np.nonzero(wrong)[0][:5])
    assert und_total <= R.UNDECIDED_CAP * 3 * per_image


@pytest.mark.parametrize("per_image", R.PER_IMAGE)
def test_op_against_the_float64_decision(per_image):
    """cdc_op_rdo_quantize, B = 3 with mu = (0, 0.5, 8), from host and from device memory (the same bits).

    The band is 10 x the float32 method's own loss, measured on the CPU over the case's inputs (1.8e-2 with the scale point 2048 in,
    1.3e-5 for per_image = 1).  Measured on an MI355X (profiles/rdo_quant.md; every run prints the figures): of the 4 044 symbols of the
    four cases none is decided otherwise than in float64, inside the band or outside it, so 4 x the device's own difference does not
    exceed the CPU-side band and that one stays."""
    comp, _ = _model()
    y, m, s = R.op_case(per_image)
    q, moved = comp.rdo_quantize(y, m, s, R.MUS)
    assert q.shape == y.shape and q.dtype == np.float32 and moved.dtype == np.int64 and moved.shape == (3,)
    _check_op(per_image, q, moved, y, m, s)
    qd, moved_d = comp.rdo_quantize(_dev(y), _dev(m), _dev(s), R.MUS)
    assert np.array_equal(_bits32(qd.cpu().numpy()), _bits32(q)) and np.array_equal(moved_d, moved)
    one, moved_1 = comp.rdo_quantize(y[2:3], m[2:3], s[2:3], R.MUS[2])           # a scalar mu, batch 1: image 2's row
    assert np.array_equal(_bits32(one[0]), _bits32(q[2])) and moved_1[0] == moved[2]


def test_op_off_the_float4_alignment():
    """Operands whose base is not 16-byte aligned take the scalar path for every element and give the same symbols."""
    import torch
    comp, _ = _model()
    y, m, s = R.op_case(257)
    q, moved = comp.rdo_quantize(y, m, s, R.MUS)
    pad = [torch.zeros(3 * 257 + 1, dtype=torch.float32, device="cuda") for _ in range(3)]
    views = []
    for p, a in zip(pad, (y, m, s)):
        v = p[1:].view(3, 257)
        v.copy_(torch.from_numpy(np.array(a)))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    q2, moved2 = comp.rdo_quantize(*views, R.MUS)
    assert np.array_equal(_bits32(q2.cpu().numpy()), _bits32(q)) and np.array_equal(moved2, moved)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_op_refuses_non_finite_operands_with_nothing_written(bad):
    comp, _ = _model()
    L, h = _lib.lib(), comp._hyper_handle()
    y, m, s = (np.array(a) for a in R.op_case(63))
    for which in range(3):
        ops = [y.copy(), m.copy(), s.copy()]
        ops[which][1, 40] = bad
        q = np.full(y.shape, -77.0, np.float32)
        moved = np.full(3, -5, np.int64)
        rc = L.cdc_op_rdo_quantize(h, ops[0].ctypes.data, ops[1].ctypes.data, ops[2].ctypes.data, R.MUS.ctypes.data, q.ctypes.data,
                                   moved.ctypes.data, 3, 63, 0, None)
        assert rc == -1 and b"nothing written" in L.cdc_last_error(h), (which, rc)
        assert np.all(q == -77.0) and np.all(moved == -5)
        with pytest.raises(_lib.CdcError):
            comp.rdo_quantize(*ops, R.MUS)
    mu_bad = np.array([0.0, bad, 1.0], np.float32)
    assert L.cdc_op_rdo_quantize(h, y.ctypes.data, m.ctypes.data, s.ctypes.data, mu_bad.ctypes.data, q.ctypes.data, None, 3, 63, 0, None) == -1
    good, _ = comp.rdo_quantize(y, m, s, R.MUS)                          # the handle still works
    assert np.all(np.isfinite(good))


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------

LADDERS = {1: np.zeros(1, np.float32),
           5: np.array([0.0, 0.25, 1.0, 4.0, 64.0], np.float32),
           18: np.concatenate([np.zeros(1, np.float32), C.RDO_LADDER]),              # what compress_to_bytes(target_bpp=) sweeps
           32: np.concatenate([np.zeros(1, np.float32), np.geomspace(2.0 ** -8, 2.0 ** 8, 31).astype(np.float32)])}


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 64, 64), (1, 128, 192), (3, 128, 192)])
@pytest.mark.parametrize("L", [1, 5, 18, 32])
def test_sweep_against_the_coder_and_float64(B, H, W, L):
    comp, psd = _model()
    latent, hyper, streams0, q0, qh, mean, scale = _analysed(B, H, W)
    mus = LADDERS[L]
    t = comp._sweep(latent, hyper, mus)
    bits, sse, moved = t["bits"], t["sse"], t["moved"]
    assert bits.shape == sse.shape == moved.shape == (B, L) and moved.dtype == np.int64
    # the column mu = 0: cdc_bpp * H * W of today's symbols to float32 rounding, nothing moved, the float64 squared error
    plain = comp.rate(qh, q0, mean, scale, (H, W)).astype(np.float64) * (H * W)
    assert np.all(np.abs(bits[:, 0] - plain) <= 4.0 * np.spacing(plain.astype(np.float32))), (bits[:, 0], plain)
    assert not moved[:, 0].any()
    sse0 = ((latent.astype(np.float64) - q0.astype(np.float64)) ** 2).reshape(B, -1).sum(1)
    assert np.allclose(sse[:, 0], sse0, rtol=1e-12, atol=0)
    # monotone along the ladder, exactly
    assert np.all(np.diff(bits, axis=1) <= 0) and np.all(np.diff(moved, axis=1) >= 0) and np.all(np.diff(sse, axis=1) >= 0)
    # every entry against an encode at that mu, decoded: the same count, and the float64 price of those symbols
    for j, mu in enumerate(mus):
        qj = q0 if mu == 0 else comp.decompress_from_bytes(comp.latents_to_bytes(latent, hyper, rdo=float(mu)))
        changed = (_bits32(qj) != _bits32(q0)).reshape(B, -1).sum(1)
        assert np.array_equal(changed, moved[:, j]), (j, mu, changed, moved[:, j])
        h64, c64 = RR.rate_terms_f64(psd, qh, qj, mean, scale)
        h32, c32 = RR.rate_terms_f32(psd, qh, qj, mean, scale)
        for b in range(B):
            ref = float(h64[b].sum() + c64[b].sum())
            own = float(np.abs(h32[b] - h64[b]).sum() + np.abs(c32[b] - c64[b]).sum())
            tol = 8.0 * own + 8.0 * float(np.spacing(np.float32(ref)))
            assert abs(bits[b, j] - ref) <= tol, (b, j, bits[b, j], ref, tol)
            sse_j = float(((latent[b].astype(np.float64) - qj[b].astype(np.float64)) ** 2).sum())
            assert np.isclose(sse[b, j], sse_j, rtol=1e-12, atol=0)
    print(f"[rdo] sweep {B} x {H} x {W}, L = {L}: bits {bits[0, 0]:.1f} -> {bits[0, -1]:.1f}, moved {moved[0, -1]} of {latent[0].size}")
    # the same bits again, and the rows of batch-1 calls
    again = comp._sweep(latent, hyper, mus)
    assert all(np.array_equal(again[k].view(np.int64), t[k].view(np.int64)) for k in t)
    if B > 1:
        for b in range(B):
            one = comp._sweep(latent[b:b + 1], hyper[b:b + 1], mus)
            assert all(np.array_equal(one[k][0].view(np.int64), t[k][b].view(np.int64)) for k in t), b
        dev = comp._sweep(_dev(latent), _dev(hyper), mus)
        assert all(np.array_equal(dev[k].view(np.int64), t[k].view(np.int64)) for k in t)


def test_sweep_refusals():
    comp, _ = _model()
    L, h = _lib.lib(), comp._hyper_handle()
    latent, hyper = _analysed(1, 64, 64)[:2]
    med = comp._median_vector()
    out = [np.zeros(40, np.float64), np.zeros(40, np.float64), np.zeros(40, np.int64)]

    def call(mu, n, lat=latent):
        return L.cdc_entropy_rate_sweep(h, lat.ctypes.data, hyper.ctypes.data, med.ctypes.data, 1, 1, 1, mu.ctypes.data, n,
                                        *[o.ctypes.data for o in out], 0, None)
    ok = np.ones(40, np.float32)
    assert call(ok, 0) == -1 and call(ok, 33) == -1 and call(ok, 32) == 0 and call(ok, 1) == 0
    for bad in (-1.0, np.nan, np.inf):
        mu = ok.copy()
        mu[2] = bad
        assert call(mu, 5) == -1 and call(mu, 2) == 0
    lat = np.array(latent)
    lat[0, 3, 1, 1] = np.nan
    assert call(ok, 3, lat) == -1 and b"non-finite" in L.cdc_last_error(h)
    assert call(ok, 3) == 0


# ---- streams --------------------------------------------------------------------------------------------------------------------------------

MU3 = [0.0, 0.5, 8.0]


def test_rdo_unset_and_rdo_0_give_the_plain_bytes():
    comp, _ = _model()
    images = _images(3, 128, 192)
    plain = comp.compress_to_bytes(images)
    assert comp.compress_to_bytes(images, rdo=0.0) == plain
    assert comp.compress_to_bytes(images, rdo=[0.0, 0.0, 0.0]) == plain
    assert comp.compress_to_bytes(images, rdo=8.0) != plain
    assert comp.compress_to_bytes(images) == plain                      # the handle keeps nothing of the call before
    latent, hyper, streams0 = _analysed(3, 128, 192)[:3]
    assert list(streams0) == plain
    L, h = _lib.lib(), comp._hyper_handle()
    two = np.array([1.0, 2.0], np.float32)                              # a later call with n neither 1 nor B fails, as the VBR rule does
    assert L.cdc_set_rdo(h, two.ctypes.data, 2) == 0
    with pytest.raises(_lib.CdcError, match="1 or 3 expected"):
        comp.latents_to_bytes(latent, hyper)
    assert L.cdc_set_rdo(h, None, 0) == 0 and comp.latents_to_bytes(latent, hyper) == plain


def test_streams_with_one_mu_per_image():
    comp, _ = _model()
    latent, hyper, streams0, q0, qh, mean, scale = _analysed(3, 128, 192)
    streams = comp.latents_to_bytes(latent, hyper, rdo=MU3)
    q, qh2 = comp.decompress_from_bytes(streams, return_hyper=True)      # every stream decodes
    assert np.array_equal(_bits32(qh2), _bits32(qh))
    for b, mu in enumerate(MU3):
        one = comp.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], rdo=mu)
        assert one[0] == streams[b], b                                    # row b = the batch-1 stream with mu_b, byte for byte
    assert streams[0] == streams0[0]
    # the same through compress_to_bytes, with the report: mu as given, the counts and the estimate of the symbols coded
    s5, i5 = comp.compress_to_bytes(_images(3, 128, 192), rdo=MU3, return_info=True)
    assert s5 == streams and i5["mu"].tolist() == MU3 and i5["met"].all() and i5["reencodes"] == 0
    assert np.array_equal(i5["moved"], (_bits32(q) != _bits32(q0)).reshape(3, -1).sum(1)) and i5["moved"][0] == 0 < i5["moved"][2]
    got = _rate_of(comp, streams, (128, 192))
    assert np.all(np.abs(got.astype(np.float64) - i5["estimated_bpp"]) <= 4.0 * np.spacing(got))
    assert np.allclose(i5["latent_mse"], ((latent.astype(np.float64) - q.astype(np.float64)) ** 2).reshape(3, -1).mean(1), rtol=1e-12)
    _, i6 = comp.compress_to_bytes(_images(3, 128, 192), return_info=True)
    assert not i6["mu"].any() and not i6["moved"].any() and np.array_equal(i6["estimated_bpp"][:1], i5["estimated_bpp"][:1])
    # one image along mu: lengths do not increase, the symbols differ from the mu = 0 ones by at most one step towards the mean
    lengths = []
    for mu in (0.0, 0.25, 0.5, 2.0, 8.0, 64.0):
        s = comp.latents_to_bytes(latent[1:2], hyper[1:2], rdo=mu)
        qm = comp.decompress_from_bytes(s)
        k0 = np.rint(q0[1:2].astype(np.float64) - mean[1:2])
        km = np.rint(qm.astype(np.float64) - mean[1:2])
        step = km - k0
        assert np.all((step == 0) | ((step == -np.sign(k0)) & (k0 != 0))), mu
        lengths.append(len(s[0]))
    print("[rdo] stream bytes along mu = 0, 0.25, 0.5, 2, 8, 64:", lengths)
    assert lengths == sorted(lengths, reverse=True) and lengths[-1] < lengths[0]


def _rate_of(comp, streams, hw):
    q, qh = comp.decompress_from_bytes(streams, return_hyper=True)
    out = []
    for b in range(len(streams)):
        mean, scale = comp.hyper_decode(qh[b:b + 1])
        out.append(comp.rate(qh[b:b + 1], q[b:b + 1], mean, scale, hw)[0])
    return np.array(out, np.float32)


def test_target_bpp():
    comp, _ = _model()
    H, W = 128, 192
    images = _images(3, H, W)
    plain = comp.compress_to_bytes(images)
    ladder = LADDERS[18]
    curve = comp.rate_sweep(images, ladder)
    assert sorted(curve) == ["bpp", "latent_mse", "moved", "mu"] and curve["bpp"].shape == (3, 18)
    bpp = curve["bpp"]
    # per image a target between its bpp at two ladder entries (the last strict drop of its curve)
    js = [int(np.nonzero(np.diff(bpp[b]) < 0)[0][-1]) + 1 for b in range(3)]
    target = np.array([0.5 * (bpp[b, j] + bpp[b, j - 1]) for b, j in enumerate(js)])
    streams, info = comp.compress_to_bytes(images, target_bpp=target, return_info=True)
    assert sorted(info) == ["estimated_bpp", "latent_mse", "met", "moved", "mu", "reencodes"] and info["reencodes"] == 0
    assert info["met"].all() and np.all(info["estimated_bpp"] <= target)
    got = _rate_of(comp, streams, (H, W))
    assert np.all(np.abs(got.astype(np.float64) - info["estimated_bpp"]) <= 4.0 * np.spacing(got)), (got, info["estimated_bpp"])
    for b, j in enumerate(js):
        lo, hi = ladder[j - 1], ladder[j]
        assert lo < info["mu"][b] <= hi
        fine = C.rdo_refine_ladder(lo, hi)
        k = int(np.nonzero(fine == info["mu"][b])[0][0])
        below = comp.rate_sweep(images[b:b + 1], fine[k - 1:k + 1])["bpp"][0]
        assert below[0] > target[b] >= below[1], (b, below, target[b])     # the ladder entry below the chosen mu exceeds the target
        assert len(streams[b]) <= len(plain[b])
    print(f"[rdo] target_bpp {target} -> mu {info['mu']}, estimated {info['estimated_bpp']}, moved {info['moved']}")
    # a target above the plain bpp: mu = 0 and the plain bytes
    s2, i2 = comp.compress_to_bytes(images, target_bpp=float(bpp[:, 0].max()) * 1.01, return_info=True)
    assert s2 == plain and not i2["mu"].any() and i2["met"].all() and not i2["moved"].any()
    # a target below the last ladder entry: met = False, the largest mu, a valid stream
    s3, i3 = comp.compress_to_bytes(images, target_bpp=float(bpp[:, -1].min()) * 0.5, return_info=True)
    assert not i3["met"].any() and np.all(i3["mu"] == ladder[-1])
    assert np.array_equal(_rate_of(comp, s3, (H, W)) <= _rate_of(comp, plain, (H, W)), np.ones(3, bool))
    # one scalar target for the batch, mixed: image by image as its own batch-1 call
    mid = float(np.sort(target)[1])
    s4, i4 = comp.compress_to_bytes(images, target_bpp=mid, return_info=True)
    for b in range(3):
        s1, i1 = comp.compress_to_bytes(images[b:b + 1], target_bpp=mid, return_info=True)
        assert i1["mu"][0] == i4["mu"][b]


def test_max_bytes():
    comp, _ = _model()
    images = _images(3, 128, 192)
    plain = comp.compress_to_bytes(images)
    budget = [int(0.9 * len(s)) for s in plain]
    streams, info = comp.compress_to_bytes(images, max_bytes=budget, return_info=True)
    comp.decompress_from_bytes(streams)
    print(f"[rdo] max_bytes {budget}: {[len(s) for s in streams]} bytes (plain {[len(s) for s in plain]}), mu {info['mu']}, met {info['met']}, "
          f"re-encodes {info['reencodes']}")
    for b in range(3):
        assert info["met"][b] == (len(streams[b]) <= budget[b])
    assert info["met"].all() or info["reencodes"] == 3
    assert 0 <= info["reencodes"] <= 3
    # (the first choice rests on the ESTIMATE, which may price an image above what the coder then writes -- on this synthetic model by a
    # fifth: a budget the plain stream only just meets can still get a mu > 0; one with that margin gets mu = 0 and the plain bytes)
    roomy, i2 = comp.compress_to_bytes(images, max_bytes=[2 * len(s) for s in plain], return_info=True)
    assert roomy == plain and i2["met"].all() and i2["reencodes"] == 0 and not i2["mu"].any()


def test_encode_and_forward_with_rdo():
    comp, _ = _model()
    H, W = 70, 100
    images = M.as_u8(M.picture(3, H, W))
    plain = comp.forward(images)
    again = comp.forward(images, rdo=None)
    for k in ("bpp", "q_latent", "q_hyper_latent"):
        assert np.array_equal(_bits32(plain[k]), _bits32(again[k]))
    assert all(np.array_equal(_bits32(a), _bits32(b)) for a, b in zip(plain["output"], again["output"]))
    q, qh, st = comp.encode(images, rdo=MU3)
    assert sorted(st) == ["hyper_latent", "latent", "latent_distribution", "q_latent", "rdo_moved"]
    dist = st["latent_distribution"]
    assert np.array_equal(_bits32(q[0]), _bits32(plain["q_latent"][0])) and st["rdo_moved"][0] == 0 and st["rdo_moved"][2] > 0
    assert np.array_equal(_bits32(comp.dequantize(st["latent"], dist.mean)), _bits32(plain["q_latent"]))     # state4bpp keeps the unquantised latent
    changed = (_bits32(q) != _bits32(plain["q_latent"])).reshape(3, -1).sum(1)
    assert np.array_equal(changed, st["rdo_moved"])
    out = comp.forward(images, rdo=MU3)
    assert np.array_equal(_bits32(out["q_latent"]), _bits32(q))
    assert np.array_equal(_bits32(out["bpp"]), _bits32(comp.rate(qh, q, dist.mean, dist.scale, (H, W))))
    assert np.array_equal(_bits32(out["bpp"]), _bits32(comp.bpp((3, 3, H, W), st)))
    assert out["bpp"][0] == plain["bpp"][0] and out["bpp"][2] < plain["bpp"][2]
    ctx = comp.decode(q)
    assert all(np.array_equal(_bits32(a), _bits32(b)) for a, b in zip(out["output"], ctx))                   # the pyramid comes from that q_latent
    rm = comp.forward(images, rdo=MU3, return_rate_map=True)["rate_map"]
    assert np.array_equal(_bits32(rm), _bits32(comp.rate_map(qh, q, dist.mean, dist.scale)["cell"]))


def test_diffusion_compress_to_bytes_with_a_target_and_decompress():
    """The feature reaches the public surface: GaussianDiffusion.compress_to_bytes(target_bpp=) then decompress gives an image of the
    right size (no quality claim), and compress(rdo=) reports the bpp of the symbols chosen."""
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))["x"]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0))
    comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
    comp.load_state_dict(synth.unet_state_dict([(k, tuple(v)) for k, v in meta["comp_manifest"]], seed=meta["seed"]))
    diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    images = M.as_u8(M.picture(2, 70, 100))
    plain = diff.compress_to_bytes(images)
    base = comp.rate_sweep(images, [0.0, 256.0])["bpp"]
    target = 0.5 * (base[:, 0] + base[:, 1])
    streams, info = diff.compress_to_bytes(images, target_bpp=target, return_info=True)
    assert len(streams) == 2 and np.all(info["estimated_bpp"] <= target)
    assert np.array_equal(info["met"], base[:, 1] <= target)
    rec = diff.decompress(streams, sample_steps=2, seed=1, gamma=0.8)
    assert tuple(rec.shape) == (2, 3, 70, 100) and np.all(np.isfinite(np.asarray(rec)))
    assert diff.compress_to_bytes(images, rdo=0.0) == plain
    rec2, bpp2 = diff.compress(images, sample_steps=2, bpp_return_mean=False, seed=1, gamma=0.8, rdo=256.0)
    rec0, bpp0 = diff.compress(images, sample_steps=2, bpp_return_mean=False, seed=1, gamma=0.8)
    assert tuple(rec2.shape) == (2, 3, 70, 100) and np.all(np.asarray(bpp2) <= np.asarray(bpp0))
    assert np.allclose(np.asarray(bpp2, np.float64), base[:, 1], rtol=1e-6)
