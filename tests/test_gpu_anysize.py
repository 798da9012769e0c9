"""Images of any size on the GPU: the frame kernels bit for bit against torch on the CPU, and every fixture of
tests/golden/make_golden_anysize.py -- the real reference on the replicate-padded image with the zero-extended init, cropped, bpp
over H * W -- through the public Python surface.

Bounds are the project's own for the same model and step count, not new ones:
  bpp            1e-5 relative             (test_kodak_crops_500_steps_match_reference)
  symbols        _symbols_close, copied    (its cap of max(1, 1e-4 n) flips is a condition: the generator refuses images on which
                                            the reference flips a symbol against itself in float64)
  decode         TOL_DEC = 5e-5 relative for the few-step runs (test_decode_matches_reference_golden); 3e-5 absolute on the
                 sampled pixels and 1e-5 per pixel on the sum for the 65-step run (the Kodak test's bounds)
The decode half is fed the FIXTURE's q_latent, so an encoder flip cannot pass for decoder error.  When the GPU encoder does flip a
symbol against the reference the bpp comparison of that image is skipped and reported; more than one such image fails
(test_at_most_one_image_flipped_a_symbol, which runs last in this file)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, frame, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL_DEC = 5e-5
WIDTHS = [1, 3, 4, 5, 63, 64, 65, 333]
FLIPPED = []          # (fixture, image) whose GPU q_latent differs from the reference's by a flipped symbol


def relerr(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _symbols_close(a, ref, max_flip_frac=1e-4):
    """tests/test_gpu_parity.py::_symbols_close; returns the number of flipped symbols."""
    d = np.abs(a - ref)
    near = d <= 1.5e-5 * max(1.0, float(np.abs(ref).max()))
    flip = np.abs(d - 1.0) <= 1e-3
    assert (near | flip).all()
    assert flip.sum() <= max(1, int(max_flip_frac * flip.size)), (int(flip.sum()), flip.size)
    return int(flip.sum())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the two kernels against torch on the CPU, bit for bit --------------------------------------------------------------------------

def _handle():
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    return un, un._handle()


def _boundary_values():
    """Floats whose uint8 image sits exactly on a rounding boundary ((x / 2 + .5) * 255 + .5 an integer), their neighbours, values
    outside [-1, 1] and on its ends."""
    k = np.arange(0, 257, dtype=np.float64)
    base = (2.0 * ((k - 0.5) / 255.0) - 1.0).astype(np.float32)
    v = [base]
    for _ in range(3):
        v.append(np.nextafter(v[-1], np.float32(2)))
    lo = base
    for _ in range(3):
        lo = np.nextafter(lo, np.float32(-2))
        v.append(lo)
    v.append(np.array([-1.0, 1.0, -1.5, 1.5, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45, 0.5, -0.5, 0.99999994, -0.99999994], np.float32))
    return np.concatenate(v).astype(np.float32)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("W", WIDTHS)
def test_frame_kernels_match_torch_bit_for_bit(W, where):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    keep, h = _handle()
    B, H = 2, 5
    rng = np.random.default_rng(W)
    to = (lambda a: torch.from_numpy(a).cuda()) if where == "device" else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if where == "device" else (lambda a: a)
    for Hp, Wp in ((H, W), (8, -(-W // 64) * 64), (H + 59, -(-W // 64) * 64 + 64), (7, W + 3)):
        f32 = (rng.standard_normal((B, 3, H, W)) * 0.8).astype(np.float32)
        f32.reshape(-1)[: min(f32.size, 4)] = np.array([np.inf, -0.0, 1e-45, -3e38], np.float32)[: min(f32.size, 4)]
        u8 = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
        u8.reshape(-1)[: min(u8.size, 256)] = np.arange(256, dtype=np.uint8)[: min(u8.size, 256)]
        pad = (0, Wp - W, 0, Hp - H)
        # frame-in: float copy with edge replication, zero fill, uint8 -> float
        want = F.pad(torch.from_numpy(f32), pad, mode="replicate").numpy()
        got = back(frame.pad(h, to(f32), Hp, Wp, 0))
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), ("f32 edge", W, Hp, Wp)
        want = F.pad(torch.from_numpy(f32), pad, value=0.0).numpy()
        got = back(frame.pad(h, to(f32), Hp, Wp, 0, zero=True))
        assert np.array_equal(_bits(got), _bits(want)), ("f32 zero", W, Hp, Wp)
        want = F.pad(torch.from_numpy(u8).float() / 255.0 * 2.0 - 1.0, pad, mode="replicate").numpy()
        got = back(frame.pad(h, to(u8), Hp, Wp, 0))
        assert np.array_equal(_bits(got), _bits(want)), ("u8 edge", W, Hp, Wp)
        # frame-out: the window as float, and as the uint8 the reference script saves
        fr = (rng.standard_normal((B, 3, Hp, Wp)) * 0.8).astype(np.float32)
        bv = _boundary_values()
        n = min(fr.size, bv.size)
        fr.reshape(-1)[:n] = bv[:n]
        m = min(H * W, bv.size)
        idx = np.unravel_index(np.arange(m), (H, W))
        fr[0, 1, idx[0], idx[1]] = bv[rng.permutation(bv.size)[:m]]       # boundary values inside the window too
        got = back(frame.crop(h, to(fr), H, W, 0))
        assert got.shape == (B, 3, H, W) and np.array_equal(_bits(got), _bits(fr[:, :, :H, :W])), ("crop f32", W, Hp, Wp)
        t = torch.from_numpy(fr[:, :, :H, :W].copy())
        want = ((t.clamp(-1, 1) / 2.0 + 0.5).mul(255).add_(0.5).clamp_(0, 255)).to(torch.uint8).numpy()
        got = back(frame.crop(h, to(fr), H, W, 0, as_uint8=True))
        assert got.dtype == np.uint8 and np.array_equal(got, want), ("crop u8", W, Hp, Wp, int((got != want).sum()))
    del keep


@pytest.mark.parametrize("H,W", [(37, 50), (40, 48)])      # W % 4 != 0: the element path; W % 4 == 0: the 16-byte path
def test_frame_entry_points_give_the_same_bits_from_host_and_device_memory(H, W):
    """The host-staging path of cdc_frame_pad / cdc_frame_crop (operands copied through call scratch) against device operands."""
    torch = pytest.importorskip("torch")
    keep, h = _handle()
    rng = np.random.default_rng(H * 100 + W)
    f32 = (rng.standard_normal((2, 3, H, W)) * 0.8).astype(np.float32)
    u8 = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    fr = (rng.standard_normal((2, 3, 64, 64)) * 0.8).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    for img in (f32, u8):
        for zero in (False, True):
            host = frame.pad(h, img, 64, 64, 0, zero=zero)
            assert host.shape == (2, 3, 64, 64) and np.array_equal(_bits(host), _bits(frame.pad(h, dev(img), 64, 64, 0, zero=zero).cpu().numpy()))
        assert np.array_equal(_bits(host[:, :, :H, :W]), _bits(f32 if img is f32 else (img.astype(np.float32) / 255.0 * 2.0 - 1.0).astype(np.float32)))
    host = frame.crop(h, fr, H, W, 0)
    assert np.array_equal(_bits(host), _bits(fr[:, :, :H, :W])) and np.array_equal(_bits(host), _bits(frame.crop(h, dev(fr), H, W, 0).cpu().numpy()))
    host = frame.crop(h, fr, H, W, 0, as_uint8=True)
    assert host.dtype == np.uint8 and np.array_equal(host, frame.crop(h, dev(fr), H, W, 0, as_uint8=True).cpu().numpy())
    del keep


def test_frame_entry_points_refuse_bad_sizes():
    keep, h = _handle()
    L = _lib.lib()
    a = np.zeros((1, 3, 8, 8), np.float32)
    o = np.zeros((1, 3, 8, 8), np.float32)
    for B, H, W, Hp, Wp in ((1, 8, 8, 7, 8), (1, 8, 8, 8, 7), (0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, -1, 8, 8)):
        assert L.cdc_frame_pad(h, a.ctypes.data, o.ctypes.data, B, H, W, Hp, Wp, 0, 0, 0, None) == -1
        assert L.cdc_frame_crop(h, a.ctypes.data, o.ctypes.data, B, H, W, Hp, Wp, 0, 0, None) == -1
    assert L.cdc_frame_pad(h, a.ctypes.data, o.ctypes.data, 1, 8, 8, 8, 8, 2, 0, 0, None) == -1       # element kind
    assert L.cdc_frame_pad(h, a.ctypes.data, o.ctypes.data, 1, 8, 8, 8, 8, 0, 2, 0, None) == -1       # fill mode
    assert L.cdc_frame_pad(h, None, o.ctypes.data, 1, 8, 8, 8, 8, 0, 0, 0, None) == -1
    del keep


# ---- the fixtures end to end -------------------------------------------------------------------------------------------------------

def _images():
    return np.load(os.path.join(GOLDEN, "anysize_images.npz"))


def _full_x():
    un_meta = json.load(open(os.path.join(GOLDEN, "manifest_full_x.json")))
    kw = dict(un_meta["unet_kwargs"])
    un = cdc.Unet(**kw)
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in un_meta["manifest"]], seed=0))
    meta = json.load(open(os.path.join(GOLDEN, "manifest_encoder_full_x.json")))
    comp = cdc.ResnetCompressor(**meta["kwargs"])
    comp.load_state_dict(synth.unet_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=15))
    return cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine"), un, comp


def _small(tag):
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))[tag]
    kw = dict(meta["unet_kwargs"])
    un = cdc.Unet(**kw)
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0 if tag == "x" else 0.2))
    man = [(k, tuple(v)) for k, v in meta["comp_manifest"]]
    if tag == "x":
        comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
        comp.load_state_dict(synth.unet_state_dict(man, seed=meta["seed"]))
        diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    else:
        comp = cdc.BigCompressor(**meta["comp_kwargs"])
        comp.load_state_dict((synth.compressor_state_dict if tag == "vbr" else synth.unet_state_dict)(man, seed=meta["seed"]))
        diff = cdc.GaussianDiffusionEps(un, comp, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear", vbr=tag == "vbr")
    return diff, un, comp, (np.array(meta["rates"], np.float32) if meta.get("rates") else None)


def _check_case(diff, un, comp, g, tag, u8, steps_list, full, rates=None, long_run=(), **ckw):
    """One fixture case through compress(), the compressor's forward(), decompress() of the fixture's q_latent and the byte streams."""
    B, _, H, W = u8.shape
    Hp, Wp = (int(v) for v in g[f"{tag}_padded_hw"])
    assert (H, W) == tuple(int(v) for v in g[f"{tag}_hw"])
    assert diff.padded_size(H, W) == (Hp, Wp) and comp.padded_size(H, W) == (Hp, Wp)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    ekw = {} if rates is None else {"bitrate_scale": rates}
    fkw = () if rates is None else (rates,)
    # encoder: symbols of the padded frame, bpp over H * W
    out = comp(u8, *fkw)
    assert out["output"][0].shape[-2:] == (Hp, Wp) and out["bpp"].shape == (B,)
    nflip = _symbols_close(out["q_latent"], g[f"{tag}_q_latent"])
    print(f"[anysize] {tag}: flipped symbols {nflip} of {out['q_latent'].size}; bpp {out['bpp']} reference {g[f'{tag}_bpp']} "
          f"rel {np.abs(out['bpp'] - g[f'{tag}_bpp']).max() / np.abs(g[f'{tag}_bpp']).max():.3e}")
    if nflip:
        FLIPPED.append(tag)
    else:
        assert np.abs(out["bpp"] - g[f"{tag}_bpp"]).max() <= 1e-5 * float(np.abs(g[f"{tag}_bpp"]).max()), (out["bpp"], g[f"{tag}_bpp"])
    x = (u8.astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    out_f = comp(x, *fkw)                                      # the float image gives the same symbols as the uint8 one
    np.testing.assert_array_equal(out_f["q_latent"], out["q_latent"])
    np.testing.assert_array_equal(out_f["bpp"], out["bpp"])
    for steps in steps_list:
        # decode half alone, from the fixture's q_latent
        ctx = comp.decode(g[f"{tag}_q_latent"], *fkw)
        rec = diff.decompress(ctx, (B, 3, H, W), sample_steps=steps, init=init)
        assert rec.shape == (B, 3, H, W)
        if full:
            e = relerr(rec, g[f"{tag}_rec{steps}"])
            print(f"[anysize] {tag}: {steps}-step decode relerr {e:.3e}")
            assert e < TOL_DEC, (tag, steps, e)
        else:
            d = np.abs(rec.reshape(-1)[g[f"{tag}_rec{steps}_idx"]] - g[f"{tag}_rec{steps}_val"])
            ds = abs(float(rec.astype(np.float64).sum()) - float(g[f"{tag}_rec{steps}_sum"])) / rec.size
            print(f"[anysize] {tag}: {steps}-step decode max abs {d.max():.3e} on {d.size} pixels, sum/pixel {ds:.3e}")
            if steps in long_run:
                assert d.max() < 3e-5 and ds < 1e-5, (tag, steps, float(d.max()), ds)
            else:
                assert relerr(rec.reshape(-1)[g[f"{tag}_rec{steps}_idx"]], g[f"{tag}_rec{steps}_val"]) < TOL_DEC, (tag, steps, float(d.max()))
        # whole compress(): cropped reconstruction, bpp over H * W; the padded init is accepted as it is
        rec2, bpp = diff.compress(u8, sample_steps=steps, bpp_return_mean=False, init=init, **ekw, **ckw)
        assert rec2.shape == (B, 3, H, W)
        np.testing.assert_array_equal(bpp, out["bpp"])
        if not nflip and full:
            assert relerr(rec2, g[f"{tag}_rec{steps}"]) < TOL_DEC
        initp = np.zeros((B, 3, Hp, Wp), np.float32)
        initp[:, :, :H, :W] = init
        rec3, _ = diff.compress(u8, sample_steps=steps, bpp_return_mean=False, init=initp, **ekw, **ckw)
        np.testing.assert_array_equal(_bits(rec3), _bits(rec2))
        # bytes round trip: no shape needed, the same bits as compress()
        streams = diff.compress_to_bytes(u8, **ekw)
        want_version = (4 if rates is not None else 3) + (2 if (Hp, Wp) != (H, W) else 0)
        assert all(s[3] == want_version for s in streams), [s[3] for s in streams]
        assert comp.image_size_of(streams, comp.frame_multiple) == [(H, W)] * B
        rec4 = diff.decompress(streams, sample_steps=steps, init=init)
        np.testing.assert_array_equal(_bits(rec4), _bits(rec2))
        np.testing.assert_array_equal(_bits(diff.decompress(streams, (B, 3, H, W), sample_steps=steps, init=init)), _bits(rec2))
        with pytest.raises(_lib.CdcError, match="contradicts"):
            diff.decompress(streams, (B, 3, H + 1, W), sample_steps=steps, init=init)
        u = diff.decompress(streams, sample_steps=steps, init=init, as_uint8=True)
        assert u.dtype == np.uint8 and u.shape == (B, 3, H, W)
        if B > 1:                                               # a batch call returns the batch-1 streams byte for byte
            lat, hyp = comp.analysis(frame.pad(comp._enc_handle(), u8, Hp, Wp, 0), *fkw)
            for b in range(B):
                one = comp.latents_to_bytes(lat[b:b + 1], hyp[b:b + 1], None if rates is None else rates[b:b + 1], image_hw=(H, W))
                assert one[0] == comp.latents_to_bytes(lat, hyp, rates, image_hw=(H, W))[b]
        if want_version in (5, 6):                              # the size field is part of the stream: relabelled as 3 / 4 it is refused, not decoded
            bad = streams[0][:3] + bytes([want_version - 2]) + streams[0][4:]
            with pytest.raises(_lib.CdcError):
                diff.decompress([bad], sample_steps=steps, init=init[:1])
    assert un.status()["range_faults"] == 0 and comp.range_faults == 0, (un.status(), comp.status())
    return streams


@pytest.mark.parametrize("tag,key", [("x_10x10", "w10x10"), ("eps_33x48", "w33x48"), ("vbr_33x48", "w33x48")])
def test_small_models_any_size_match_reference(tag, key):
    g = np.load(os.path.join(GOLDEN, "anysize_small.npz"))
    model = tag.split("_")[0]
    diff, un, comp, rates = _small(model)
    ckw = {} if model == "x" else {"sample_mode": "ddim"}
    _check_case(diff, un, comp, g, tag, _images()[key], [4 if model == "x" else 3], True, rates=rates, **ckw)


@pytest.mark.parametrize("tag,steps", [("64x100", [4]), ("10x10", [4]), ("500x333", [4])])
def test_full_model_any_size_matches_reference(tag, steps):
    g = np.load(os.path.join(GOLDEN, "anysize_full_x_500x333.npz" if tag == "500x333" else "anysize_full_x.npz"))
    diff, un, comp = _full_x()
    _check_case(diff, un, comp, g, tag, _images()["w" + tag], steps, False)


def test_full_model_500x333_65_steps_matches_reference():
    """The reference script's default step count on the 500 x 333 window: the Kodak test's long-run bounds."""
    g = np.load(os.path.join(GOLDEN, "anysize_full_x_500x333.npz"))
    diff, un, comp = _full_x()
    u8 = _images()["w500x333"]
    init = synth.normal("init", u8.shape, seed=1, std=0.8)
    rec = diff.decompress(comp.decode(g["500x333_q_latent"]), u8.shape, sample_steps=65, init=init)
    d = np.abs(rec.reshape(-1)[g["500x333_rec65_idx"]] - g["500x333_rec65_val"])
    ds = abs(float(rec.astype(np.float64).sum()) - float(g["500x333_rec65_sum"])) / rec.size
    print(f"[anysize] 500x333: 65-step decode max abs {d.max():.3e} on {d.size} pixels, sum/pixel {ds:.3e}")
    assert d.max() < 3e-5, float(d.max())
    assert ds < 1e-5, ds
    assert un.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0} and comp.range_faults == 0


def test_exact_size_takes_todays_path_byte_for_byte(monkeypatch):
    """(256, 256): the new encode entry returns the bytes cdc_entropy_encode returns (version 3), compress() equals the fixture and
    neither compress() nor decompress() launches a frame kernel."""
    g = np.load(os.path.join(GOLDEN, "anysize_full_x.npz"))
    diff, un, comp = _full_x()
    u8 = _images()["w256x256"]
    x = (u8.astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    assert diff.padded_size(256, 256) == (256, 256)
    lat, hyp = comp.analysis(x)
    old = comp.latents_to_bytes(lat, hyp)
    new = comp.latents_to_bytes(lat, hyp, image_hw=(256, 256))
    assert old == new and old[0][3] == 3
    assert comp.compress_to_bytes(x) == old
    L = _lib.lib()
    calls = []
    real_pad, real_crop = L.cdc_frame_pad, L.cdc_frame_crop
    monkeypatch.setattr(L, "cdc_frame_pad", lambda *a: calls.append("pad") or real_pad(*a))
    monkeypatch.setattr(L, "cdc_frame_crop", lambda *a: calls.append("crop") or real_crop(*a))
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    L.cdc_prof_enable(un._handle(), 1)
    rec, bpp = diff.compress(x, sample_steps=4, bpp_return_mean=False, init=init)
    rec_b = diff.decompress(old, sample_steps=4, init=init)
    labels = []
    for i in range(L.cdc_prof_num_ops(un._handle())):
        lab = ctypes.c_char_p()
        L.cdc_prof_op(un._handle(), i, ctypes.byref(lab), None, None, None)
        labels.append(lab.value.decode())
    L.cdc_prof_enable(un._handle(), 0)
    assert calls == [] and labels and not any("frame" in s for s in labels), (calls, labels[:4])
    np.testing.assert_array_equal(_bits(rec), _bits(rec_b))
    d = relerr(rec.reshape(-1)[g["256x256_rec4_idx"]], g["256x256_rec4_val"])
    nflip = _symbols_close(comp(x)["q_latent"], g["256x256_q_latent"])
    print(f"[anysize] 256x256: decode relerr {d:.3e}, flipped {nflip}, bpp {bpp} reference {g['256x256_bpp']}")
    if nflip:
        FLIPPED.append("256x256")
    else:
        assert d < TOL_DEC
        assert np.abs(bpp - g["256x256_bpp"]).max() <= 1e-5 * float(np.abs(g["256x256_bpp"]).max())
    # the uint8 form of the same image goes through the conversion kernel and gives the same bits
    rec_u, bpp_u = diff.compress(u8, sample_steps=4, bpp_return_mean=False, init=init)
    assert calls == ["pad"]
    np.testing.assert_array_equal(_bits(rec_u), _bits(rec))
    np.testing.assert_array_equal(bpp_u, bpp)


def test_eta_draws_its_noise_at_the_padded_shape():
    """eta != 0: compress() of a 10 x 10 image is the window of the reference-shaped p_sample_loop on the 16 x 16 frame with the
    zero-extended init and the same host noise draws."""
    diff, un, comp, _ = _small("x")
    u8 = _images()["w10x10"]
    init = synth.normal("init", u8.shape, seed=1, std=0.8)
    np.random.seed(5)
    rec, _ = diff.compress(u8, sample_steps=3, bpp_return_mean=False, init=init, eta=0.5)
    assert rec.shape == (1, 3, 10, 10) and np.isfinite(rec).all()
    ctx = comp(frame.pad(comp._enc_handle(), u8, 16, 16, 0))["output"]
    initp = np.zeros((1, 3, 16, 16), np.float32)
    initp[:, :, :10, :10] = init
    np.random.seed(5)
    diff.set_sample_schedule(3)
    full = diff.p_sample_loop((1, 3, 16, 16), ctx, clip_denoised=True, init=initp, eta=0.5)
    np.testing.assert_array_equal(_bits(rec), _bits(full[:, :, :10, :10]))
    with pytest.raises(_lib.CdcError, match="init has shape"):
        diff.compress(u8, sample_steps=3, init=np.zeros((1, 3, 12, 12), np.float32))


def test_version_5_header_refusals_in_the_decoder():
    """A hand-edited size field: img_h = 0, one row beyond the coded extent, one block short of it -- refused before anything is decoded."""
    diff, un, comp, _ = _small("eps")
    u8 = _images()["w33x48"][:1]
    s = diff.compress_to_bytes(u8)[0]
    assert s[3] == 5 and comp.image_size_of([s], comp.frame_multiple) == [(33, 48)]
    M = comp.frame_multiple                                     # 16: coded extent 48 x 48

    def with_size(h, w):
        return s[:34] + int(h).to_bytes(4, "little") + int(w).to_bytes(4, "little") + s[42:]

    assert with_size(33, 48) == s
    for h, w in ((49, 48), (32, 48), (33, 49), (33, 32), (2 ** 31 - 1, 48)):
        with pytest.raises(_lib.CdcError, match="does not pad to the coded extent"):
            comp.decompress_from_bytes([with_size(h, w)])
    for h, w in ((0, 48), (33, 0), (2 ** 32 - 1, 48), (33, 2 ** 31)):       # no size at all: the peeks already refuse the header
        with pytest.raises(_lib.CdcError, match="not a CDC bitstream"):
            comp.decompress_from_bytes([with_size(h, w)])
    q = comp.decompress_from_bytes([with_size(48, 48)])         # the extent itself is a valid recorded size
    assert q.shape[-2:] == (48 // M * 4, 48 // M * 4)
    with pytest.raises(_lib.CdcError):
        comp.decompress_from_bytes([s[:40]])


def test_example_script_round_trips_a_500x333_png(tmp_path):
    """examples/test_xparam.py on a folder holding the 500 x 333 PNG writes a 500 x 333 PNG: the fixture's uint8 image except where
    the float reconstruction lies within the decode bound of a rounding boundary, and prints the fixture's bpp."""
    Image = pytest.importorskip("PIL.Image")
    g = {**np.load(os.path.join(GOLDEN, "anysize_full_x_500x333.npz")), **np.load(os.path.join(GOLDEN, "anysize_full_x_500x333_saved.npz"))}
    u8 = _images()["w500x333"][0]
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(u8.transpose(1, 2, 0)).save(src / "a.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                        "--n_denoise_step", "65", "--img_dir", str(src), "--out_dir", str(dst)],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, CDC_SYNTHETIC_INIT="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.asarray(Image.open(dst / "a.png").convert("RGB")).transpose(2, 0, 1)
    assert got.shape == (3, 500, 333)
    want = g["500x333_u8_65"][0]
    near = np.unpackbits(g["500x333_near_65"])[: want.size].reshape(want.shape).astype(bool)
    differ = got != want
    print(f"[anysize] example: {int(differ.sum())} of {want.size} pixels differ, {int(near.sum())} lie near a rounding boundary")
    assert not (differ & ~near).any(), int((differ & ~near).sum())
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    bpp = [float(line.split("(")[1].split(",")[0].split(")")[0]) for line in r.stdout.splitlines() if line.startswith("bpp:")]
    # (the printed value against the reference's, as test_inference_script_counterpart_on_kodak_crops does)
    assert len(bpp) == 1 and abs(bpp[0] - float(g["500x333_bpp"][0])) <= 1e-5 * float(g["500x333_bpp"][0]), (bpp, g["500x333_bpp"])


def test_at_most_one_image_flipped_a_symbol():
    """Runs last: the bpp comparison was skipped for the images listed here (a GPU symbol on a rounding boundary)."""
    print(f"[anysize] images whose bpp comparison was skipped for a flipped symbol: {FLIPPED}")
    assert len(FLIPPED) <= 1, FLIPPED
