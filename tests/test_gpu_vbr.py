"""Variable-bitrate context model (BigCompressor(vbr=True)) on the GPU against the real reference's goldens
(tests/golden/make_golden_vbr.py): synthesis transform, hyper decoder, encoder and the whole forward at three rate cases (distinct
rates, one broadcast rate, an extrapolated rate with negative scales at every site), under the default plan, CDC_PF=0, CDC_PF=1
and the bf16x3 arithmetic; batch = batch-1; version-4 bitstreams; the end-to-end compress() of the reference."""
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
TOL_FWD = 1e-5     # as tests/test_gpu_parity.py: one compressor forward (or a stage of it) against the reference golden
TOL_DEC = 5e-5     # a few-step decode chain against the reference golden
MODES = {"default": ({}, None), "pf0": ({"CDC_PF": "0"}, None), "pf1": ({"CDC_PF": "1", "CDC_PF_MAXPIX": "0"}, None),
         "bf16x3": ({}, 0)}
CASES = ["distinct", "bcast", "neg"]


def relerr(a, ref):
    return float(np.abs(np.asarray(a) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def _symbols_close(a, ref, max_flip_frac=1e-4):
    """As tests/test_gpu_parity.py: equal up to round-off except single-step flips at rounding boundaries (a small fraction)."""
    d = np.abs(a - ref)
    near = d <= 1.5e-5 * max(1.0, float(np.abs(ref).max()))
    flip = np.abs(d - 1.0) <= 1e-3
    assert (near | flip).all()
    assert flip.sum() <= max(1, int(max_flip_frac * flip.size)), (int(flip.sum()), flip.size)


def _load(name):
    meta = json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))
    return meta, np.load(os.path.join(GOLDEN, f"{name}.npz"))


def _model(meta, mode=None, monkeypatch=None, vbr=True):
    env, arith = MODES[mode or "default"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    man = [(k, tuple(v)) for k, v in meta["manifest"]]
    sd = synth.compressor_state_dict(man, seed=meta["seed"])
    if not vbr:
        sd = {k: v for k, v in sd.items() if not synth.is_vbr_key(k)}
    m = cdc.BigCompressor(vbr=vbr, **meta["kwargs"])
    if arith is not None:
        for hnd in (m._handle(), m._hyper_handle(), m._enc_handle()):
            _lib.check(hnd, _lib.lib().cdc_set_arith(hnd, arith))
    m.load_state_dict(sd)
    return m


def _inputs(meta, B):
    s = meta["seeds"]
    x = synth.normal("vbr_image", (3, 3) + tuple(meta["image_hw"]), seed=s["image"], std=0.5).clip(-1, 1).astype(np.float32)[:B]
    kw = meta["kwargs"]
    c0 = kw["dim"] * kw["dim_mults"][-1]
    q = np.round(synth.normal("vbr_q_latent", (3, c0) + tuple(meta["latent_hw"]), seed=s["q_latent"], std=2.0)).astype(np.float32)[:B]
    ch = kw["dim"] * kw["hyper_dims_mults"][-1]
    qh = (np.round(synth.normal("vbr_q_hyper", (3, ch) + tuple(meta["hyper_hw"]), seed=s["q_hyper"], std=2.0)) + 0.25).astype(np.float32)[:B]
    return x, q, qh


def _check(a, g, key, tol=TOL_FWD):
    a = np.asarray(a)
    assert list(a.shape) == list(g[f"{key}_shape"]), key
    assert relerr(a.reshape(-1)[g[f"{key}_idx"]], g[f"{key}_val"]) < tol, (key, relerr(a.reshape(-1)[g[f"{key}_idx"]], g[f"{key}_val"]))
    if key in g.files:
        assert relerr(a, g[key]) < tol, (key, relerr(a, g[key]))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["vbr_small", "vbr_full"])
def test_vbr_compressor_matches_reference_golden(name, mode, monkeypatch):
    meta, g = _load(name)
    m = _model(meta, mode, monkeypatch)
    for case in CASES:
        rates = g[f"{case}_rates"]
        B = int(g[f"{case}_B"])
        x, q, qh = _inputs(meta, B)
        # synthesis transform (Compressor.decode), finest first
        outs = m.decode(q, rates)
        for i, o in enumerate(outs):
            _check(o, g, f"{case}_dec{i}")
        # hyper decoder
        mean, scale = m.hyper_decode(qh, cond=rates)
        _check(mean, g, f"{case}_mean")
        _check(scale, g, f"{case}_scale")
        assert float(scale.min()) >= 0.1
        # analysis transform + hyper encoder
        latent, hyper = m.analysis(x, rates)
        _check(latent, g, f"{case}_latent")
        _check(hyper, g, f"{case}_hyper_latent")
        # the whole forward
        out = m(x, rates)
        for key in ("q_latent", "q_hyper_latent"):
            if f"{case}_{key}" in g.files:
                _symbols_close(out[key], g[f"{case}_{key}"])
        ref_bpp = g[f"{case}_bpp"]
        assert np.abs(out["bpp"] - ref_bpp).max() <= 2e-3 * max(1.0, float(np.abs(ref_bpp).max())), (case, out["bpp"], ref_bpp)
        if f"{case}_q_latent" in g.files and np.array_equal(out["q_latent"], g[f"{case}_q_latent"]):
            for i in range(len(out["output"])):
                _check(out["output"][i], g, f"{case}_ctx{i}")
    assert m.status()["dec"]["nonfinite_results"] == 0


def test_vbr_rate_changes_the_result_and_is_required():
    """The affine is applied at every site (different rates, different outputs), and the library itself refuses a call with no
    rate, or with a rate count that fits neither 1 nor B -- no default."""
    meta, g = _load("vbr_small")
    m = _model(meta)
    x, q, qh = _inputs(meta, 2)
    a = m.decode(q, np.array([0.2], np.float32))
    b = m.decode(q, np.array([0.8], np.float32))
    assert all(relerr(u, v) > 1e-3 for u, v in zip(a, b))
    L = _lib.lib()
    fresh = _model(meta)
    h = fresh._hyper_handle()
    mean = np.empty((2, fresh.reversed_hyper_dims[-1] // 2, 8, 8), np.float32)     # hyper_dec: x4 up from 2 x 2
    scale = np.empty_like(mean)
    rc = L.cdc_hyperdec_decode(h, qh.ctypes.data, mean.ctypes.data, scale.ctypes.data, 2, 2, 2, 0.1, 0, None)
    assert rc == -2 and b"no bitrate_scale set" in L.cdc_last_error(h)
    three = np.array([0.1, 0.2, 0.3], np.float32)
    _lib.check(h, L.cdc_set_bitrate_scale(h, three.ctypes.data, 3))
    rc = L.cdc_hyperdec_decode(h, qh.ctypes.data, mean.ctypes.data, scale.ctypes.data, 2, 2, 2, 0.1, 0, None)
    assert rc == -1 and b"3 values for a batch of 2" in L.cdc_last_error(h)


@pytest.mark.parametrize("mode", ["default", "pf1"])
def test_vbr_batch_equals_batch1_calls(mode, monkeypatch):
    """Image b's result depends on its own rate only: a distinct-rate batch equals B batch-1 calls (streams byte for byte,
    their decoded latents bit for bit; the float stages within TOL_FWD, as the launch plans depend on the batch)."""
    meta, g = _load("vbr_full")
    m = _model(meta, mode, monkeypatch)
    rates = np.array([0.0, 0.37, 1.0], np.float32)
    x, q, qh = _inputs(meta, 3)
    outs = m.decode(q, rates)
    mean, scale = m.hyper_decode(qh, cond=rates)
    latent, hyper = m.analysis(x, rates)
    streams = m.latents_to_bytes(latent, hyper, rates)
    for b in range(3):
        r = rates[b:b + 1]
        for o, o1 in zip(outs, m.decode(q[b:b + 1], r)):
            assert relerr(o[b:b + 1], o1) < TOL_FWD
        m1, s1 = m.hyper_decode(qh[b:b + 1], cond=r)
        assert relerr(mean[b:b + 1], m1) < TOL_FWD and relerr(scale[b:b + 1], s1) < TOL_FWD
        l1, h1 = m.analysis(x[b:b + 1], r)
        assert relerr(latent[b:b + 1], l1) < TOL_FWD and relerr(hyper[b:b + 1], h1) < TOL_FWD
        assert m.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], r)[0] == streams[b]
    q_all = m.decompress_from_bytes(streams)
    np.testing.assert_array_equal(q_all, np.concatenate([m.decompress_from_bytes([s]) for s in streams]))


def test_vbr_bitstreams_round_trip_and_carry_the_rate():
    meta, g = _load("vbr_full")
    m = _model(meta)
    rates = np.array([0.0, 0.37, 1.0], np.float32)
    x, _, _ = _inputs(meta, 3)
    latent, hyper = m.analysis(x, rates)
    streams = m.compress_to_bytes(x, rates)
    assert all(s[:4] == b"CDC\x04" for s in streams)
    np.testing.assert_array_equal(m.bitrate_scale_of(streams).view(np.uint32), rates.view(np.uint32))
    for b in range(3):
        q_hyper = m.dequantize(hyper[b:b + 1], m._medians_like(hyper[b:b + 1]))
        mean, _ = m.hyper_decode(q_hyper, cond=rates[b:b + 1])
        q_latent = m.dequantize(latent[b:b + 1], mean)
        ql, qh, rr = m.decompress_from_bytes([streams[b]], return_hyper=True, return_bitrate_scale=True)
        np.testing.assert_array_equal(ql, q_latent)
        np.testing.assert_array_equal(qh, q_hyper)
        assert rr.view(np.uint32)[0] == rates.view(np.uint32)[b]
    # one decode call holding streams of different rates, coded in different calls (and a broadcast rate)
    other = m.compress_to_bytes(x[:2], np.array([0.6], np.float32))
    np.testing.assert_array_equal(m.bitrate_scale_of(other), np.array([0.6, 0.6], np.float32))
    mixed = [streams[0], other[1], streams[2]]
    q_mixed = m.decompress_from_bytes(mixed)
    np.testing.assert_array_equal(q_mixed, np.concatenate([m.decompress_from_bytes([s]) for s in mixed]))
    # the handle's own rate is left as it was: a latents_to_bytes with no new rate set reuses it
    h = m._hyper_handle()
    one = np.array([0.37], np.float32)
    _lib.check(h, _lib.lib().cdc_set_bitrate_scale(h, one.ctypes.data, 1))
    m.decompress_from_bytes(mixed)
    q1 = m.dequantize(hyper[1:2], m._medians_like(hyper[1:2]))
    assert q1.shape[2:] == (1, 1)
    mean_a = np.empty((1, m.reversed_hyper_dims[-1] // 2, 4, 4), np.float32)
    mean_b = np.empty_like(mean_a)
    sc = np.empty_like(mean_a)
    L = _lib.lib()
    _lib.check(h, L.cdc_hyperdec_decode(h, q1.ctypes.data, mean_a.ctypes.data, sc.ctypes.data, 1, 1, 1, 0.1, 0, None))
    mean_b[...] = m.hyper_decode(q1, cond=one)[0]
    np.testing.assert_array_equal(mean_a, mean_b)
    # version 3 / version 4 mismatches are refused by the library
    fixed = _model(meta, vbr=False)
    v3 = fixed.compress_to_bytes(x[:1])
    assert v3[0][:4] == b"CDC\x03"
    with pytest.raises(_lib.CdcError, match="fixed-rate stream"):
        m.decompress_from_bytes(v3)
    with pytest.raises(_lib.CdcError, match="variable-bitrate stream"):
        fixed.decompress_from_bytes(streams[:1])


def _e2e():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_e2e.json")))
    g = np.load(os.path.join(GOLDEN, "vbr_e2e.npz"))
    uman = [(k, tuple(v)) for k, v in meta["unet_manifest"]]
    un = cdc.Unet(**meta["unet_kwargs"])
    un.load_state_dict(synth.unet_state_dict(uman, seed=0, final_gain=0.2))
    cman = [(k, tuple(v)) for k, v in meta["comp_manifest"]]
    comp = cdc.BigCompressor(vbr=True, **meta["comp_kwargs"])
    comp.load_state_dict(synth.compressor_state_dict(cman, seed=meta["seed"]))
    diff = cdc.GaussianDiffusionEps(un, comp, **meta["diffusion"])
    B, H, W = len(meta["rates"]), meta["H"], meta["W"]
    x = synth.normal("vbr_e2e_image", (B, 3, H, W), seed=26, std=0.5).clip(-1, 1).astype(np.float32)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    return meta, g, diff, comp, x, init


def test_vbr_compress_end_to_end_matches_reference_golden():
    meta, g, diff, comp, x, init = _e2e()
    rec, bpp = diff.compress(x, meta["steps"], bitrate_scale=g["rates"], sample_mode="ddim", bpp_return_mean=False, init=init)
    assert relerr(rec, g["rec"]) < TOL_DEC, relerr(rec, g["rec"])
    assert np.abs(bpp - g["bpp"]).max() <= 2e-3 * max(1.0, float(np.abs(g["bpp"]).max())), (bpp, g["bpp"])
    with pytest.raises(ValueError, match="needs a bitrate_scale"):
        diff.compress(x, 2, sample_mode="ddim", init=init)


def test_vbr_decompress_from_streams_equals_compress():
    """decompress(streams) needs no rate: each stream carries its own.  Per image (batch-1 plans on both sides) the
    reconstruction equals compress()'s bit for bit; a batch of three rates agrees within round-off; decompress(q_latent,
    bitrate_scale=...) is the latent form."""
    meta, g, diff, comp, x, init = _e2e()
    for b, r in enumerate(g["rates"]):
        rr = np.array([r], np.float32)
        rec, _ = diff.compress(x[b:b + 1], 2, bitrate_scale=rr, sample_mode="ddim", init=init[b:b + 1])
        streams = diff.compress_to_bytes(x[b:b + 1], bitrate_scale=rr)
        np.testing.assert_array_equal(diff.decompress(streams, x[b:b + 1].shape, 2, init[b:b + 1]), rec)
        q_latent = comp(x[b:b + 1], rr)["q_latent"]
        np.testing.assert_array_equal(diff.decompress(q_latent, x[b:b + 1].shape, 2, init[b:b + 1], bitrate_scale=rr), rec)
    rec3, _ = diff.compress(x, 2, bitrate_scale=g["rates"], sample_mode="ddim", init=init)
    streams = diff.compress_to_bytes(x, bitrate_scale=g["rates"])
    assert relerr(diff.decompress(streams, x.shape, 2, init), rec3) < 2e-5
