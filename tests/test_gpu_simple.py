"""SimpleCompressor (the GDN context model of the epsilon tree) on the GPU: the GDN1 operator against the real reference's outputs
and a float64 evaluation, then context decoder, hyper decoder, encoder, forward, end-to-end compress, streams and evaluate() against
the goldens of tests/golden/make_golden_simple.py.

Tolerances, as tests/test_gpu_parity.py states them: the outer bound is TOL = 1e-4 * max(1, max|ref|).  Every figure is printed
before it is asserted (run with -s).
  GDN operator against float64 numpy, element-wise relative error: bounded by the arithmetic itself -- the norm is a float32 fmaf
      chain of C + 1 non-negative terms (relative error <= (C + 1) 2^-24), the quotient / product rounds once more: (C + 2) 2^-24
      (1.2e-5 at C = 192, 1.1e-6 at C = 16).
  one compressor stage against the reference golden: TOL_FWD, the project's bound for a compressor forward or a stage of it.
  the three-step compress() against the reference golden: TOL_DEC, the project's bound for a few-step decode chain.
No figure measured on the MI355X is recorded here yet: these are reasoned bounds, not 3x a measurement.  The first run with -s prints
every figure; the constants tighten to about 3x of them then (tests/test_gpu_parity.py's rule)."""
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from cdc_compression_amd.ops import Ops
from helpers import GOLDEN
from simple_ref import gdn1_np, gdn_case, gdn_reparam_np

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_FWD = 1e-5     # as tests/test_gpu_parity.py
TOL_DEC = 5e-5
SIMPLE = ["simple_small", "simple_full"]


def relerr(a, ref, what=""):
    e = float(np.abs(np.asarray(a) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print(f"[simple] {what}: relerr {e:.3e}")
    return e


def elem_relerr(a, want, what=""):
    nz = want != 0
    e = float((np.abs(a[nz] - want[nz]) / np.abs(want[nz])).max())
    print(f"[simple] {what}: element-wise relative error {e:.3e}")
    return e


@pytest.fixture(scope="module")
def G():
    return Ops(0)


@pytest.fixture(scope="module")
def gdn_ops():
    return np.load(os.path.join(GOLDEN, "gdn_ops.npz"))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", range(4))
def test_gdn_matches_reference_and_float64(G, gdn_ops, k, inverse):
    shape, x, beta, gamma, y, yinv = gdn_case(gdn_ops, k)
    ref = yinv if inverse else y
    got = G.gdn(x, beta, gamma, inverse)
    assert got.shape == ref.shape and got.dtype == np.float32
    want = gdn1_np(x, *gdn_reparam_np(beta, gamma), inverse)
    e64 = elem_relerr(got, want, f"gdn {shape}{' inv' if inverse else ''} vs float64")
    eref = relerr(got, ref, f"gdn {shape}{' inv' if inverse else ''} vs reference")
    assert (got[want == 0] == 0).all()
    assert e64 <= (shape[1] + 2) * 2.0 ** -24, e64
    assert eref < TOL_FWD, eref
    assert G.status()["nonfinite_results"] == 0


def test_gdn_refuses_unsupported_channels_without_a_launch(G):
    L = _lib.lib()
    for C in (24, 8, 272):
        x = synth.normal("x", (1, C, 4, 4), seed=1)
        beta, gamma = synth.gdn_layer_params(C, seed=1)
        y = np.empty_like(x)
        G.prof(True)
        rc = L.cdc_op_gdn(G._h, x.ctypes.data, beta.ctypes.data, gamma.ctypes.data, y.ctypes.data, 1, C, 16, 0)
        assert rc == -4 and f"GDN over {C} channels".encode() in L.cdc_last_error(G._h), (rc, L.cdc_last_error(G._h))
        assert G.prof_total_ms()[1] == 0
        G.prof(False)
    with pytest.raises(_lib.CdcError, match="multiples of 16"):
        G.gdn(synth.normal("x", (1, 24, 4, 4), seed=1), *synth.gdn_layer_params(24, seed=1))


def test_gdn_batch_equals_batch1_calls_bit_for_bit(G, gdn_ops):
    shape, x, beta, gamma, _, _ = gdn_case(gdn_ops, 1)
    assert shape[0] == 3
    for inverse in (False, True):
        got = G.gdn(x, beta, gamma, inverse)
        one = np.concatenate([G.gdn(x[b:b + 1], beta, gamma, inverse) for b in range(3)])
        np.testing.assert_array_equal(got.view(np.uint32), one.view(np.uint32))


def test_gdn_stress_reproduces_its_bits(G, gdn_ops):
    shape, x, beta, gamma, _, _ = gdn_case(gdn_ops, 1)
    G.stress(2000)
    try:
        G.gdn(x, beta, gamma)
        assert G.stress_result() == (2000, 0)
    finally:
        G.stress(0)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _load(name):
    meta = json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))
    return meta, np.load(os.path.join(GOLDEN, f"{name}.npz"))


def _model(meta, arith=None, kwargs_key="kwargs", manifest_key="manifest"):
    man = [(k, tuple(v)) for k, v in meta[manifest_key]]
    sd = synth.simple_compressor_state_dict(man, seed=meta["seed"])
    m = cdc.epsilonparam.SimpleCompressor(**meta[kwargs_key])
    if arith is not None:
        for hnd in (m._handle(), m._hyper_handle(), m._enc_handle()):
            _lib.check(hnd, _lib.lib().cdc_set_arith(hnd, arith))
    m.load_state_dict(sd)
    return m


def _inputs(meta):
    B, _, H, W = meta["image_shape"]
    s, kw = meta["seeds"], meta["kwargs"]
    n, nh = len(kw["dim_mults"]), len(kw["hyper_dims_mults"])
    x = synth.normal("simple_image", (B, 3, H, W), seed=s["image"], std=0.5).clip(-1, 1).astype(np.float32)
    q = np.round(synth.normal("simple_q_latent", (B, kw["dim"] * kw["dim_mults"][-1], H >> n, W >> n), seed=s["q_latent"], std=2.0)).astype(np.float32)
    qh = (np.round(synth.normal("simple_q_hyper", (B, kw["dim"] * kw["hyper_dims_mults"][-1], H >> (n + nh - 1), W >> (n + nh - 1)),
                                seed=s["q_hyper"], std=2.0)) + 0.25).astype(np.float32)
    return x, q, qh


def _check(a, g, key, tol=TOL_FWD):
    a = np.asarray(a)
    assert list(a.shape) == list(g[f"{key}_shape"]), key
    e = relerr(a.reshape(-1)[g[f"{key}_idx"]], g[f"{key}_val"], f"{key} (digest)")
    assert e < tol, (key, e)
    if key in g.files:
        e = relerr(a, g[key], key)
        assert e < tol, (key, e)


def _symbols_close(a, ref, cap_floor):
    """As tests/test_gpu_parity.py: equal up to round-off except single-step flips at rounding boundaries; at most max(1, 1e-4 n) of
    them -- the cap the float32 reference itself was held to against its float64 evaluation (the fixture's flips_* counts)."""
    d = np.abs(np.asarray(a) - ref)
    near = d <= 1.5e-5 * max(1.0, float(np.abs(ref).max()))
    flip = np.abs(d - 1.0) <= 1e-3
    print(f"[simple] symbols: {int(flip.sum())} of {flip.size} flipped (the float32 reference against float64: {cap_floor})")
    assert (near | flip).all()
    assert flip.sum() <= max(1, int(1e-4 * flip.size)), (int(flip.sum()), flip.size)
    return int(flip.sum())


def _check_model(m, meta, g):
    x, q, qh = _inputs(meta)
    outs = m.decode(q)                                           # synthesis transform, finest first
    assert len(outs) == len(meta["kwargs"]["dim_mults"])
    for i, o in enumerate(outs):
        _check(o, g, f"dec{i}")
    mean, scale = m.hyper_decode(qh)
    _check(mean, g, "mean")
    _check(scale, g, "scale")
    assert float(np.asarray(scale).min()) >= 0.1
    latent, hyper = m.analysis(x)
    _check(latent, g, "latent")
    _check(hyper, g, "hyper_latent")
    out = m(x)
    assert int(g["flips_q_latent"]) <= max(1, int(1e-4 * g["q_latent"].size))
    _symbols_close(out["q_latent"], g["q_latent"], int(g["flips_q_latent"]))
    _symbols_close(out["q_hyper_latent"], g["q_hyper_latent"], int(g["flips_q_hyper_latent"]))
    ref_bpp = g["bpp"]
    print(f"[simple] bpp {out['bpp']} reference {ref_bpp}")
    assert np.abs(out["bpp"] - ref_bpp).max() <= 1e-4 * max(1.0, float(np.abs(ref_bpp).max())), (out["bpp"], ref_bpp)
    # the pyramid of the forward, from the GOLDEN symbols: a flipped symbol of ours cannot propagate into this check
    for i, o in enumerate(m.decode(g["q_latent"])):
        _check(o, g, f"ctx{i}")
    st = m.status()
    assert all(v["nonfinite_results"] == 0 and v["range_faults"] == 0 for v in st.values()), st


@pytest.mark.parametrize("name", SIMPLE)
def test_simple_compressor_matches_reference_golden(name):
    meta, g = _load(name)
    _check_model(_model(meta), meta, g)


def test_simple_compressor_in_bf16x3_arithmetic_meets_the_same_goldens():
    meta, g = _load("simple_small")
    m = _model(meta, arith=0)                                    # CDC_ARITH_BF16X3
    _check_model(m, meta, g)
    assert all(v["arith"] == 0 for v in m.status().values())


def test_simple_programs_run_the_gdn_kernel():
    """The launch programs hold one GDN op per level but the last (inverse in the decoder), labelled as the planner labels them."""
    import ctypes
    meta, g = _load("simple_small")
    m = _model(meta)
    x, q, _ = _inputs(meta)
    m.decode(q)
    m.analysis(x)
    L = _lib.lib()

    def labels(h):
        out = []
        for i in range(L.cdc_prof_num_ops(h)):
            lab = ctypes.c_char_p()
            L.cdc_prof_op(h, i, ctypes.byref(lab), None, None, None)
            out.append(lab.value.decode())
        return out
    dec, enc = labels(m._handle()), labels(m._enc_handle())
    assert [s for s in dec if s.startswith("gdn")] == ["gdn C=48 HW=128 inv", "gdn C=32 HW=512 inv", "gdn C=16 HW=2048 inv"], dec
    assert [s for s in enc if s.startswith("gdn")] == ["gdn C=16 HW=2048", "gdn C=32 HW=512", "gdn C=48 HW=128"], enc
    assert sum(s.startswith("conv") for s in dec) == 4 and sum(s.startswith("conv") for s in enc) == 4 + 3


def _e2e():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_simple_e2e.json")))
    g = np.load(os.path.join(GOLDEN, "simple_e2e.npz"))
    uman = [(k, tuple(v)) for k, v in meta["unet_manifest"]]
    un = cdc.epsilonparam.Unet(**meta["unet_kwargs"])
    un.load_state_dict(synth.unet_state_dict(uman, seed=0, final_gain=0.2))
    comp = _model(meta, kwargs_key="comp_kwargs", manifest_key="comp_manifest")
    diff = cdc.GaussianDiffusionEps(un, comp, **meta["diffusion"])
    H, W = meta["H"], meta["W"]
    x = synth.normal("simple_e2e_image", (1, 3, H, W), seed=meta["image_seed"], std=0.5).clip(-1, 1).astype(np.float32)
    init = synth.normal("init", (1, 3, H, W), seed=1, std=0.8)
    return meta, g, diff, comp, x, init


def test_compress_end_to_end_matches_reference_golden():
    meta, g, diff, comp, x, init = _e2e()
    assert int(g["flips_q_latent"]) == 0                        # the float32 reference's symbols are those of float64 here
    rec, bpp = diff.compress(x, meta["steps"], None, "ddim", bpp_return_mean=False, init=init)
    e = relerr(rec, g["rec"], "compress() reconstruction")
    print(f"[simple] e2e bpp {bpp} reference {g['bpp']}")
    assert e < TOL_DEC, e
    assert np.abs(bpp - g["bpp"]).max() <= 1e-4 * max(1.0, float(np.abs(g["bpp"]).max())), (bpp, g["bpp"])


def test_streams_round_trip_at_frame_and_odd_sizes():
    """compress_to_bytes -> decompress: q_latent equals the encoder's; version 3 at 64 x 64, version 5 at 50 x 70; the streams of a
    batch equal the batch-1 streams of the same latent rows byte for byte; decompress(streams) equals compress() per image."""
    meta, g, diff, comp, _, _ = _e2e()
    for (H, W), version in (((64, 64), 3), ((50, 70), 5)):
        x = synth.normal("simple_rt_image", (2, 3, H, W), seed=3, std=0.5).clip(-1, 1).astype(np.float32)
        init = synth.normal("init", (2, 3, H, W), seed=1, std=0.8)
        streams = diff.compress_to_bytes(x)
        assert len(streams) == 2 and all(s[:3] == b"CDC" and s[3] == version for s in streams), [s[:4] for s in streams]
        assert comp.image_size_of(streams, comp.frame_multiple) == [(H, W)] * 2
        q, (h_rec, w_rec) = comp.decompress_from_bytes(streams, return_image_size=True)
        assert (h_rec, w_rec) == (H, W)
        framed, hw = comp._framed(x)
        assert hw == (H, W) and tuple(framed.shape[2:]) == comp.padded_size(H, W)
        latent, hyper = comp.analysis(framed)
        assert comp.latents_to_bytes(latent, hyper, image_hw=hw) == streams
        for b in range(2):
            assert comp.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], image_hw=hw)[0] == streams[b]
            q_hyper = comp.dequantize(hyper[b:b + 1], comp._medians_like(hyper[b:b + 1]))
            mean, _ = comp.hyper_decode(q_hyper)
            ql, qh = comp.decompress_from_bytes([streams[b]], return_hyper=True)
            np.testing.assert_array_equal(ql, comp.dequantize(latent[b:b + 1], mean))
            np.testing.assert_array_equal(qh, q_hyper)
            np.testing.assert_array_equal(ql, q[b:b + 1])
            # decompress(streams) is compress() of the same image (batch-1 plans on both sides), bit for bit
            one = diff.compress_to_bytes(x[b:b + 1])
            rec, _ = diff.compress(x[b:b + 1], 2, None, "ddim", init=init[b:b + 1])
            rec_s = diff.decompress(one, None, 2, init[b:b + 1])
            assert rec.shape == (1, 3, H, W)
            np.testing.assert_array_equal(rec_s.view(np.uint32), rec.view(np.uint32))


def test_evaluate_returns_psnr():
    meta, g, diff, comp, x, init = _e2e()
    x2 = np.concatenate([x, -x])
    out = diff.evaluate(x2, 2, None, "ddim", init=np.concatenate([init, init]))
    assert out["reconstruction"].shape == x2.shape and out["bpp"].shape == (2,)
    assert out["psnr"].shape == (2,) and np.isfinite(out["psnr"]).all() and out["ms_ssim"] is None
    from cdc_compression_amd import metrics
    np.testing.assert_array_equal(out["psnr"], metrics.psnr(diff.denoise_fn, out["reconstruction"], x2, as_saved=True))
