"""cdc_distortion on the GPU (csrc/metric_kernels.hip) against the float64 restatement of tests/metrics_ref.py, which
tests/test_metrics_host.py checks on the CPU.  Inputs are made here; a reference is computed once and shared by the host-pointer and
the device-pointer run.  Bounds: PSNR of two byte operands 1e-12 relative (the MSE is an exact integer ratio), float PSNR 1e-3 dB at
<= 45 dB, MS-SSIM and each of its 15 components 1e-5 absolute.  The worst figures seen are printed (profiles/metrics.md quotes them:
float PSNR 1.0e-5 dB, MS-SSIM 2.0e-8 on an MI355X)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cdc_compression_amd as cdc
import metrics_ref as R
from cdc_compression_amd import _lib, metrics, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PSNR_SIZES = [(1, 1), (7, 3), (5, 4), (64, 64), (333, 500), (161, 162)]
TH, TW = 16, 32                                   # the MS-SSIM tile of the valid map (metric_kernels.hip)
# 161 x 161: the minimum (a 1 x 1 last map); 171 x 202 / 170 x 203: a valid map one pixel beyond a whole number of tiles, in each direction
MS_SIZES = [(161, 161), (162, 161), (176, 203), (333, 500), (10 + 10 * TH + 1, 10 + 6 * TW), (10 + 10 * TH, 10 + 6 * TW + 1)]
SIGMAS = [0.01, 0.05, 0.2]
WHERE = ["host", "device"]
WORST = {"psnr_db": 0.0, "msssim": 0.0}


@functools.lru_cache(maxsize=None)
def _model():
    return cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))


def _to(where):
    if where == "device":
        import torch
        return lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return lambda a: a


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _in_frame(win, fill, mult=64, extra=0):
    """The window inside a frame of sides 64 ceil(. / 64) (+ extra) whose outside is `fill`."""
    B, C, H, W = win.shape
    f = np.full((B, C, -(-H // mult) * mult + extra, -(-W // mult) * mult + extra), fill, win.dtype)
    f[:, :, :H, :W] = win
    return f


# ---- 1. PSNR of two byte operands: the exact integer MSE ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _byte_case(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    a = rng.integers(0, 256, (3, 3, H, W), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    f = rng.uniform(-1.3, 1.3, a.shape).astype(np.float32)               # the clamp works; its saved bytes against b
    return a, b, f, R.psnr(a, b), R.psnr(f, b, saved_a=True)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("H,W", PSNR_SIZES)
def test_psnr_of_bytes_is_exact(H, W, where):
    m, to = _model(), _to(where)
    a, b, f, want_u8, want_saved = _byte_case(H, W)
    close = lambda got, want: np.all(np.abs(got - want) <= 1e-12 * np.abs(want))     # noqa: E731
    got = metrics.psnr(m, to(a), to(b))
    assert got.dtype == np.float64 and got.shape == (3,) and close(got, want_u8), (got, want_u8)
    assert close(metrics.psnr(m, to(f), to(b), as_saved=True), want_saved)
    assert close(metrics.psnr(m, to(b), to(f), as_saved=(False, True)), want_saved)
    # frame operands: each its own frame, 64 ceil(. / 64) on a side and one that is not a multiple of 4
    assert close(metrics.psnr(m, to(_in_frame(a, 255)), to(_in_frame(b, 7, extra=3)), size=(H, W)), want_u8)
    assert close(metrics.psnr(m, to(_in_frame(f, 1e30)), to(b), size=(H, W), as_saved=True), want_saved)
    assert np.all(np.isposinf(metrics.psnr(m, to(a), to(a.copy()))))
    assert np.all(np.isposinf(metrics.psnr(m, to(f), to(R.saved_u8(f)), as_saved=True)))


def test_psnr_gives_the_same_bits_from_host_and_device_memory():
    """The host-staging path of cdc_distortion against device operands: 37 x 50 windows of 64 x 64 frames, every operand kind."""
    m, dev = _model(), _to("device")
    a, b, f, _, _ = _byte_case(37, 50)
    g = np.random.default_rng(5).uniform(-1.3, 1.3, f.shape).astype(np.float32)
    for x, y, saved in ((a, b, False), (f, b, True), (f, g, False), (a, g, (False, True))):
        fx, fy = _in_frame(x, 255 if x.dtype == np.uint8 else 1e30), _in_frame(y, 7 if y.dtype == np.uint8 else -1e30)
        host = metrics.psnr(m, fx, fy, size=(37, 50), as_saved=saved)
        assert np.all(np.isfinite(host)) and np.array_equal(_bits(host), _bits(metrics.psnr(m, dev(fx), dev(fy), size=(37, 50), as_saved=saved)))
        assert np.array_equal(_bits(host), _bits(metrics.psnr(m, x, y, as_saved=saved)))


# ---- 2. PSNR with a float operand -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _float_case(H, W):
    rng = np.random.default_rng(H * 1000 + W + 1)
    a = rng.uniform(-1.3, 1.3, (3, 3, H, W)).astype(np.float32)
    cases = []
    for k, sigma in enumerate(SIGMAS):
        b = (a + rng.normal(0, 2 * sigma, a.shape)).astype(np.float32)
        u = R.as_u8(np.clip(R.to_unit(a) + rng.normal(0, sigma, a.shape), 0, 1))
        cases += [(a, b, R.psnr(a, b)), (a, u, R.psnr(a, u))]
    return cases


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("H,W", PSNR_SIZES)
def test_psnr_float_against_float64(H, W, where):
    m, to = _model(), _to(where)
    for a, b, want in _float_case(H, W):
        got = metrics.psnr(m, to(a), to(b))
        got_f = metrics.psnr(m, to(_in_frame(a, np.nan)), to(_in_frame(b, 255 if b.dtype == np.uint8 else -1e30, extra=1)), size=(H, W))
        assert np.array_equal(_bits(got), _bits(got_f))
        sel = want <= 45.0
        if sel.any():
            err = float(np.abs(got - want)[sel].max())
            WORST["psnr_db"] = max(WORST["psnr_db"], err)
            print(f"[metrics] {where} psnr float {H}x{W}: {want} dB, error {err:.3g} dB (worst so far {WORST['psnr_db']:.3g})")
            assert err <= 1e-3, (got, want)
        assert np.all(np.isfinite(got) | (want > 45.0))
    f = _float_case(H, W)[0][0]
    assert np.all(np.isposinf(metrics.psnr(m, to(f), to(f.copy()))))


# ---- 3. MS-SSIM -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ms_cases(H, W):
    """[(a, b, as_saved, (msssim, components)) ...]: three noise levels, float32 / uint8 / as-saved operands, B = 2 distinct images."""
    p = R.picture(2, H, W)
    out = []
    for k, sigma in enumerate(SIGMAS):
        q = R.noisy(p, sigma, 10 * k + H + W)
        for a, b, saved in ((R.as_f32(p), R.as_f32(q), (False, False)), (R.as_u8(p), R.as_u8(q), (False, False)),
                            (R.as_u8(p), R.as_f32(q), (False, True))):
            ms, comp, pre = R.ms_ssim(a, b, *saved)
            # v^w is ill-conditioned at 0: a tolerance-tested case stays away from it (asserted on the restatement alone)
            assert np.all(np.abs(pre) >= 0.05), (H, W, sigma, pre)
            out.append((a, b, saved, ms, comp))
    return out


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("H,W", MS_SIZES)
def test_ms_ssim_against_float64(H, W, where):
    m, to = _model(), _to(where)
    for a, b, saved, want, want_comp in _ms_cases(H, W):
        got, comp = metrics.ms_ssim(m, to(a), to(b), as_saved=saved, return_components=True)
        assert got.shape == (2,) and comp.shape == (2, 5, 3)
        err = max(float(np.abs(got - want).max()), float(np.abs(comp - want_comp).max()))
        WORST["msssim"] = max(WORST["msssim"], err)
        print(f"[metrics] {where} ms-ssim {H}x{W} {a.dtype}/{b.dtype} saved {saved}: {want}, error {err:.3g} (worst so far {WORST['msssim']:.3g})")
        assert err <= 1e-5, (got, want)


@pytest.mark.parametrize("where", WHERE)
def test_ms_ssim_closed_forms(where):
    m, to = _model(), _to(where)
    p = R.picture(2, 176, 203)
    for x in (R.as_f32(p), R.as_u8(p)):
        got, comp = metrics.ms_ssim(m, to(x), to(x.copy()), return_components=True)
        assert np.abs(got - 1.0).max() <= 1e-5 and np.abs(comp - 1.0).max() <= 1e-5
    u = R.as_u8(p)
    got, comp = metrics.ms_ssim(m, to(u), to(255 - u), return_components=True)       # Y = 1 - X: negative cs means, relu, exactly 0
    assert np.all(got == 0.0) and np.all(comp[:, :4] == 0.0)
    f = R.as_f32(p)
    assert np.all(metrics.ms_ssim(m, to(f), to(-f)) == 0.0)
    a, b = 0.3, 0.8
    want = ((2 * a * b + R.C1) / (a * a + b * b + R.C1)) ** 0.1333                    # 0.945654839...
    for (H, W), w in (((176, 192), want), ((176, 203), None)):
        xa, xb = np.full((1, 3, H, W), a), np.full((1, 3, H, W), b)
        ref, ref_comp, _ = R.ms_ssim_unit(xa, xb)
        if w is not None:
            assert abs(ref[0] - w) < 1e-12
        else:
            assert abs(ref[0] - 0.9431) < 5e-5                                        # the counted zero pad darkens the border
        got, comp = metrics.ms_ssim(m, to(R.as_f32(xa)), to(R.as_f32(xb)), return_components=True)
        assert abs(got[0] - ref[0]) <= 1e-5 and np.abs(comp - ref_comp).max() <= 1e-5, (got, ref)


# ---- 4. the window is the window ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", WHERE)
def test_nothing_outside_the_window_counts(where):
    m, to = _model(), _to(where)
    H, W = 176, 203
    p = R.picture(2, H, W)
    q = R.noisy(p, 0.05, 3)
    for a, b, fa, fb, saved in ((R.as_f32(p), R.as_f32(q), np.nan, 1e30, False), (R.as_f32(p), R.as_u8(q), 1e30, 255, True),
                                (R.as_u8(p), R.as_f32(q), 255, np.nan, False)):
        ps, ms = metrics.distortion(m, to(a), to(b), as_saved=saved)
        ms2, comp = metrics.ms_ssim(m, to(a), to(b), as_saved=saved, return_components=True)
        assert np.array_equal(_bits(ms), _bits(ms2))
        for extra in (0, 5):
            fps, fms = metrics.distortion(m, to(_in_frame(a, fa, extra=extra)), to(_in_frame(b, fb)), size=(H, W), as_saved=saved)
            _, fcomp = metrics.ms_ssim(m, to(_in_frame(a, fa)), to(_in_frame(b, fb, extra=extra)), size=(H, W), as_saved=saved, return_components=True)
            assert np.array_equal(_bits(fps), _bits(ps)) and np.array_equal(_bits(fms), _bits(ms)) and np.array_equal(_bits(fcomp), _bits(comp))
        assert np.all(np.isfinite(ps)) and np.all(np.isfinite(ms))


# ---- 5. reproducibility ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", WHERE)
def test_results_depend_on_neither_the_run_nor_the_batch(where):
    m, to = _model(), _to(where)
    for H, W in ((176, 203), (333, 500)):
        p = R.picture(5, H, W)
        a, b = R.as_f32(p), R.as_f32(R.noisy(p, 0.05, 11))
        u = R.as_u8(R.noisy(p, 0.05, 12))
        for x, y in ((a, b), (a, u), (R.as_u8(p), u)):
            ps, ms = metrics.distortion(m, to(x), to(y))
            ps2, ms2 = metrics.distortion(m, to(x), to(y))
            assert np.array_equal(_bits(ps), _bits(ps2)) and np.array_equal(_bits(ms), _bits(ms2))
            for i in (0, 3, 4):
                p1, m1 = metrics.distortion(m, to(x[i:i + 1]), to(y[i:i + 1]))
                assert _bits(p1)[0] == _bits(ps)[i] and _bits(m1)[0] == _bits(ms)[i], (H, W, i)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------

def test_entry_point_refusals():
    m = _model()
    h, L = m._handle(), _lib.lib()
    a = np.zeros((1, 3, 200, 200), np.float32)
    u = np.zeros((1, 3, 200, 200), np.uint8)
    out = (ctypes.c_double * 32)()
    view = lambda t, kind=None, Hf=200, Wf=200, saved=0: _lib.ImageView(t.ctypes.data, (1 if t.dtype == np.uint8 else 0) if kind is None else kind, Hf, Wf, saved)   # noqa: E731

    def call(va, vb, B=1, H=200, W=200, what=3, ps=out, ms=out, comp=None):
        rc = L.cdc_distortion(h, ctypes.byref(va), ctypes.byref(vb), B, H, W, what, ps, ms, comp, 0, None)
        return rc, (L.cdc_last_error(h) or b"").decode()

    assert call(view(a), view(u))[0] == 0
    bad = [dict(B=0), dict(H=0), dict(W=-1),                                         # B, H, W < 1
           dict(H=201), dict(W=201),                                                  # Hf < H, Wf < W
           dict(what=0), dict(what=1, ps=None), dict(what=2, ms=None), dict(what=3, ms=None),
           dict(H=160), dict(W=160, what=2)]                                          # MS-SSIM with min(H, W) <= 160
    for kw in bad:
        rc, msg = call(view(a), view(u), **kw)
        assert rc == -1 and msg, (kw, rc, msg)
    for va, vb in ((view(a, kind=2), view(u)), (view(a), view(u, kind=-1)),           # an unknown element kind
                   (view(a), view(u, saved=1)),                                       # as_saved on a uint8 operand
                   (view(a, Hf=199), view(u)), (view(a), view(u, Wf=10))):
        rc, msg = call(va, vb)
        assert rc == -1 and msg, (rc, msg)
    assert call(view(a), view(u), H=160, W=100, what=1)[0] == 0                       # PSNR has no lower limit
    with pytest.raises(ValueError):
        metrics.ms_ssim(m, a[:, :, :160], a[:, :, :160])


# ---- 7. evaluate() --------------------------------------------------------------------------------------------------------------------

def _small(tag):
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))[tag]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0 if tag == "x" else 0.2))
    man = [(k, tuple(v)) for k, v in meta["comp_manifest"]]
    if tag == "x":
        comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
        comp.load_state_dict(synth.unet_state_dict(man, seed=meta["seed"]))
        return cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine"), {}
    comp = cdc.BigCompressor(**meta["comp_kwargs"])
    comp.load_state_dict(synth.unet_state_dict(man, seed=meta["seed"]))
    return cdc.GaussianDiffusionEps(un, comp, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear"), {"sample_mode": "ddim"}


@pytest.mark.parametrize("tag", ["x", "eps"])
def test_evaluate_is_compress_plus_the_metrics(tag):
    diff, kw = _small(tag)
    un = diff.denoise_fn
    u8 = R.as_u8(R.picture(2, 176, 203))
    f32 = R.as_f32(R.picture(2, 176, 203, seed=1))
    for images in (u8, f32):
        rec, bpp = diff.compress(images, sample_steps=2, bpp_return_mean=False, **kw)
        ev = diff.evaluate(images, sample_steps=2, **kw)
        assert sorted(ev) == ["bpp", "ms_ssim", "psnr", "reconstruction"]
        assert ev["reconstruction"].shape == (2, 3, 176, 203) and np.array_equal(ev["reconstruction"].view(np.int32), rec.view(np.int32))
        assert np.array_equal(np.asarray(ev["bpp"]), np.asarray(bpp)) and np.asarray(ev["bpp"]).shape == (2,)
        assert np.array_equal(_bits(ev["psnr"]), _bits(metrics.psnr(un, rec, images, as_saved=True)))
        assert np.array_equal(_bits(ev["ms_ssim"]), _bits(metrics.ms_ssim(un, rec, images, as_saved=True)))
        assert ev["psnr"].shape == (2,) and np.all(np.isfinite(ev["psnr"])) and np.all((ev["ms_ssim"] >= 0) & (ev["ms_ssim"] <= 1))
        raw = diff.evaluate(images, sample_steps=2, as_saved=False, **kw)
        assert np.array_equal(_bits(raw["psnr"]), _bits(metrics.psnr(un, rec, images)))
    small = diff.evaluate(u8[:, :, :100, :120], sample_steps=2, **kw)
    assert small["ms_ssim"] is None and small["psnr"].shape == (2,) and small["reconstruction"].shape == (2, 3, 100, 120)


# ---- 8. the example script ------------------------------------------------------------------------------------------------------------

def test_example_script_prints_the_metrics_only_when_asked(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(R.as_u8(R.picture(1, 176, 203))[0].transpose(1, 2, 0)).save(src / "a.png")
    outs = []
    for flags in ([], ["--metrics"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                            "--n_denoise_step", "2", "--img_dir", str(src), "--out_dir", str(tmp_path / ("out" + str(len(flags))))] + flags,
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, CDC_SYNTHETIC_INIT="1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout.splitlines())
    plain, with_metrics = outs
    assert len(plain) == 2 and plain[0] == "image: a.png" and plain[1].startswith("bpp:")        # today's output
    assert with_metrics[:2] == plain and len(with_metrics) == 4
    assert with_metrics[2].startswith("psnr: ") and with_metrics[3].startswith("ms_ssim: ")
    ps, ms = float(with_metrics[2].split()[1]), float(with_metrics[3].split()[1])
    got = np.asarray(Image.open(tmp_path / "out1" / "a.png").convert("RGB")).transpose(2, 0, 1)[None]
    want = np.asarray(Image.open(src / "a.png").convert("RGB")).transpose(2, 0, 1)[None]
    assert abs(ps - R.psnr(got, want)[0]) <= 1e-9 * ps and abs(ms - R.ms_ssim(got, want)[0][0]) <= 1e-5
