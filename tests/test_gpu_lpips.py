"""cdc_lpips on the GPU (csrc/lpips_kernels.hip + the VGG16 program of csrc/cdc_planner.hip) against the float64 restatement of
tests/lpips_ref.py, which tests/test_lpips_host.py checks on the CPU.  Synthetic weights (synth.lpips_vgg_state_dict), operands a
smoothed random picture against the picture plus Gaussian noise of sigma 0.02 ... 0.3.  A reference is computed once per case and
shared.  Bound: the project's forward bound, 1e-5 relative (Parity bounds), on each of the five layer values and
on the sum, per image; plain float32 arithmetic sits at <= 1.6e-6 / 1.2e-7 on these cases (test_lpips_host.py).  Every observed
figure is printed and, with CDC_TEST_OBS=<file>, appended there.  Worst seen on an MI355X (profiles/lpips.md): 6.0e-6 on a layer
value (16 x 16, the 1 x 1 map of relu5_3), 3.5e-7 on the sum."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
import lpips_ref as LR
import metrics_ref as R
from cdc_compression_amd import _lib, metrics, synth
from cdc_compression_amd.ops import Ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOUND = 1e-5


def _obs(what, err):
    print(f"[lpips] {what}: {err:.3g}")
    obs = os.environ.get("CDC_TEST_OBS")
    if obs:
        with open(obs, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "what": what, "relerr": err}) + "\n")
    return err


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.lpips_vgg_state_dict(seed=0)


@functools.lru_cache(maxsize=None)
def _model():
    return cdc.LpipsVGG().load_state_dict(_sd())


def _in_frame(win, fill, Hf, Wf):
    B, C, H, W = win.shape
    f = np.full((B, C, Hf, Wf), fill, win.dtype)
    f[:, :, :H, :W] = win
    return f


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. single layers first: a planner gap fails under its own name --------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(33, 47), (16, 16)])
@pytest.mark.parametrize("Cin,Cout", [(3, 64), (64, 64), (256, 512), (512, 512)])
def test_conv_bias_relu_of_the_vgg_widths(Cin, Cout, H, W):
    import torch
    x = synth.normal("lx", (1, Cin, H, W), 5)
    w = synth.normal("lw", (Cout, Cin, 3, 3), 5, float(np.sqrt(2.0 / (Cin * 9))))
    b = synth.normal("lb", (Cout,), 5, 0.01, 0.05)
    ref = torch.relu(torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)).numpy()
    got = Ops(0).conv2d(x, w, b, 1, 1, relu=True)
    assert got.shape == ref.shape and np.all(got >= 0)
    err = _obs(f"conv+relu {Cin}->{Cout} {H}x{W}", float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
    assert err <= BOUND


# ---- 2. parity against float64 ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _plain_case(B, H, W):
    p, q = LR.operands(B, H, W)
    a, b = R.as_f32(p), R.as_f32(q)
    return a, b, LR.lpips_torch(_sd(), a, b)


def _check(what, got, lay, want, want_lay):
    assert got.dtype == np.float64 and got.shape == want.shape and lay.shape == want_lay.shape
    e_lay = _obs(f"{what} layers", float(np.abs((lay - want_lay) / want_lay).max()))
    e_sum = _obs(f"{what} sum", float(np.abs((got - want) / want).max()))
    assert e_lay <= BOUND and e_sum <= BOUND, (got, want, lay, want_lay)
    assert np.array_equal(got, lay.sum(1))                     # the result is the sum of the five layer values, in that order


# 16 x 16: the last map is 1 x 1;  33 x 47: an odd side at every level, element accesses;  64 x 64: the 16-byte forms;
# 200 x 136: more than one partial per image, the 16^2 / 8^2-pixel levels with >= 100 pixels
@pytest.mark.parametrize("B,H,W", [(3, 16, 16), (3, 33, 47), (3, 64, 64), (1, 200, 136)])
def test_parity_against_float64(B, H, W):
    a, b, (want, want_lay) = _plain_case(B, H, W)
    got, lay = _model()(a, b, return_layers=True)
    _check(f"{H}x{W}", got, lay, want, want_lay)


def test_parity_of_a_framed_window_with_mixed_element_kinds():
    """A 96 x 80 window inside a 128 x 128 float32 frame, measured as saved, against a 96 x 80 uint8 image."""
    p, q = LR.operands(3, 96, 80)
    a, b = R.as_f32(q), R.as_u8(p)
    want, want_lay = LR.lpips_torch(_sd(), a, b, saved_a=True)
    fa = _in_frame(a, 1e30, 128, 128)
    got, lay = _model()(fa, b, size=(96, 80), as_saved=(True, False), return_layers=True)
    _check("96x80 in 128x128 saved/u8", got, lay, want, want_lay)
    got2 = metrics.lpips(_model(), b, fa, size=(96, 80), as_saved=True)       # as_saved on a uint8 operand means nothing
    assert np.abs((got2 - want) / want).max() <= BOUND
    want_raw, _ = LR.lpips_torch(_sd(), a, b)
    assert np.abs((_model()(fa, b, size=(96, 80)) - want_raw) / want_raw).max() <= BOUND


def test_identical_operands_give_exactly_zero():
    a = _plain_case(3, 33, 47)[0]
    got, lay = _model()(a, a.copy(), return_layers=True)
    assert np.all(got == 0.0) and np.all(lay == 0.0)


# ---- 3. a result depends on nothing but its pair ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(33, 47), (64, 64)])
def test_batch_chunk_and_run_independence_bitwise(H, W, monkeypatch):
    p, q = LR.operands(5, H, W, seed=1)
    a, b = R.as_f32(p), R.as_f32(q)
    m = _model()
    got, lay = m(a, b, return_layers=True)
    again, lay_again = m(a, b, return_layers=True)
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(_bits(lay), _bits(lay_again))
    for i in (0, 2, 4):
        one, lay_one = m(a[i:i + 1], b[i:i + 1], return_layers=True)
        assert _bits(one)[0] == _bits(got)[i] and np.array_equal(_bits(lay_one)[0], _bits(lay)[i]), (H, W, i)
    # a chunk budget of 8 MB holds two pairs at 33 x 47 and one at 64 x 64: the batch of five is split
    monkeypatch.setenv("CDC_LPIPS_BUDGET_MB", "8")
    split, lay_split = m(a, b, return_layers=True)
    assert np.array_equal(_bits(got), _bits(split)) and np.array_equal(_bits(lay), _bits(lay_split))


def test_framed_and_cropped_operands_and_nothing_outside_the_window():
    a, b, _ = _plain_case(3, 33, 47)
    m = _model()
    got, lay = m(a, b, return_layers=True)
    for fill_a, fill_b, Hf, Wf in ((np.nan, 1e30, 64, 64), (-np.inf, np.nan, 40, 51)):
        f, fl = m(_in_frame(a, fill_a, Hf, Wf), _in_frame(b, fill_b, 33, 48), size=(33, 47), return_layers=True)
        assert np.array_equal(_bits(f), _bits(got)) and np.array_equal(_bits(fl), _bits(lay))
    assert np.all(np.isfinite(got))


def test_operand_places_give_the_same_bits():
    import torch
    p, q = LR.operands(2, 40, 48)
    a, b = R.as_f32(p), R.as_u8(q)
    m = _model()
    want = m(a, b)
    for x, y in ((_cuda(a), _cuda(b)), (torch.from_numpy(a), torch.from_numpy(b)), (_cuda(a), b), (a, _cuda(b))):
        got = m(x, y)
        assert isinstance(got, np.ndarray) and np.array_equal(_bits(got), _bits(want))


# ---- 4. the range guard ----------------------------------------------------------------------------------------------------------------

def test_range_guard_repeats_a_hostile_network_in_the_full_range_arithmetic():
    sd = dict(_sd())
    for k in ("net.slice1.0.weight", "net.slice1.0.bias"):
        sd[k] = sd[k] * np.float32(1e5)                           # activations of 1e5 ... 1e6 from the first layer on: beyond fp16
    m = cdc.LpipsVGG().load_state_dict(sd)
    p, q = LR.operands(2, 32, 32)                                  # (sides of 4 k: the 16-bit-operand kernels run, not the fp32 MFMA one)
    a, b = R.as_f32(p), R.as_f32(q)
    want, want_lay = LR.lpips_torch(sd, a, b)
    assert m.status()["range_faults"] == 0
    got, lay = m(a, b, return_layers=True)
    st = m.status()
    assert st["range_faults"] == 1 and st["nonfinite_results"] == 0 and st["arith"] == 0, st
    _check("32x32 slice1.0 x 1e5", got, lay, want, want_lay)       # the normalisation absorbs the scale
    got2 = m(a, b)
    assert np.array_equal(_bits(got), _bits(got2)) and m.status()["range_faults"] == 1


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------

def _small_x(with_lpips):
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))["x"]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
    diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    sd = {"denoise_fn." + k: v for k, v in synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0).items()}
    sd.update({"context_fn." + k: v for k, v in synth.unet_state_dict([(k, tuple(v)) for k, v in meta["comp_manifest"]], seed=meta["seed"]).items()})
    if with_lpips:
        sd.update(synth.lpips_vgg_state_dict(seed=0, prefix="loss_fn_vgg.", with_duplicates=True))
    return diff.load_state_dict(sd)


def test_evaluate_reports_lpips_when_the_state_dict_carried_the_network():
    images = R.as_u8(LR.operands(2, 50, 44)[0])
    plain = _small_x(False).evaluate(images, sample_steps=2)
    assert sorted(plain) == ["bpp", "ms_ssim", "psnr", "reconstruction"]
    diff = _small_x(True)
    ev = diff.evaluate(images, sample_steps=2)
    assert sorted(ev) == ["bpp", "lpips", "ms_ssim", "psnr", "reconstruction"]
    assert ev["lpips"].shape == (2,) and ev["lpips"].dtype == np.float64 and np.all(np.isfinite(ev["lpips"])) and np.all(ev["lpips"] > 0)
    assert np.array_equal(_bits(ev["lpips"]), _bits(metrics.lpips(diff.loss_fn_vgg, ev["reconstruction"], images, as_saved=True)))
    # the network on board changes nothing else
    assert np.array_equal(ev["reconstruction"].view(np.int32), plain["reconstruction"].view(np.int32))
    assert np.array_equal(_bits(ev["psnr"]), _bits(plain["psnr"])) and np.array_equal(np.asarray(ev["bpp"]), np.asarray(plain["bpp"]))
    want = LR.lpips_torch(_sd(), ev["reconstruction"], images, saved_a=True)[0]
    assert np.abs((ev["lpips"] - want) / want).max() <= BOUND


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------

def test_entry_point_refusals():
    L = _lib.lib()
    a = np.zeros((1, 3, 32, 32), np.float32)
    u = np.zeros((1, 3, 32, 32), np.uint8)
    out = (ctypes.c_double * 8)()
    view = lambda t, Hf=32, Wf=32, saved=0, kind=None: _lib.ImageView(t.ctypes.data, (1 if t.dtype == np.uint8 else 0) if kind is None else kind, Hf, Wf, saved)   # noqa: E731

    def call(h, va, vb, B=1, H=32, W=32, res=out, lay=None):
        rc = L.cdc_lpips(h, ctypes.byref(va), ctypes.byref(vb), B, H, W, res, lay, 0, None)
        return rc, (L.cdc_last_error(h) or b"").decode()

    h = _model()._ready()
    assert call(h, view(a), view(u))[0] == 0
    for kw in (dict(H=15), dict(W=15), dict(B=0), dict(H=33), dict(W=33), dict(res=None)):
        rc, msg = call(h, view(a), view(u), **kw)
        assert rc == -1 and msg, (kw, rc, msg)
    for va, vb in ((view(a, Hf=31), view(u)), (view(a), view(u, saved=1)), (view(a, kind=2), view(u))):
        rc, msg = call(h, va, vb)
        assert rc == -1 and msg, (rc, msg)
    with pytest.raises(_lib.CdcError, match="H, W >= 16"):
        _lib.check(h, call(h, view(a), view(u), H=15)[0])
    unet = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    hu = unet._handle()
    with pytest.raises(_lib.CdcError, match="not an LPIPS-VGG network"):
        _lib.check(hu, call(hu, view(a), view(u))[0])
    fresh = cdc.LpipsVGG().load_state_dict(_sd())                  # parameters loaded, not finalized
    hf = fresh._handle()
    with pytest.raises(_lib.CdcError, match="not finalized"):
        _lib.check(hf, call(hf, view(a), view(u))[0])
    with pytest.raises(ValueError, match="H, W >= 16"):
        _model()(a[:, :, :15], a[:, :, :15])
