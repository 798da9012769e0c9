"""Distortion metrics, host side (no GPU): the float64 restatement the GPU tests compare against (tests/metrics_ref.py) is itself
checked -- against a structurally different evaluation (torch float64: grouped conv2d, avg_pool2d with padding) and against closed
forms that pin the pooling convention -- and the Python layer's argument rules and the library's exports are checked."""
import numpy as np
import pytest

import metrics_ref as R
from cdc_compression_amd import _lib, metrics

SIZES = [(161, 161), (162, 161), (176, 203), (333, 500)]
SIGMAS = [0.01, 0.05, 0.2]


def _torch_ms_ssim(x, y):
    """pytorch-msssim 0.2.1's structure in float64: grouped F.conv2d per axis, F.avg_pool2d(kernel 2, padding = side % 2)."""
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    g = torch.from_numpy(R.gauss())
    wr, wc = g.view(1, 1, 11, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, 11).repeat(3, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, wr, groups=3), wc, groups=3)     # noqa: E731
    vals = []
    for l in range(5):
        m1, m2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - m1 * m1, filt(Y * Y) - m2 * m2, filt(X * Y) - m1 * m2
        cs = (2 * s12 + R.C2) / (s1 + s2 + R.C2)
        ss = (2 * m1 * m2 + R.C1) / (m1 * m1 + m2 * m2 + R.C1) * cs
        vals.append(torch.relu((cs if l < 4 else ss).flatten(2).mean(-1)))
        if l < 4:
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    v = torch.stack(vals, 0)                                                # [5, B, 3]
    w = torch.tensor(R.WEIGHTS, dtype=torch.float64).view(-1, 1, 1)
    return torch.prod(v ** w, 0).mean(1).numpy(), v.permute(1, 0, 2).numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_agrees_with_torch_float64(H, W):
    p = R.picture(2, H, W)
    for k, sigma in enumerate(SIGMAS):
        q = R.noisy(p, sigma, 100 + k)
        for x, y in ((p, q), (R.to_unit(R.as_u8(p)), R.to_unit(R.as_f32(q)))):
            ms, comp, _ = R.ms_ssim_unit(x, y)
            tms, tcomp = _torch_ms_ssim(x, y)
            err = max(float(np.abs(ms - tms).max()), float(np.abs(comp - tcomp).max()))
            print(f"[metrics] {H}x{W} sigma {sigma}: ms-ssim {ms}, restatement vs torch float64 {err:.3g}")
            assert err <= 1e-8


def test_noise_levels_give_the_expected_figures():
    p = R.picture(2, 176, 203)
    for sigma, lo, hi, db in ((0.01, 0.99, 0.999, 40.0), (0.05, 0.9, 0.97, 26.0), (0.2, 0.6, 0.75, 14.4)):
        q = R.noisy(p, sigma, 7)
        ms = R.ms_ssim_unit(p, q)[0]
        ps = R.psnr(R.as_f32(p), R.as_f32(q))
        assert (ms > lo).all() and (ms < hi).all(), (sigma, ms)
        assert np.abs(ps - db).max() < 1.0, (sigma, ps)


def test_closed_forms():
    p = R.picture(1, 176, 203)
    assert R.ms_ssim_unit(p, p.copy())[0][0] == 1.0
    ms, comp, pre = R.ms_ssim_unit(p, 1.0 - p)
    assert ms[0] == 0.0 and (pre[:, :4] < -0.05).all()                      # clearly negative cs means: relu clamps them
    a, b = 0.3, 0.8
    want = ((2 * a * b + R.C1) / (a * a + b * b + R.C1)) ** 0.1333
    assert abs(want - 0.945654839) < 1e-9
    # every side stays even through four poolings: the constants survive, cs = 1 at every scale
    ms = R.ms_ssim_unit(np.full((1, 3, 176, 192), a), np.full((1, 3, 176, 192), b))[0][0]
    assert abs(ms - want) < 1e-12
    # an odd side: the counted zero pad darkens the border of every pooled plane
    ms = R.ms_ssim_unit(np.full((1, 3, 176, 203), a), np.full((1, 3, 176, 203), b))[0][0]
    assert abs(ms - 0.9431) < 5e-5, ms
    tms = _torch_ms_ssim(np.full((1, 3, 176, 203), a), np.full((1, 3, 176, 203), b))[0][0]
    assert abs(ms - tms) < 1e-10


def test_pyramid_sizes():
    assert [s[0] for s in R.pyramid_sizes(161, 161)] == [161, 81, 41, 21, 11]
    assert R.pyramid_sizes(333, 500) == [(333, 500), (167, 250), (84, 125), (42, 63), (21, 32)]
    x = np.zeros((1, 3, 333, 500))
    for want in R.pyramid_sizes(333, 500)[1:]:
        x = R._pool(x)
        assert x.shape[2:] == want


def test_psnr_restatement():
    a = np.array([[[[0, 255]], [[10, 10]], [[3, 4]]]], np.uint8)            # [1, 3, 1, 2]
    b = np.array([[[[0, 0]], [[10, 11]], [[3, 4]]]], np.uint8)
    assert R.psnr(a, b)[0] == 10.0 * np.log10(1.0 / ((255 ** 2 + 1) / (65025 * 6)))
    assert np.isinf(R.psnr(a, a.copy())[0])
    f = np.array([1.3, -1.3, 0.0, 0.999], np.float32).reshape(1, 1, 2, 2).repeat(3, 1)
    assert list(R.saved_u8(f)[0, 0].ravel()) == [255, 0, 128, 255]
    assert np.isinf(R.psnr(f, R.saved_u8(f), saved_a=True)[0])


def test_new_names_are_exported():
    assert "cdc_distortion" in _lib.EXPORTS
    assert (_lib.CDC_METRIC_PSNR, _lib.CDC_METRIC_MSSSIM) == (1, 2)
    assert [f[0] for f in _lib.ImageView._fields_] == ["data", "elem_kind", "Hf", "Wf", "as_saved"]


class _NoModel:
    """Stands where a model goes: touching the library is the failure."""
    device_index = 0

    def _handle(self):
        raise AssertionError("an argument error must be raised before the library is touched")


def test_argument_errors_need_no_gpu():
    m = _NoModel()
    f = lambda *s: np.zeros(s, np.float32)                                  # noqa: E731
    for fn in (metrics.psnr, metrics.ms_ssim):
        with pytest.raises(ValueError, match="images"):
            fn(m, f(2, 3, 200, 200), f(3, 3, 200, 200))                     # mismatched batch
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            fn(m, f(2, 1, 200, 200), f(2, 1, 200, 200))                     # not 3 channels
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            fn(m, f(3, 200, 200), f(3, 200, 200))
        with pytest.raises(ValueError, match="larger than operand b"):
            fn(m, f(2, 3, 256, 256), f(2, 3, 200, 256), size=(201, 256))    # a window larger than an operand
        with pytest.raises(ValueError, match="size="):
            fn(m, f(2, 3, 256, 256), f(2, 3, 200, 200))                     # differing frames need the window
        with pytest.raises(ValueError, match="float32 or uint8"):
            fn(m, np.zeros((2, 3, 200, 200), np.float64), f(2, 3, 200, 200))
    with pytest.raises(ValueError, match="160"):
        metrics.ms_ssim(m, f(1, 3, 160, 300), f(1, 3, 160, 300))
    with pytest.raises(ValueError, match="160"):
        metrics.ms_ssim(m, f(1, 3, 256, 256), f(1, 3, 256, 256), size=(200, 160))


def test_ms_ssim_db():
    assert metrics.ms_ssim_db(0.9) == pytest.approx(10.0)
    assert np.allclose(metrics.ms_ssim_db(np.array([0.0, 0.99])), [0.0, 20.0])
    assert metrics.ms_ssim_db(1.0) == np.inf
