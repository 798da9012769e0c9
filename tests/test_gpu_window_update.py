"""The update of one Picard sweep alone (cdc_op_window_update; include/cdc_hip.h: THE SWEEP) on the MI355X, against the float64
recurrence of tests/picard_ref.py over tests/sampler_ref.py's DDIM update.

The bound of row m (the new guess of y_{w+m+1}), element by element: the sum over the rows l <= m of sampler_ref's bound of row l's
update -- at most (m + 1) times the largest of them -- plus 2 (m + 1) 2^-24 ymax for the add and the subtract of every row, ymax the
largest magnitude the recurrence forms (picard_ref states it; tests/test_picard_host.py checks that the float32 restatement stays inside).

The residuals: float64 sums of the float32 squares of the float32 differences of the returned values, to 1e-12 relative -- the
summation order is the only freedom -- and the same bits in two runs.

Two handles as in test_gpu_ddim_update.py (5-step schedules: the x tree with the tables of pred_mode "v", the eps tree); the U-Net
never runs.  Frames: 3 x 5 x 7 (H W % 4 != 0: the element path, the last quad of an image partial) and 3 x 64 x 64 (the 16-byte path,
12 workgroups per image)."""
import ctypes

import numpy as np
import pytest

import picard_ref as PR
import sampler_ref as R
from cdc_compression_amd import _lib
from test_gpu_ddim_update import handles, _of, _randn_dev          # noqa: F401  (handles: the module fixture of the two trees)

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
F64P = ctypes.POINTER(ctypes.c_double)
SEEDS = [(9 << 32) + 5, 2 ** 64 - 3]
ETA = 0.7


def _op(un, fx, y, w, eta, pred, clip, seeds=None):
    """cdc_op_window_update on host arrays -> (y after the sweep, residuals [B][p])."""
    L, h = _lib.lib(), un._handle()
    B, p, C, H, W = fx.shape
    y = y.copy()
    res = np.full((B, p), np.nan, np.float64)
    sd = None if seeds is None else np.ascontiguousarray(seeds[:B], dtype=np.uint64)
    _lib.check(h, L.cdc_op_window_update(h, fx.ctypes.data, y.ctypes.data, None if sd is None else sd.ctypes.data_as(U64P), eta, w, p,
                                         res.ctypes.data_as(F64P), B, C, H, W, pred, clip, _lib.CDC_MEM_HOST, None))
    return y, res


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 64, 64)])
@pytest.mark.parametrize("p", [2, 5])
def test_update_against_float64(handles, shape, p):
    worst = 0.0
    for B in (1, 2):
        fx, y = PR.inputs(B, p, shape)
        for pred in (R.PRED_X, R.PRED_NOISE, R.PRED_V):
            un, s = _of(handles, pred)
            for w in (0, s.steps - p + 1 if p < s.steps else 2):                 # the second base leaves a dead last row (or more)
                live = PR.live_rows(w, p, s.steps)
                assert live == p if w == 0 else live < p
                for eta in (0.0, ETA):
                    seeds = SEEDS if eta else None
                    noise = None if not eta else [_randn_dev(un, SEEDS[:B], (B,) + shape, s.steps - 1 - (w + m) + 1) for m in range(live)]
                    for clip in R.CLIPS:
                        got, res = _op(un, fx, y, w, eta, pred, clip, seeds)
                        ref, bound = PR.sweep_f64(s, w, fx, y, noise, eta, pred, clip)
                        err = np.abs(got[:, 1:live + 1].astype(np.float64) - ref)
                        ratio = float((err / bound).max())
                        assert np.all(err <= bound), (B, pred, w, eta, clip, ratio)
                        worst = max(worst, ratio)
                        # what the sweep does not own stays: y_w, and the states behind a dead row
                        np.testing.assert_array_equal(got[:, 0], y[:, 0])
                        np.testing.assert_array_equal(got[:, live + 1:], y[:, live + 1:])
                        want = PR.residuals(got[:, 1:live + 1], y)
                        np.testing.assert_allclose(res[:, :live], want, rtol=1e-12, atol=0)
                        assert np.all(res[:, live:] == 0)
                        got2, res2 = _op(un, fx, y, w, eta, pred, clip, seeds)
                        np.testing.assert_array_equal(got, got2)
                        assert res.tobytes() == res2.tobytes()
    assert worst > 0
    print(f"{shape} p={p}: worst error / bound = {worst:.3f}")


def test_a_converged_window_returns_the_sequential_bits_and_zero_residuals(handles):
    """The guesses ARE the chain: every row is Phi(y) + 0 -- the bits of cdc_op_ddim_update -- and every residual is exactly 0."""
    from test_gpu_ddim_update import _op as ddim_op
    B, p, shape = 2, 5, (3, 64, 64)
    fx, y = PR.inputs(B, p, shape)
    un, s = _of(handles, R.PRED_V)
    for eta, seeds in ((0.0, None), (ETA, SEEDS)):
        chain = y.copy()
        for m in range(p):
            chain[:, m + 1] = ddim_op(un, s.steps - 1 - m, fx[:, m].copy(), chain[:, m].copy(), None, eta, R.PRED_V, R.CLIP_ALL, seeds=seeds)
        got, res = _op(un, fx, chain, 0, eta, R.PRED_V, R.CLIP_ALL, seeds)
        np.testing.assert_array_equal(got, chain)
        assert np.all(res == 0)


def test_device_tensors_and_a_nonfinite_model_output(handles):
    """Device memory on the caller's stream; a NaN in the model output goes where the update puts it and nowhere else."""
    import torch
    dev = torch.device("cuda", 0)
    B, p, shape = 2, 5, (3, 64, 64)
    fx, y = PR.inputs(B, p, shape)
    un, s = _of(handles, R.PRED_X)
    want, wres = _op(un, fx, y, 0, 0.0, R.PRED_X, R.CLIP_ALL)
    L, h = _lib.lib(), un._handle()
    st = torch.cuda.Stream(device=dev)
    res = np.zeros((B, p), np.float64)
    with torch.cuda.stream(st):
        dfx, dy = torch.from_numpy(fx).to(dev) * 1.0, torch.from_numpy(y).to(dev) * 1.0
        _lib.check(h, L.cdc_op_window_update(h, dfx.data_ptr(), dy.data_ptr(), None, 0.0, 0, p, res.ctypes.data_as(F64P), B, *shape, R.PRED_X,
                                             R.CLIP_ALL, _lib.CDC_MEM_DEVICE, ctypes.c_void_p(st.cuda_stream)))
        got = (dy * 1.0).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert res.tobytes() == wres.tobytes()
    bad = fx.copy()
    bad[1, 2, 0, 3, 4] = np.nan
    got, res = _op(un, bad, y, 0, 0.0, R.PRED_X, R.CLIP_NONE)
    hit = np.isnan(got)
    assert hit[1, 3:, 0, 3, 4].all() and hit.sum() == p - 2 and np.isnan(res[1, 2:]).all() and np.isfinite(res[0]).all()


def test_refusals(handles):
    un, s = _of(handles, R.PRED_X)
    L, h = _lib.lib(), un._handle()
    fx, y = PR.inputs(1, 2, (3, 5, 7))
    res = np.zeros((1, 2), np.float64)

    def call(w=0, p=2, eta=0.0, seeds=None, B=1, fxp=fx.ctypes.data):
        rc = L.cdc_op_window_update(h, fxp, y.ctypes.data, seeds, eta, w, p, res.ctypes.data_as(F64P), B, 3, 5, 7, R.PRED_X, R.CLIP_ALL,
                                    _lib.CDC_MEM_HOST, None)
        return rc, L.cdc_last_error(h).decode()

    for kw, msg in ((dict(p=1), "window 1"), (dict(p=s.steps + 1), "window"), (dict(w=s.steps), "window base"), (dict(w=-1), "window base"),
                    (dict(eta=0.5), "needs seeds"), (dict(B=0), "elements"), (dict(fxp=None), "null")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    assert call()[0] == 0
