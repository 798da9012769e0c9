"""Parallel-in-time decode without a GPU (cdc_compression_amd/picard.py; include/cdc_hip.h: cdc_decode_parallel): the two forms of a
sweep on a float64 toy chain, the sweep loop at the two ends of the tolerance, the stride rule on hand-made residual tables, the
window bookkeeping, the float32 restatement of the update kernel against the float64 bound it is tested with on the GPU, and the
argument rules of the Python mirror and of the library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import cdc_compression_amd as cdc
import picard_ref as PR
import sampler_ref as R
from cdc_compression_amd import _lib, picard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = 12, 4


def toy_chain():
    """Phi_j(y) = a_j y + b_j tanh(y), 12 steps, on a vector of 7 float64 values."""
    rng = np.random.default_rng(3)
    a, b = rng.uniform(0.6, 1.1, N), rng.uniform(-0.5, 0.5, N)
    phis = [lambda y, a=a[j], b=b[j]: a * y + b * np.tanh(y) for j in range(N)]
    return phis, rng.standard_normal(7)


def sequential(phis, y0):
    y = y0
    for f in phis:
        y = f(y)
    return y


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
def test_recurrence_equals_the_prefix_sum_form():
    phis, y0 = toy_chain()
    rng = np.random.default_rng(4)
    for w in (0, 3, 9, 11):                                  # 9, 11: dead rows at the end of the schedule
        ys = [y0 + 0.3 * rng.standard_normal(7) for _ in range(N + 1)]
        new, res = picard.sweep(phis, ys, w, P)
        pre = picard.sweep_prefix(phis, ys, w, P)
        assert len(new) == len(pre) == len(res) == picard.live_rows(w, P, N) == min(P, N - w)
        for a, b in zip(new, pre):
            assert float(np.abs(a - b).max()) <= 1e-14
        for m, r in enumerate(res):
            assert r == pytest.approx(float(((new[m] - ys[w + m + 1]) ** 2).sum()), rel=1e-15)
        np.testing.assert_array_equal(new[0], phis[w](ys[w]))            # row 0: Phi(y_w) + 0


def test_tol_zero_is_the_sequential_chain_exactly():
    phis, y0 = toy_chain()
    got, strides = picard.solve(phis, y0, P, 0.0)
    np.testing.assert_array_equal(got, sequential(phis, y0))
    assert len(strides) <= N and sum(strides) == N


def test_a_tolerance_nothing_misses_takes_ceil_n_over_p_sweeps():
    phis, y0 = toy_chain()
    got, strides = picard.solve(phis, y0, P, 1e30)
    assert len(strides) == math.ceil(N / P) and sum(strides) == N and np.isfinite(got).all()
    got5, strides5 = picard.solve(phis, y0, 5, 1e30)
    assert strides5 == [5, 5, 2]


def test_a_moderate_tolerance_lies_between_and_stays_close():
    phis, y0 = toy_chain()
    got, strides = picard.solve(phis, y0, P, 1e-6)
    assert math.ceil(N / P) <= len(strides) <= N and sum(strides) == N
    assert float(np.abs(got - sequential(phis, y0)).max()) < 1e-4


# ---- the stride rule and the bookkeeping ---------------------------------------------------------------------------------------------------
def test_stride_rule_on_hand_made_tables():
    numel, tol = 100, 1e-3
    ok, bad = 0.5 * numel * tol ** 2, 4.0 * numel * tol ** 2       # RMS 0.7 tol and 2 tol
    assert picard.stride([[0.0, 0.0, 0.0, bad]], numel, tol, 4) == 3         # a leading zero run
    assert picard.stride([[0.0, 0.0, bad, 0.0]], numel, 0.0, 4) == 2         # tol = 0 accepts exact zeros only
    assert picard.stride([[ok, ok, bad, ok]], numel, tol, 4) == 2
    assert picard.stride([[bad, ok, ok, ok]], numel, tol, 4) == 1            # the first row over the tolerance: 1, it is final anyway
    assert picard.stride([[ok, ok, ok, ok]], numel, tol, 4) == 4
    assert picard.stride([[numel * tol ** 2, bad]], numel, tol, 2) == 1      # the edge counts: sqrt(r / numel) == tol
    # several images share the window: a row counts only if every image accepts it
    assert picard.stride([[ok, ok, ok, ok], [ok, bad, ok, ok]], numel, tol, 4) == 1
    assert picard.stride([[ok, ok, ok, bad], [ok, ok, bad, ok]], numel, tol, 4) == 2
    # dead rows at the end of the schedule never count, whatever their entries say
    assert picard.stride([[ok, ok, 0.0, 0.0]], numel, tol, 2) == 2
    assert picard.stride([[bad, 0.0, 0.0, 0.0]], numel, tol, 1) == 1
    assert picard.stride([[float("nan"), ok]], numel, tol, 2) == 1           # a NaN accepts nothing
    assert picard.stride([[ok, float("inf")]], numel, 1e30, 2) == 1


def _lib_stride(residuals, numel, tol, live):
    r = np.ascontiguousarray(residuals, dtype=np.float64)
    return _lib.lib().cdc_parallel_stride(r.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), r.shape[0], r.shape[1], live, float(numel), float(tol))


def _lib_row_steps(w, p, steps):
    out = (ctypes.c_int * p)()
    assert _lib.lib().cdc_parallel_row_steps(w, p, steps, out) == 0
    return list(out)


def test_the_librarys_own_rule_on_the_same_tables(monkeypatch):
    """The host functions the sweep loop of cdc_decode_parallel calls (window_stride, window_row_steps), through their device-free
    entry points: the hand-made tables above and a random sweep of tables against the Python statement."""
    monkeypatch.setattr(picard, "stride", _lib_stride)
    monkeypatch.setattr(picard, "row_steps", _lib_row_steps)
    test_stride_rule_on_hand_made_tables()
    test_row_steps_follow_the_ring()
    monkeypatch.undo()
    rng = np.random.default_rng(7)
    for _ in range(300):
        B, p = int(rng.integers(1, 4)), int(rng.integers(2, 9))
        live, tol = int(rng.integers(1, p + 1)), float(rng.choice([0.0, 1e-3, 1e30]))
        r = np.where(rng.random((B, p)) < 0.6, 0.0, rng.random((B, p)) * 3e-4)
        assert _lib_stride(r, 100, tol, live) == picard.stride(r.tolist(), 100, tol, live)
        w, steps = int(rng.integers(0, 20)), int(rng.integers(2, 30))
        assert _lib_row_steps(w, p, steps) == picard.row_steps(w, p, steps)
    assert _lib_stride(np.zeros((1, 2)), 100, 0.0, 3) < 0 and _lib_stride(np.zeros((1, 2)), 0, 0.0, 1) < 0


def test_row_steps_follow_the_ring():
    assert picard.row_steps(0, 4, 12) == [11, 10, 9, 8]
    assert picard.row_steps(1, 4, 12) == [7, 10, 9, 8]                       # y_4 took the slot of y_0
    assert picard.row_steps(6, 4, 12) == [3, 2, 5, 4]
    assert picard.row_steps(10, 4, 12) == [0, 0, 1, 0]                       # j = 12, 13: dead, clamped
    assert [picard.live_rows(w, 4, 12) for w in (0, 8, 9, 11)] == [4, 4, 3, 1]
    for w in range(12):
        steps = picard.row_steps(w, 5, 12)
        for k in range(5):
            assert steps[(w + k) % 5] == max(0, 11 - (w + k))


# ---- the float32 restatement inside the bound the GPU test uses -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,p,B", [((3, 5, 7), 5, 2), ((3, 8, 8), 2, 1)])
def test_float32_restatement_stays_inside_the_float64_bound(shape, p, B):
    fx, y = PR.inputs(B, p, shape)
    from cdc_compression_amd import synth
    worst = 0.0
    for pred in (R.PRED_X, R.PRED_NOISE, R.PRED_V):
        s = R.schedules()[R.tree_of(pred)]
        for clip in R.CLIPS:
            for eta in (0.0, 0.7):
                for w in (0, s.steps - p + 1 if p < s.steps else 2):          # the second base leaves dead rows
                    noise = None if eta == 0 else [synth.normal(f"z{m}", (B,) + shape, seed=9 + m, std=1.0) for m in range(p)]
                    ref, bound = PR.sweep_f64(s, w, fx, y, noise, eta, pred, clip)
                    assert ref.shape[1] == (p if w == 0 else s.steps - w) and (w == 0 or ref.shape[1] < p)
                    for cand in (0, 1):
                        got = PR.sweep_f32(s, w, fx, y, noise, eta, pred, clip, c_eps=cand)
                        err = np.abs(got.astype(np.float64) - ref)
                        assert np.all(err <= bound), (pred, clip, eta, w, float((err / bound).max()))
                        worst = max(worst, float((err / bound).max()))
    assert 0 < worst <= 1
    print(f"{shape} p={p} B={B}: worst float32 error / bound = {worst:.3f}")


# ---- argument rules -----------------------------------------------------------------------------------------------------------------------
def test_check_args():
    assert picard.check_args(None, None, 10, 1) is None and picard.check_args(False, None, 10, 1) is None
    assert picard.check_args(True, None, 500, 1) == (16, 1e-3) == (picard.DEFAULT_WINDOW, picard.DEFAULT_TOL)
    assert picard.check_args(8, 0, 500, 2) == (8, 0.0)
    assert picard.check_args(32, 1e-2, 7, 1) == (7, 1e-2)                    # a window above the schedule is the whole schedule
    assert picard.check_args(4, None, 7, 2, eta=0.7, seed=3) == (4, 1e-3)
    for kw, msg in ((dict(sampler="dpmpp_2m"), "history"), (dict(tile=64), "excludes tile"), (dict(samples=4), "excludes samples"),
                    (dict(trajectory=[0]), "excludes trajectory"), (dict(eta=0.5), "needs a seed")):
        with pytest.raises(ValueError, match=msg):
            picard.check_args(4, None, 10, 1, **kw)
    for args, msg in (((1, None, 10, 1), "at least 2 steps"), ((4, None, 1, 1), "at least 2 steps"), ((4, -1e-3, 10, 1), "parallel_tol"),
                      ((4, float("nan"), 10, 1), "parallel_tol"), ((400, None, 5000, 1), "at most 256"), ((16, None, 100, 5000), "rows"),
                      ((None, 1e-3, 10, 1), "belongs to parallel")):
        with pytest.raises(ValueError, match=msg):
            picard.check_args(*args)


def test_the_mirror_refuses_before_the_library_is_touched():
    """No weights are loaded: the refusal is the argument's, not a missing state dict's."""
    kw = dict(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    diff = cdc.GaussianDiffusionEps(cdc.Unet(**kw), cdc.BigCompressor(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3),
                                    num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")
    M = diff.padded_size(1, 1)[0]
    q = np.zeros((1, 48, 8 * M // 4, 8 * M // 4), np.float32)
    img = np.zeros((1, 3, 8 * M, 8 * M), np.float32)
    dec = lambda **k: diff.decompress(q, (1, 3, 8 * M, 8 * M), sample_steps=4, **k)      # noqa: E731
    for call in (dec, lambda **k: diff.compress(img, 4, sample_mode="ddim", **k), lambda **k: diff.evaluate(img, 4, sample_mode="ddim", **k)):
        with pytest.raises(ValueError, match="history"):
            call(parallel=4, sampler="dpmpp_2m")
        with pytest.raises(ValueError, match="excludes tile"):
            call(parallel=True, tile=2 * M)
        with pytest.raises(ValueError, match="excludes trajectory"):
            call(parallel=4, trajectory=[0])
        with pytest.raises(ValueError, match="needs a seed"):
            call(parallel=4, eta=0.5)
        with pytest.raises(ValueError, match="belongs to parallel"):
            call(parallel_tol=1e-3)
    with pytest.raises(ValueError, match="excludes samples"):
        dec(parallel=4, samples=2, seed=1, gamma=0.8)
    with pytest.raises(ValueError, match="excludes partial"):
        dec(parallel=4, partial=True)
    with pytest.raises(ValueError, match="return_info belongs to parallel"):
        dec(return_info=True)


def test_the_library_refuses_by_argument_name():
    """On a handle that never touches a device: what cdc_decode_parallel checks before it asks for one."""
    L = _lib.lib()
    un = cdc.Unet(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    h = un._handle()
    out = np.zeros((1, 3, 64, 64), np.float32)
    ctx = (ctypes.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
    seeds = (ctypes.c_uint64 * 1)(5)

    def call(B=1, window=4, tol=1e-3, eta=0.0, sd=None, gamma=0.0):
        rc = L.cdc_decode_parallel(h, out.ctypes.data, gamma, sd, eta, ctx, 2, out.ctypes.data, B, 64, 64, 0, 1, window, tol, None, None,
                                   _lib.CDC_MEM_HOST, None)
        return rc, L.cdc_last_error(h).decode()

    for kw, msg in ((dict(window=1), "window 1"), (dict(window=257), "beyond the update kernel's 256 rows"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(eta=0.5), "eta != 0 needs seeds"),
                    (dict(B=4096, window=16), "B \\* window"), (dict(B=0), "B=0"), (dict(eta=float("inf"), sd=seeds), "not finite")):
        rc, err = call(**kw)
        assert rc != 0 and re.search(msg, err), (kw, rc, err)
    rc, err = call()                                         # nothing wrong with the arguments: the state is what is missing
    assert rc != 0 and "window" not in err and "tol" not in err


def test_entry_points_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "cdc_hip.h")).read()
    L = _lib.lib()
    for name in ("cdc_decode_parallel", "cdc_op_window_update", "cdc_parallel_stride", "cdc_parallel_row_steps"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(L, name)
    assert "cdc_parallel_info" in hdr and ctypes.sizeof(_lib.ParallelInfo) == 24
