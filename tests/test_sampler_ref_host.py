"""tests/sampler_ref.py checked against itself, without a GPU: the float32 operation-by-operation evaluation stays inside the float64
statement's bound at every case tests/test_gpu_ddim_update.py runs, deliberately wrong variants leave it on the same inputs, and the
inputs reach the edges the cases are there for.

One variant cannot leave ANY honest bound around the float64 value and is handled apart (test_a_fused_numerator_...): a fused
`sqrt_recip x - x0` rounds once where the reference rounds twice, so it is the more accurate of the two and sits inside whatever bound
the unfused form needs.  What sees it is equality of bits with ddim_update_f32, which the GPU test asserts beside the bound."""
import ctypes

import numpy as np
import pytest

import sampler_ref as R
from cdc_compression_amd import _lib

SCHED = R.schedules()
SMALL_SHAPES = [s for s in R.SHAPES if s != R.BIG]


@pytest.fixture(scope="module")
def data():
    return {shape: R.inputs(shape) for shape in SMALL_SHAPES}


def _inside(got, ref, bound):
    """Elementwise |got - ref| <= bound; a NaN on either side is outside."""
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - ref) <= bound


def _statement(s, i, fx, x, noise, eta, pred, clip, wrong=None):
    """ddim_update_f64's value restated (wrong=None: the same numbers), with one deliberate mistake `wrong`."""
    fx, x = fx.astype(np.float64), x.astype(np.float64)
    B = x.shape[0]
    d = lambda t: np.float64(t[i])                                   # noqa: E731
    r, m = d(s.sqrt_recip), d(s.sqrt_recipm1)
    x0 = fx if pred == R.PRED_X else (d(s.sqrt_ac) * x - d(s.sqrt_one_minus_ac) * fx if pred == R.PRED_V else r * x - m * fx)
    n = R.n_clipped(B, clip)
    clamped = x0.copy()
    if wrong == "other_half" and clip == R.CLIP_HALF:
        clamped[B - n:] = np.clip(x0[B - n:], -1.0, 1.0)
    else:
        clamped[:n] = np.clip(x0[:n], -1.0, 1.0)
    from_x0 = x0 if wrong == "clip_after_eps" else clamped
    eps = fx if pred in (R.PRED_NOISE, R.PRED_NOISE_XTREE) else (r * x - from_x0) / m
    sig = np.float64(s.sigma[i]) if wrong == "sigma_without_eta" else np.float64(np.float32(np.float32(eta) * s.sigma[i]))
    var = d(s.one_minus_ac_prev) - sig * sig
    clamp_var = (pred != R.PRED_NOISE) != (wrong == "sqrt_clamp_swapped")
    with np.errstate(invalid="ignore"):
        c_eps = np.sqrt(max(var, 0.0) if clamp_var else var)
        out = d(s.sqrt_ac_prev) * clamped + c_eps * eps
    return out if noise is None else out + sig * noise.astype(np.float64)


def test_the_restatement_is_the_statement(data):
    fx, x, nz = data[(3, 3, 5, 7)]
    for pred, clip, eta in R.combos((3, 3, 5, 7)):
        for i in R.STEP_LIST:
            noise = nz if eta else None
            ref, bound = R.ddim_update_f64(SCHED[R.tree_of(pred)], i, fx, x, noise, eta, pred, clip)
            got = _statement(SCHED[R.tree_of(pred)], i, fx, x, noise, eta, pred, clip)
            # (the statement takes c_eps from the exact rational var, this one from the float64 difference: 2^-53 apart, relatively)
            assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-300), (pred, clip, eta, i)
            assert np.all(bound >= 0) and np.all(np.isfinite(bound))


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_float32_operation_by_operation_stays_inside_the_bound(data, shape):
    """What the reference's tensor operations compute, for either contraction of the step's scalars."""
    fx, x, nz = data[shape]
    worst = 0.0
    for pred, clip, eta in R.combos(shape):
        s = SCHED[R.tree_of(pred)]
        for i in R.STEP_LIST:
            noise = nz if eta else None
            ref, bound = R.ddim_update_f64(s, i, fx, x, noise, eta, pred, clip)
            for c in R.step_scalars(s, i, eta, pred)["c_eps"]:
                got = R.ddim_update_f32(s, i, fx, x, noise, eta, pred, clip, c_eps=c)
                ok = _inside(got, ref, bound)
                assert ok.all(), (shape, pred, clip, eta, i, int((~ok).sum()))
                worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
    print(f"{shape}: float32 operation by operation, worst error / bound = {worst:.3f}")
    assert worst > 0.25                      # (and the bound is no orders of magnitude above what one evaluation really loses)


# the edge, the cases it concerns: (pred, clip, eta, i)
def _concerned(wrong):
    if wrong == "other_half":                # three images: the first is clamped, the variant clamps the last
        return [(p, R.CLIP_HALF, e, i) for p in R.PREDS for e in (0.0, 0.5) for i in R.STEP_LIST]
    if wrong == "sqrt_clamp_swapped":        # dropped in the x tree (NaN), added in the eps tree (numbers where the reference has NaN)
        return [(p, c, R.ETA_OVER, R.OVER_STEP) for p in R.PREDS for c in R.CLIPS]
    if wrong == "sigma_without_eta":
        return [(p, c, 0.5, i) for p in R.PREDS for c in R.CLIPS for i in (4, 2)]           # (sigma[0] = 0)
    if wrong == "clip_after_eps":            # eps is formed from x0 in pred_mode x and v only, and weighs c_eps = 0 at i = 0
        return [(p, c, e, i) for p in (R.PRED_X, R.PRED_V) for c in (R.CLIP_ALL, R.CLIP_HALF) for e in (0.0, 0.5) for i in (4, 2)]
    raise KeyError(wrong)


@pytest.mark.parametrize("wrong", ["other_half", "sqrt_clamp_swapped", "sigma_without_eta", "clip_after_eps"])
@pytest.mark.parametrize("shape", [(3, 3, 24, 44), (3, 3, 5, 7)])
def test_a_wrong_update_leaves_the_bound(data, shape, wrong):
    fx, x, nz = data[shape]
    for pred, clip, eta, i in _concerned(wrong):
        s = SCHED[R.tree_of(pred)]
        noise = nz if eta else None
        ref, bound = R.ddim_update_f64(s, i, fx, x, noise, eta, pred, clip)
        bad = _statement(s, i, fx, x, noise, eta, pred, clip, wrong=wrong)
        out = ~_inside(bad, ref, bound)
        assert out.any(), (wrong, pred, clip, eta, i)
        if wrong == "sqrt_clamp_swapped":
            assert out.all() and np.isnan(bad).all() == (pred != R.PRED_NOISE) and np.isnan(ref).all() == (pred == R.PRED_NOISE)


@pytest.mark.parametrize("shape", [(3, 3, 24, 44), (3, 3, 5, 7)])
def test_the_draw_of_another_step_leaves_the_bound(shape):
    """Noise drawn with index i in place of i + 1 (cdc_randn_host: the generator's host statement)."""
    fx, x, _ = R.inputs(shape)
    L = _lib.lib()
    seeds = (ctypes.c_uint64 * shape[0])(*[(7 << 32) + 11 + b for b in range(shape[0])])
    per = int(np.prod(shape[1:]))

    def draw(k):
        z = np.empty(shape, np.float32)
        assert L.cdc_randn_host(seeds, shape[0], per, k, 1.0, z.ctypes.data) == 0
        return z
    for pred in R.PREDS:
        s = SCHED[R.tree_of(pred)]
        for i in (4, 2):
            ref, bound = R.ddim_update_f64(s, i, fx, x, draw(i + 1), 0.5, pred, R.CLIP_ALL)
            bad, _ = R.ddim_update_f64(s, i, fx, x, draw(i), 0.5, pred, R.CLIP_ALL)
            assert (~_inside(bad, ref, bound)).mean() > 0.5, (pred, i)


def test_a_fused_numerator_stays_inside_the_bound_and_differs_in_bits(data):
    """fma(sqrt_recip, x, -x0) in eps's numerator, pred_mode x and v.  It rounds once where the unfused form rounds twice, so its error
    is bounded by the same derivation less one term: no bound that the reference's own arithmetic meets can exclude it.  It does change
    bits wherever c_eps != 0 -- about one element in four at (3,3,24,44) -- so the check that sees it is bit equality with
    ddim_update_f32, which tests/test_gpu_ddim_update.py asserts.  At i = 0, the step with the smallest sqrt_recipm1, c_eps is 0 in every
    mode and eps does not reach the result at all."""
    fx, x, nz = data[(3, 3, 24, 44)]
    s = SCHED["x"]
    for pred in (R.PRED_X, R.PRED_V):
        for clip in R.CLIPS:
            for eta, i in ((0.0, 4), (0.0, 2), (0.5, 4), (0.5, 2), (1.0, 2), (0.0, 0), (0.5, 0)):
                noise = nz if eta else None
                ref, bound = R.ddim_update_f64(s, i, fx, x, noise, eta, pred, clip)
                plain = R.ddim_update_f32(s, i, fx, x, noise, eta, pred, clip)
                fused = R.ddim_update_f32(s, i, fx, x, noise, eta, pred, clip, fused=True)
                assert _inside(fused, ref, bound).all()
                differs = int((plain != fused).sum())
                assert (differs > 100) if i else (differs == 0), (pred, clip, eta, i, differs)


def test_the_inputs_reach_the_edges(data):
    for s in SCHED.values():
        for t in (s.sqrt_recip, s.sqrt_recipm1, s.sqrt_ac_prev, s.one_minus_ac_prev, s.sigma, s.sqrt_ac, s.sqrt_one_minus_ac):
            assert t.dtype == np.float32 and np.isfinite(t).all()
        assert np.all(s.sqrt_recipm1 != 0)
        assert s.one_minus_ac_prev[0] == 0 and s.sigma[0] == 0
        assert int(np.argmin(s.sqrt_recipm1)) in R.STEP_LIST
    # clip = half at three images: some |x0| > 1 in the clipped image and in an unclipped one, in every mode at every step
    for shape in ((3, 3, 24, 44), (3, 3, 24, 42), (3, 3, 5, 7)):
        fx, x, _ = data[shape]
        assert R.n_clipped(shape[0], R.CLIP_HALF) == 1
        for pred in R.PREDS:
            for i in R.STEP_LIST:
                x0, _ = R.predict_x0_f64(SCHED[R.tree_of(pred)], i, fx.astype(np.float64), x.astype(np.float64), pred, R.CLIP_NONE)
                assert (np.abs(x0[0]) > 1).any() and (np.abs(x0[1:]) > 1).any(), (shape, pred, i)
    # eta > 1: var < 0 for both float32 candidates, in both trees (the x tree clamps it, the eps tree takes its root)
    for pred in R.PREDS:
        k = R.step_scalars(SCHED[R.tree_of(pred)], R.OVER_STEP, R.ETA_OVER, R.PRED_NOISE)      # (unclamped: as the eps tree forms it)
        assert all(v < 0 for v in k["var"]), (pred, k["var"])
    k = R.step_scalars(SCHED["eps"], R.OVER_STEP, R.ETA_OVER, R.PRED_NOISE)
    assert all(np.isnan(c) for c in k["c_eps"]) and np.isnan(k["c_eps64"])
    k = R.step_scalars(SCHED["x"], R.OVER_STEP, R.ETA_OVER, R.PRED_X)
    assert all(c == 0 for c in k["c_eps"]) and k["c_eps64"] == 0 and k["dc"] == 0
    # the eps tree at the etas of the float64 comparison: the two candidates agree on var's sign, so no case hangs on the contraction
    for eta in R.ETAS:
        for i in R.STEP_LIST:
            v = R.step_scalars(SCHED["eps"], i, eta, R.PRED_NOISE)["var"]
            assert (v[0] < 0) == (v[1] < 0) and not any(x < 0 for x in v), (eta, i, v)
    # eta = 1 cancels: the candidates differ somewhere, and the spread is carried
    assert any(R.step_scalars(s, i, 1.0, p)["var"][0] != R.step_scalars(s, i, 1.0, p)["var"][1]
               for p, s in ((R.PRED_X, SCHED["x"]), (R.PRED_NOISE, SCHED["eps"])) for i in R.STEP_LIST)


def test_round_to_float32_of_a_rational():
    from fractions import Fraction
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert R._round_f32(one + ulp / 2) == np.float32(1)                              # a tie: to the even neighbour
    assert R._round_f32(one + 3 * ulp / 2) == np.float32(1 + 2.0 ** -22)             # a tie: to the even neighbour, upwards
    assert R._round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.float32(1 + 2.0 ** -23)      # float64 would have made it a tie
    assert R._round_f32(Fraction(-3, 8)) == np.float32(-0.375)


def test_combine_sums_the_rows_inside_the_image():
    rng = np.random.default_rng(0)
    P = rng.standard_normal((2, 3, 7, 4, 8)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    got, mag = R.combine(P, b, 3, np.float64)
    want = np.zeros((2, 3, 4, 8))
    for y in range(4):
        for ky in range(7):
            if 0 <= y + ky - 3 < 4:
                want[:, :, y] += P[:, :, ky, y + ky - 3]
    want += b[None, :, None, None]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert np.all(mag >= np.abs(got) - 1e-12)
    f32, _ = R.combine(P, b, 3)
    assert f32.dtype == np.float32 and np.all(np.abs(f32 - got) <= 7 * R.U * mag)
