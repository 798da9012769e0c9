"""Host half of the second-order multistep sampler (no GPU): the logSNR step grid and the a / b / c tables of
cdc_compression_amd.schedule, checked on their own definitions and on a model problem with a closed-form answer.

The model problem: data N(MU, SD^2), whose exact denoiser is linear and whose probability-flow ODE keeps the quantile of the
marginal, so the sample a start point must arrive at is known.  It is driven through the package's own tables by the float64
loops below.  The conditions are about the tables' correctness (orders of convergence, the grid they need), not picture quality."""
import numpy as np
import pytest

from cdc_compression_amd import schedule
from cdc_compression_amd.schedule import SampleSchedule, half_logsnr, logsnr_index, solver_tables

PUBLISHED = [("x", "cosine", 8193), ("eps", "linear", 20000)]
MU, SD = 0.3, 0.5


@pytest.mark.parametrize("tree,vs,T", PUBLISHED)
def test_logsnr_grid_is_strictly_increasing_between_the_ends(tree, vs, T):
    for steps in (2, 3, 4, 17, 1000, T - 1, T):
        s = SampleSchedule(T, vs, tree, steps, spacing="logsnr")
        assert s.index.shape == (steps,) and s.index[0] == 0 and s.index[-1] == T - 1, steps
        assert np.all(np.diff(s.index) > 0), steps
        assert s.spacing == "logsnr" and s.steps == steps
        np.testing.assert_array_equal(s.time_in, (s.index.astype(np.float32) / np.float32(T)).astype(np.float32))
    with pytest.raises(ValueError):
        SampleSchedule(T, vs, tree, T + 1, spacing="logsnr")
    # 17 steps: on the clean half, where the train grid is fine in lambda, the steps are the uniform target step (the noisy end of
    # the cosine schedule is where the train indices themselves are 0.3 to 3.5 apart, and the grid can only take them as they are)
    s = SampleSchedule(T, vs, tree, 17, spacing="logsnr")
    lam = half_logsnr(s.alphas_cumprod)
    h = -np.diff(lam)
    target = (half_logsnr(s.alphas_cumprod[:1])[0] - lam[-1]) / 16
    assert np.all(np.abs(h[:8] / target - 1) < 0.05), (h, target)
    ref = SampleSchedule(T, vs, tree, 17)
    hr = -np.diff(half_logsnr(ref.alphas_cumprod))
    assert hr.max() / hr.min() > 10.0          # what the index-uniform grid does to the same steps


@pytest.mark.parametrize("tree,vs,T", PUBLISHED)
def test_one_step_and_index_spacing_are_todays_schedule(tree, vs, T):
    fields = ("index", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip", "sqrt_recipm1", "sqrt_ac_prev", "sqrt_ac",
              "sqrt_one_minus_ac", "one_minus_ac_prev", "sigma", "time_in")
    for steps in (1, 5, 17):
        old = SampleSchedule(T, vs, tree, steps)
        for new in ([SampleSchedule(T, vs, tree, steps, spacing="index")] + ([SampleSchedule(T, vs, tree, 1, spacing="logsnr")] if steps == 1 else [])):
            for f in fields:
                a, b = getattr(old, f), getattr(new, f)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (steps, f)
    # today's rules, stated: the two-sided float32 linspace, the x tree's one-step special case, the eps tree's t / steps
    assert SampleSchedule(T, vs, tree, 1).index[0] == (T - 1 if tree == "x" else 0)
    np.testing.assert_array_equal(SampleSchedule(T, vs, tree, 5).index, schedule.linspace_index(T, 5))
    if tree == "eps":
        np.testing.assert_array_equal(SampleSchedule(T, vs, tree, 4).time_in, np.float32([0, 0.25, 0.5, 0.75]))


def test_explicit_grid_rules():
    T = 8193
    s = SampleSchedule(T, "cosine", "x", 3, spacing=np.array([0, 100, T - 1]))
    np.testing.assert_array_equal(s.index, [0, 100, T - 1])
    e = SampleSchedule(20000, "linear", "eps", 3, spacing=[5, 100, 19999])
    np.testing.assert_array_equal(e.time_in, (np.float32([5, 100, 19999]) / np.float32(20000)).astype(np.float32))
    for bad in ([0, 100, 100], [0, 200, 100], [-1, 5, 9], [0, 5, T], [[0, 1, 2]], [0.0, 1.0, 2.0], [0, 1]):
        with pytest.raises(ValueError):
            SampleSchedule(T, "cosine", "x", 3, spacing=np.array(bad))
    with pytest.raises(ValueError):
        SampleSchedule(T, "cosine", "x", 3, spacing="karras")


@pytest.mark.parametrize("tree,vs,T", PUBLISHED)
@pytest.mark.parametrize("spacing", ["index", "logsnr"])
def test_first_order_is_the_ddim_step(tree, vs, T, spacing):
    for steps in (2, 5, 17, 65):
        s = SampleSchedule(T, vs, tree, steps, spacing=spacing)
        ac, acp = s.alphas_cumprod.astype(np.float64), s.alphas_cumprod_prev.astype(np.float64)
        a, b, c = solver_tables(s.alphas_cumprod, s.alphas_cumprod_prev, order=1, dtype=np.float64)
        assert a[0] == 0.0 and b[0] == 1.0 and not c.any()
        ddim = np.sqrt(acp[1:]) - np.sqrt(ac[1:]) * a[1:]           # x0's coefficient of the eta = 0 DDIM step, eps eliminated
        assert np.all(np.abs(b[1:] - ddim) <= 1e-9 * np.abs(ddim)), float(np.abs(b[1:] / ddim - 1).max())
        a2, b2, c2 = solver_tables(s.alphas_cumprod, s.alphas_cumprod_prev, order=2, dtype=np.float64)
        np.testing.assert_array_equal(a2, a)
        assert c2[0] == 0.0 and c2[-1] == 0.0 and b2[0] == b[0] and b2[-1] == b[-1]
        np.testing.assert_allclose(b2 + c2, b, rtol=1e-12)           # a constant prediction is integrated exactly by either order
        if steps > 2:
            assert np.all(c2[1:-1] < 0) and np.all(b2[1:-1] > b[1:-1])
        f = s.solver()
        assert all(t.dtype == np.float32 for t in f)
        np.testing.assert_array_equal(f[1], b2.astype(np.float32))
    with pytest.raises(ValueError):
        solver_tables(s.alphas_cumprod, s.alphas_cumprod_prev, order=3)


def _x0(x, ac):
    """E[x0 | x_t] for data N(MU, SD^2)."""
    al, var = np.sqrt(ac), 1.0 - ac
    return MU + al * SD * SD * (x - al * MU) / (ac * SD * SD + var)


def _model_error(tree, vs, T, steps, sampler, spacing):
    """max over 9 start points within +-2 sigma of |final sample - exact probability-flow solution|, float64 stepping over the
    package's float32 tables."""
    s = SampleSchedule(T, vs, tree, steps, spacing=spacing)
    ac = s.alphas_cumprod.astype(np.float64)
    z = np.linspace(-2.0, 2.0, 9)
    x = np.sqrt(ac[-1]) * MU + np.sqrt(ac[-1] * SD * SD + 1.0 - ac[-1]) * z
    exact = MU + SD * z
    if sampler == "ddim":
        for i in reversed(range(steps)):
            x0 = _x0(x, ac[i])
            eps = (np.float64(s.sqrt_recip[i]) * x - x0) / np.float64(s.sqrt_recipm1[i])
            x = np.float64(s.sqrt_ac_prev[i]) * x0 + np.sqrt(np.float64(s.one_minus_ac_prev[i])) * eps
    else:
        a, b, c = (t.astype(np.float64) for t in s.solver())
        prev = np.zeros_like(x)
        for i in reversed(range(steps)):
            x0 = _x0(x, ac[i])
            x = a[i] * x + b[i] * x0 + c[i] * prev
            prev = x0
    return float(np.abs(x - exact).max())


@pytest.mark.parametrize("tree,vs,T", PUBLISHED)
def test_model_problem_orders_of_convergence(tree, vs, T):
    for steps in (17, 33, 65):
        e2m, edd = _model_error(tree, vs, T, steps, "dpmpp_2m", "logsnr"), _model_error(tree, vs, T, steps, "ddim", "index")
        print(f"{vs} {steps}: 2M/logsnr {e2m:.3e}  ddim/index {edd:.3e}  ratio {edd / e2m:.2f}")
        assert e2m <= edd / 2, (steps, e2m, edd)
    f2 = _model_error(tree, vs, T, 65, "dpmpp_2m", "logsnr") / _model_error(tree, vs, T, 129, "dpmpp_2m", "logsnr")
    f1 = _model_error(tree, vs, T, 65, "ddim", "logsnr") / _model_error(tree, vs, T, 129, "ddim", "logsnr")
    print(f"{vs} 65 -> 129 on the logSNR grid: 2M falls by {f2:.2f}, ddim by {f1:.2f}")
    assert f2 >= 3.0, f2
    assert f1 <= 2.2, f1


def test_keywords_are_on_every_public_entry_and_checked_before_anything_runs():
    import inspect
    import cdc_compression_amd as cdc
    from cdc_compression_amd import _lib
    for cls in (cdc.GaussianDiffusionX, cdc.GaussianDiffusionEps):
        for meth, defaults in (("compress", ("ddim", "index")), ("decompress", ("ddim", "index")), ("set_sample_schedule", ("ddim", "index")),
                               ("p_sample_loop", (None, None))):       # p_sample_loop: None runs what set_sample_schedule was given
            p = inspect.signature(getattr(cls, meth)).parameters
            assert (p["sampler"].default, p["spacing"].default) == defaults, (cls.__name__, meth)
    # evaluate() takes compress()'s arguments
    assert "sampler" in inspect.signature(cdc.GaussianDiffusionX.compress).bind(None, None, sampler="dpmpp_2m", spacing="logsnr").arguments
    d = cdc.GaussianDiffusionX(None, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    e = cdc.GaussianDiffusionEps(None, None, num_timesteps=20000, pred_mode="noise", var_schedule="linear")
    for diff in (d, e):                                                # no model behind them: the argument rules come first
        assert diff.sampler == "ddim"
        with pytest.raises(ValueError, match="eta must be 0"):
            diff.decompress([np.zeros((1, 3, 64, 64), np.float32)], sample_steps=4, eta=0.5, sampler="dpmpp_2m")
        with pytest.raises(ValueError, match="sampler"):
            diff.decompress([np.zeros((1, 3, 64, 64), np.float32)], sample_steps=4, sampler="order1")
        with pytest.raises(ValueError, match="eta must be 0"):
            diff.compress(np.zeros((1, 3, 64, 64), np.float32), sample_steps=4, eta=0.5, seed=1, sampler="dpmpp_2m")
    for name in ("cdc_set_solver", "cdc_decode_solver", "cdc_solver_step", "cdc_op_solver_update", "cdc_op_ddim_update"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
