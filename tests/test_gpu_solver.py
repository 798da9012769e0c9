"""The second-order multistep sampler (sampler="dpmpp_2m") and the logSNR step grid on the MI355X: the sampler kernels alone against
float64 (cdc_op_solver_update), the loop against the reference's DDIM goldens through first-order tables, against the float64
statement of tests/golden/make_golden_solver.py, against its own stepped chain, under graph replay, seeded, and through the range guard.

The frames: the fixtures' own (small_x, small_eps 32 x 32; odd_x 24 x 40) take the four-pixel kernel; odd_x's model on 24 x 42 takes the
scalar one."""
import ctypes
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from cdc_compression_amd.schedule import SampleSchedule
from helpers import GOLDEN, load_case
from sampler_ref import predict_x0_f64
from test_gpu_parity import TOL_DEC, make_unet, relerr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24        # unit roundoff of float32


def _diff(un, tree, **kw):
    if tree == "x":
        return cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode=kw.get("pred_mode", "x"), var_schedule="cosine")
    return cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise=kw.get("clip_noise", "none"), pred_mode="noise",
                                    var_schedule="linear")


def _odd_on_24x42():
    kw, man, sd, *_ = load_case("odd_x")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    B, H, W = 2, 24, 42
    return un, synth.context_pyramid([5], B, H, W, seed=3), synth.normal("init", (B, 3, H, W), seed=1, std=0.8)


# ---- the update in isolation ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabled():
    """A handle holding a 5-step schedule with every table the kernels read (pred_mode "v" sets the two extra ones), and the float64
    view of those float32 tables."""
    un, *_ = make_unet("small_x")
    diff = _diff(un, "x", pred_mode="v")
    diff.set_sample_schedule(5, sampler="dpmpp_2m")
    s = diff._sched
    a, b, c = (t.astype(np.float64) for t in diff.solver_tables)
    assert c[2] != 0 and c[1] != 0 and c[0] == 0 and c[4] == 0
    return un, diff, s, a, b, c


def _update_f64(s, a, b, c, i, fx, x, prev, pred, clip):
    """-> x0, its rounding bound where the kernel computes it, and the three terms of the update, all float64."""
    fx, x, prev = (t.astype(np.float64) for t in (fx, x, prev))
    x0, e0 = predict_x0_f64(s, i, fx, x, pred, clip)                 # (shared with the DDIM update's statement)
    return x0, e0, (a[i] * x, b[i] * x0, c[i] * prev)


def _op(un, i, fx, x, prev, pred, clip):
    L, h = _lib.lib(), un._handle()
    xn, x0 = np.full_like(x, np.nan), np.full_like(x, np.nan)
    B, C, H, W = x.shape
    _lib.check(h, L.cdc_op_solver_update(h, fx.ctypes.data, x.ctypes.data, prev.ctypes.data, i, xn.ctypes.data, x0.ctypes.data, B, C, H, W,
                                         pred, clip, _lib.CDC_MEM_HOST, None))
    return xn, x0


# 24 x 44: four-pixel kernel, two blocks per plane; 24 x 42: scalar kernel, many blocks; 344 x 342: the scalar kernel's grid-stride loop
# (more than 4096 * 256 elements); 4 x 4: less than one wave
@pytest.mark.parametrize("shape", [(3, 3, 24, 44), (3, 3, 24, 42), (2, 3, 4, 4), (3, 3, 344, 342)])
def test_update_alone_against_float64(tabled, shape):
    un, diff, s, a, b, c = tabled
    fx, x, prev = (synth.normal(n, shape, seed=5, std=sd) for n, sd in (("fx", 1.2), ("x", 0.8), ("prev", 0.7)))
    big = shape[2] > 100
    worst = 0.0
    for pred in (_lib.CDC_PRED_X, _lib.CDC_PRED_NOISE, _lib.CDC_PRED_NOISE_XTREE, _lib.CDC_PRED_V):
        for clip in (_lib.CDC_CLIP_ALL, _lib.CDC_CLIP_NONE, _lib.CDC_CLIP_HALF):
            for i in ((2,) if big else (2, 1)):
                if big and (pred, clip) not in ((_lib.CDC_PRED_X, _lib.CDC_CLIP_HALF), (_lib.CDC_PRED_V, _lib.CDC_CLIP_ALL)):
                    continue
                xn, x0 = _op(un, i, fx, x, prev, pred, clip)
                r0, e0, terms = _update_f64(s, a, b, c, i, fx, x, prev, pred, clip)
                mag = sum(np.abs(t) for t in terms)
                # the derived bound: no operation is fused, so three products and two sums round once each (at most 4 u of the terms'
                # magnitudes), plus |b| times the rounding of x0 where the kernel computes it
                bound = 4 * U * mag + abs(b[i]) * e0
                err = np.abs(xn.astype(np.float64) - sum(terms))
                assert np.all(err <= bound), (pred, clip, i, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err / bound).max()))
                if pred == _lib.CDC_PRED_X:
                    np.testing.assert_array_equal(x0, r0.astype(np.float32))
                else:
                    assert np.all(np.abs(x0.astype(np.float64) - r0) <= e0), (pred, clip, i)
                # x0_out is the very x0 the update used: with it in x0's place only the update's own five roundings remain
                t1 = b[i] * x0.astype(np.float64)
                err = np.abs(xn.astype(np.float64) - (terms[0] + t1 + terms[2]))
                assert np.all(err <= 4 * U * (np.abs(terms[0]) + np.abs(t1) + np.abs(terms[2]))), (pred, clip, i)
    print(f"{shape}: worst error / bound = {worst:.3f}")


def test_update_forms_hold_the_same_bits_and_run_in_place_on_the_device(tabled):
    """The same elements through the four-pixel kernel (W = 44, and as two long rows) and, reshaped to a width of 6, through the scalar
    one; and device tensors with x0_out = x0_prev."""
    import torch
    un, diff, s, a, b, c = tabled
    L, h = _lib.lib(), un._handle()
    shape = (2, 3, 24, 44)
    fx, x, prev = (synth.normal(n, shape, seed=6, std=sd) for n, sd in (("fx", 1.2), ("x", 0.8), ("prev", 0.7)))
    for pred, clip in ((_lib.CDC_PRED_V, _lib.CDC_CLIP_ALL), (_lib.CDC_PRED_NOISE, _lib.CDC_CLIP_NONE)):
        xn4, x04 = _op(un, 2, fx, x, prev, pred, clip)
        flat = (1, 1, 2, 3 * 24 * 44)                                  # W = 3168 = 4 * 792: also four-pixel, other plane split
        xn4b, x04b = _op(un, 2, *(t.reshape(flat) for t in (fx, x, prev)), pred, clip)
        odd = (1, 1, 2 * 3 * 24 * 44 // 6, 6)                         # W = 6: the scalar kernel over the same elements
        xn1, x01 = _op(un, 2, *(t.reshape(odd) for t in (fx, x, prev)), pred, clip)
        np.testing.assert_array_equal(xn4.ravel(), xn4b.ravel())
        np.testing.assert_array_equal(xn4.ravel(), xn1.ravel())
        np.testing.assert_array_equal(x04.ravel(), x01.ravel())
        dev = torch.device("cuda:0")
        tfx, tx, th = (torch.from_numpy(t).to(dev) for t in (fx, x, prev))
        tn = torch.empty_like(tx)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(h, L.cdc_op_solver_update(h, tfx.data_ptr(), tx.data_ptr(), th.data_ptr(), 2, tn.data_ptr(), th.data_ptr(), *shape, pred, clip,
                                             _lib.CDC_MEM_DEVICE, st))
        np.testing.assert_array_equal(tn.cpu().numpy(), xn4)
        np.testing.assert_array_equal(th.cpu().numpy(), x04)


def test_solver_entry_points_refuse_what_they_cannot_run(tabled):
    un, diff, s, a, b, c = tabled
    L, h = _lib.lib(), un._handle()
    z = np.zeros((1, 3, 4, 4), np.float32)
    args = lambda i, pred=0: (h, z.ctypes.data, z.ctypes.data, z.ctypes.data, i, z.ctypes.data, z.ctypes.data, 1, 3, 4, 4, pred, 0, 0, None)   # noqa: E731
    assert L.cdc_op_solver_update(*args(5)) != 0 and L.cdc_op_solver_update(*args(-1)) != 0
    assert L.cdc_set_solver(h, 4, s.sigma.ctypes.data, s.sigma.ctypes.data, s.sigma.ctypes.data) != 0      # another step count
    un2, *_ = make_unet("small_x")
    d2 = _diff(un2, "x")
    d2.set_sample_schedule(5)                                          # a schedule without solver tables
    h2 = un2._handle()
    assert L.cdc_op_solver_update(h2, *args(2)[1:]) != 0 and b"cdc_set_solver" in L.cdc_last_error(h2)
    d2.set_sample_schedule(5, sampler="dpmpp_2m")
    assert L.cdc_op_solver_update(h2, *args(2)[1:]) == 0
    assert L.cdc_op_solver_update(h2, *args(2, _lib.CDC_PRED_V)[1:]) != 0      # "v" needs its two tables
    d2.set_sample_schedule(6)                                          # a new schedule: the solver tables are stale
    assert L.cdc_op_solver_update(h2, *args(2)[1:]) != 0
    with pytest.raises(ValueError):
        d2.p_sample_loop(z.shape, [], sampler="dpmpp_2m", eta=0.5)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tree", [("small_x", "x"), ("small_eps", "eps")])
def test_first_order_tables_reproduce_the_reference_ddim_goldens(name, tree):
    """order = 1 (b = b1, c = 0) is algebraically the DDIM step at eta = 0: the solver loop, kernels and tables, pinned to the real
    reference's decode."""
    un, kw, sd, x, time, ctx, _ = make_unet(name)
    g = np.load(os.path.join(GOLDEN, f"decode_{name}.npz"))
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    diff = _diff(un, tree)
    keys = [k for k in g.files if k.startswith("decode_")]
    assert keys
    for key in keys:
        steps = int(key.split("_")[1])
        diff.set_sample_schedule(steps, sampler="dpmpp_2m")
        diff._set_solver_tables(*diff._sched.solver(order=1))
        rec = diff.p_sample_loop(x.shape, ctx, True, init=init) if tree == "x" else diff.p_sample_loop(x.shape, ctx, "ddim", init=init)
        e = relerr(rec, g[key])
        print(f"{name} {key}: first-order solver loop against the reference's DDIM {e:.3e}")
        assert e < TOL_DEC, (key, e)


# Measured on the MI355X (relerr against tests/golden/solver_small.npz); the bound is about 3 x that, and TOL_DEC where 3 x would pass
# it: the chain is expected within the project's decode bound, since |b|, |c| <= 4.1 on these grids.  For comparison, the first-order
# loop above sits 1.8e-5 from the reference's own four-step DDIM decode of small_x: five U-Net evaluations, each fed the last one's
# error, are what both figures measure.
#                      measured    bound
SOLVER_BOUND = {
    "small_x_index":     TOL_DEC,  # 3.302e-05 (1.5 x: capped at TOL_DEC)
    "small_x_logsnr":    TOL_DEC,  # 3.317e-05 (1.5 x: capped at TOL_DEC)
    "small_eps_index":   2.2e-6,   # 7.210e-07
    "small_eps_logsnr":  2.2e-6,   # 7.136e-07
    "odd_x_index":       TOL_DEC,  # 1.773e-05 (2.8 x: capped at TOL_DEC)
    "odd_x_logsnr":      2.3e-5,   # 7.451e-06
    "small_x_v_index":   3.7e-5,   # 1.228e-05
    "small_x_v_logsnr":  3.5e-5,   # 1.165e-05
}


@pytest.mark.parametrize("key,name,tree,kw", [("small_x", "small_x", "x", {}), ("small_eps", "small_eps", "eps", {}), ("odd_x", "odd_x", "x", {}),
                                              ("small_x_v", "small_x", "x", {"pred_mode": "v"})])
@pytest.mark.parametrize("spacing", ["index", "logsnr"])
def test_dpmpp_2m_matches_the_float64_statement(key, name, tree, kw, spacing):
    g = np.load(os.path.join(GOLDEN, "solver_small.npz"))
    un, _, sd, x, time, ctx, _ = make_unet(name)
    diff = _diff(un, tree, **kw)
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    k = f"{key}_{spacing}"
    rec = diff.decompress(ctx, x.shape, sample_steps=int(g["steps"]), init=init, sampler="dpmpp_2m", spacing=spacing)
    np.testing.assert_array_equal(diff.index, g[k + "_grid"])
    assert diff.sample_steps == int(g["steps"]) and diff.sampler == "dpmpp_2m"
    for t, n in zip(diff.solver_tables, "abc"):
        np.testing.assert_array_equal(t, g[f"{k}_{n}"])
    e = relerr(rec, g[k + "_rec"])
    print(f"{k}: {e:.3e} (bound {SOLVER_BOUND[k]:.1e})")
    assert SOLVER_BOUND[k] <= TOL_DEC
    assert e < SOLVER_BOUND[k], (k, e)
    # an explicit grid of the same indices is the same decode (the eps tree's "index" spacing alone feeds the U-Net i / steps)
    if tree == "x" or spacing == "logsnr":
        np.testing.assert_array_equal(rec, diff.decompress(ctx, x.shape, init=init, sampler="dpmpp_2m", spacing=g[k + "_grid"]))


def _stepped(diff, un, ctx, init, steps, pred, clip, spacing):
    """cdc_solver_step once per step, the history handed from call to call."""
    L, h = _lib.lib(), un._handle()
    diff.set_sample_schedule(steps, sampler="dpmpp_2m", spacing=spacing)
    B, _, H, W = init.shape
    img, hist = init.copy(), None
    ptrs = (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in ctx])
    for i in reversed(range(steps)):
        out, x0 = np.empty_like(img), np.empty_like(img)
        _lib.check(h, L.cdc_solver_step(h, img.ctypes.data, None if hist is None else hist.ctypes.data, i, ptrs, len(ctx), out.ctypes.data,
                                        x0.ctypes.data, B, H, W, pred, clip, _lib.CDC_MEM_HOST, None))
        img, hist = out, x0
    return img


@pytest.mark.parametrize("name,tree,kw", [("small_x", "x", {}), ("small_eps", "eps", {"clip_noise": "half"}), ("odd_x", "x", {}),
                                          ("small_x", "x", {"pred_mode": "v"}), ("24x42", "x", {})])
def test_fused_loop_is_the_stepped_chain_bit_for_bit(name, tree, kw):
    if name == "24x42":
        un, ctx, init = _odd_on_24x42()
    else:
        un, _, sd, x, time, ctx, _ = make_unet(name)
        init = synth.normal("init", x.shape, seed=1, std=0.8)
    diff = _diff(un, tree, **kw)
    rec = diff.decompress(ctx, init.shape, sample_steps=5, init=init, sampler="dpmpp_2m", spacing="logsnr")
    assert np.isfinite(rec).all()
    clip = diff._clip_flag(True if tree == "x" else diff.clip_noise)
    np.testing.assert_array_equal(rec, _stepped(diff, un, ctx, init, 5, diff._pred_flag(), clip, "logsnr"))
    # the second-order terms really went in, and the grid really changed
    first = diff.decompress(ctx, init.shape, sample_steps=5, init=init, spacing="logsnr")
    assert not np.array_equal(rec, first)
    assert not np.array_equal(first, diff.decompress(ctx, init.shape, sample_steps=5, init=init))


@pytest.mark.parametrize("name", ["small_x", "24x42"])
def test_graph_replay_equals_the_eager_loop(name, monkeypatch):
    if name == "24x42":
        un, ctx, init = _odd_on_24x42()
    else:
        un, _, sd, x, time, ctx, _ = make_unet(name)
        init = synth.normal("init", x.shape, seed=1, std=0.8)
    diff = _diff(un, "x")
    args = dict(sample_steps=5, init=init, sampler="dpmpp_2m", spacing="logsnr")
    monkeypatch.setenv("CDC_GRAPH", "0")
    eager = diff.decompress(ctx, init.shape, **args)
    eager_ddim = diff.decompress(ctx, init.shape, sample_steps=5, init=init)
    eager_index = diff.decompress(ctx, init.shape, **{**args, "spacing": "index"})
    monkeypatch.setenv("CDC_GRAPH", "1")
    a = diff.decompress(ctx, init.shape, **args)
    b = diff.decompress(ctx, init.shape, sample_steps=5, init=init)                    # the DDIM loop after a solver capture: a new capture
    c = diff.decompress(ctx, init.shape, **{**args, "spacing": "index"})               # other tables
    d = diff.decompress(ctx, init.shape, **args)                                       # and the first again: the history starts at zero
    monkeypatch.setenv("CDC_GRAPH", "0")
    np.testing.assert_array_equal(a, eager)
    np.testing.assert_array_equal(b, eager_ddim)
    np.testing.assert_array_equal(c, eager_index)
    np.testing.assert_array_equal(d, eager)


def test_seed_and_gamma_make_the_start_image():
    un, _, sd, x, time, ctx, _ = make_unet("small_x")
    diff = _diff(un, "x")
    args = dict(sample_steps=5, sampler="dpmpp_2m", spacing="logsnr")
    start = diff.randn(5, x.shape, draw=0, scale=0.8)
    rec = diff.decompress(ctx, x.shape, seed=5, gamma=0.8, **args)
    np.testing.assert_array_equal(rec, diff.decompress(ctx, x.shape, init=start, **args))
    assert not np.array_equal(rec, diff.decompress(ctx, x.shape, seed=6, gamma=0.8, **args))
    np.testing.assert_array_equal(diff.decompress(ctx, x.shape, seed=5, **args), diff.decompress(ctx, x.shape, **args))     # no gamma: zeros


def test_range_guard_repeats_the_decode_with_a_fresh_history():
    """The heavy-tail "overflow" fixture leaves the fp16 range: the decode is repeated in CDC_ARITH_BF16X3, history zero-filled again,
    and equals the decode of a handle that was in that arithmetic from the start."""
    from test_oracle import heavy_tail_case
    kw, sd, x, time, ctx, *_ = heavy_tail_case("overflow")
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    L = _lib.lib()
    args = dict(sample_steps=5, init=init, sampler="dpmpp_2m", spacing="logsnr")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    assert L.cdc_get_arith(un._handle()) == 1
    rec = _diff(un, "x").decompress(ctx, x.shape, **args)
    assert np.isfinite(rec).all()
    assert un.status() == {"arith": 0, "range_faults": 1, "nonfinite_results": 0}
    un2 = cdc.Unet(**kw)
    un2.load_state_dict(sd)
    _lib.check(un2._handle(), L.cdc_set_arith(un2._handle(), 0))
    ref = _diff(un2, "x").decompress(ctx, x.shape, **args)
    np.testing.assert_array_equal(rec, ref)
    assert un2.status()["range_faults"] == 0


def test_defaults_are_the_ddim_decode_and_eta_is_refused():
    un, _, sd, x, time, ctx, _ = make_unet("small_eps")
    diff = _diff(un, "eps")
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    plain = diff.decompress(ctx, x.shape, sample_steps=4, init=init)
    np.testing.assert_array_equal(plain, diff.decompress(ctx, x.shape, sample_steps=4, init=init, sampler="ddim", spacing="index"))
    np.testing.assert_array_equal(diff.index, SampleSchedule(20000, "linear", "eps", 4).index)
    with pytest.raises(ValueError):
        diff.decompress(ctx, x.shape, sample_steps=4, init=init, eta=0.5, sampler="dpmpp_2m")
    with pytest.raises(ValueError):
        diff.decompress(ctx, x.shape, sample_steps=4, init=init, eta=0.5, seed=3, sampler="dpmpp_2m")
    with pytest.raises(ValueError):
        diff.decompress(ctx, x.shape, sample_steps=4, init=init, sampler="heun")
    # after a solver decode the plain call is the DDIM decode again
    diff.decompress(ctx, x.shape, sample_steps=4, init=init, sampler="dpmpp_2m")
    np.testing.assert_array_equal(plain, diff.decompress(ctx, x.shape, sample_steps=4, init=init))
    # the eps tree under a non-index spacing feeds index / num_timesteps
    diff.decompress(ctx, x.shape, sample_steps=4, init=init, spacing="logsnr")
    np.testing.assert_array_equal(diff._sched.time_in, (diff.index.astype(np.float32) / np.float32(20000)).astype(np.float32))
