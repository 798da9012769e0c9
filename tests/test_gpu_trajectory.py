"""Decode trajectory on the MI355X: x0 and x_t of chosen steps recorded inside the device loop (cdc_set_trace / cdc_trace_read, the
`trajectory=` keywords) against entry points that existed before it, bit for bit: the untraced decode, the stepped chain
(cdc_ddim_step / cdc_solver_step), x0_out of cdc_solver_step, frame.crop(as_uint8=True) -- and the tap kernel alone
(cdc_op_trace_tap) against the float64 statement of tests/sampler_ref.py.

The frames: small_x / small_eps at 32 x 32 and odd_x at 24 x 40 take the four-pixel tap kernel, odd_x's model on 24 x 42 the element
loop.  5 or 6 steps, B = 2 or 3 (CDC_CLIP_HALF splits a batch of 3 into one clipped image and two that are not)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import cdc_compression_amd as cdc
import sampler_ref as R
from cdc_compression_amd import _lib, frame, metrics, synth
from helpers import load_case

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
X0, XT, U8 = _lib.CDC_TRACE_X0, _lib.CDC_TRACE_XT, _lib.CDC_TRACE_U8

CASES = {
    "small_x": dict(model="small_x", tree="x", kw={}, chans=[8, 16], shape=(2, 3, 32, 32), steps=6),
    "small_eps_half": dict(model="small_eps", tree="eps", kw={"clip_noise": "half"}, chans=[3, 16], shape=(3, 3, 32, 32), steps=6),
    "small_eps_none": dict(model="small_eps", tree="eps", kw={"clip_noise": "none"}, chans=[3, 16], shape=(2, 3, 32, 32), steps=5),
    "small_x_noise": dict(model="small_x", tree="x", kw={"pred_mode": "noise"}, chans=[8, 16], shape=(3, 3, 32, 32), steps=5),
    "small_x_v": dict(model="small_x", tree="x", kw={"pred_mode": "v"}, chans=[8, 16], shape=(2, 3, 32, 32), steps=5),
    "odd_x": dict(model="odd_x", tree="x", kw={}, chans=[5], shape=(2, 3, 24, 40), steps=5),
    "24x42": dict(model="odd_x", tree="x", kw={}, chans=[5], shape=(3, 3, 24, 42), steps=6),
}
LOOPS = ("ddim", "seeded", "solver")
SEEDS = [(3 << 33) + 17, 2 ** 64 - 1, 8]
GAMMA, ETA = 0.8, 0.5


def _diff(un, tree, **kw):
    if tree == "x":
        return cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode=kw.get("pred_mode", "x"), var_schedule="cosine")
    return cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise=kw.get("clip_noise", "none"), pred_mode="noise",
                                    var_schedule="linear")


@functools.lru_cache(maxsize=None)
def _setup(case):
    c = CASES[case]
    kw, man, sd, *_ = load_case(c["model"])
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    B, _, H, W = c["shape"]
    diff = _diff(un, c["tree"], **c["kw"])
    clip_denoised = True if c["tree"] == "x" else diff.clip_noise
    return types.SimpleNamespace(un=un, diff=diff, ctx=synth.context_pyramid(c["chans"], B, H, W, seed=3), shape=c["shape"], steps=c["steps"],
                                 init=synth.normal("init", c["shape"], seed=1, std=0.8), clip_denoised=clip_denoised,
                                 clip=diff._clip_flag(clip_denoised), pred=diff._pred_flag(), B=B)


def _loop_args(s, loop):
    """-> (keywords of decompress, the schedule keywords of the loop)."""
    if loop == "ddim":
        return dict(init=s.init), {}
    if loop == "seeded":
        return dict(seed=SEEDS[:s.B], gamma=GAMMA, eta=ETA), {}
    return dict(init=s.init, sampler="dpmpp_2m", spacing="logsnr"), dict(sampler="dpmpp_2m", spacing="logsnr")


@functools.lru_cache(maxsize=None)
def _record(case, loop):
    """One plain decode and the same decode with every step recorded, both kinds, float32: computed once, shared, left unchanged."""
    s = _setup(case)
    args, sched = _loop_args(s, loop)
    common = dict(sample_steps=s.steps, clip_denoised=s.clip_denoised)
    plain = s.diff.decompress(s.ctx, s.shape, **common, **args)
    rec, traj = s.diff.decompress(s.ctx, s.shape, **common, **args, trajectory=1, trajectory_of="both")
    start = s.diff.randn(SEEDS[:s.B], s.shape, draw=0, scale=GAMMA) if loop == "seeded" else s.init
    for t in (plain, rec, traj.x0, traj.x_t):
        t.setflags(write=False)
    return types.SimpleNamespace(plain=plain, rec=rec, traj=traj, start=start, sched=sched)


def _ptrs(ctx):
    return (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in ctx])


def _state_before(r, k):
    """The input of the k-th executed step: the start image, or the recorded state the step before it produced."""
    return np.ascontiguousarray(r.start if k == 0 else r.traj.x_t[k - 1])


# ---- 1. recording changes nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("case", list(CASES))
def test_a_traced_decode_returns_the_bits_of_the_plain_one(case, loop):
    s, r = _setup(case), _record(case, loop)
    assert np.isfinite(r.plain).all()
    np.testing.assert_array_equal(r.rec, r.plain)
    t = r.traj
    assert t.steps == list(range(s.steps - 1, -1, -1)) and len(t) == s.steps
    np.testing.assert_array_equal(t.train_index, np.asarray(s.diff.index)[t.steps])
    assert t.x0.shape == t.x_t.shape == (s.steps,) + tuple(s.shape) and t.x0.dtype == t.x_t.dtype == np.float32
    np.testing.assert_array_equal(t.x_t[-1], r.plain)                  # x_t of index 0 is the decode's result
    assert not np.array_equal(t.x0[0], t.x0[-1]) and not np.array_equal(t.x_t[0], t.x_t[-1])
    if s.clip == _lib.CDC_CLIP_ALL:
        assert np.abs(t.x0).max() <= 1.0
    if s.clip == _lib.CDC_CLIP_HALF:                                     # B = 3: image 0 is clipped, images 1 and 2 are not
        assert np.abs(t.x0[:, :1]).max() <= 1.0 < np.abs(t.x0[:, 1:]).max()


# ---- 2. x_t against the stepped chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("case", list(CASES))
def test_x_t_is_the_stepped_chain_fed_with_the_previous_recorded_state(case, loop):
    s, r = _setup(case), _record(case, loop)
    L, h = _lib.lib(), s.un._handle()
    s.diff.set_sample_schedule(s.steps, **r.sched)
    B, _, H, W = s.shape
    ptrs = _ptrs(s.ctx)
    for k, i in enumerate(r.traj.steps):
        x_in, out = _state_before(r, k), np.full(s.shape, np.nan, np.float32)
        if loop == "solver":
            prev = None if k == 0 else np.ascontiguousarray(r.traj.x0[k - 1])
            x0 = np.empty_like(out)
            _lib.check(h, L.cdc_solver_step(h, x_in.ctypes.data, None if prev is None else prev.ctypes.data, i, ptrs, len(s.ctx),
                                            out.ctypes.data, x0.ctypes.data, B, H, W, s.pred, s.clip, _lib.CDC_MEM_HOST, None))
            np.testing.assert_array_equal(x0, r.traj.x0[k])
        else:
            eta = ETA if loop == "seeded" else 0.0
            nz = s.diff.randn(SEEDS[:B], s.shape, draw=i + 1) if loop == "seeded" else None
            _lib.check(h, L.cdc_ddim_step(h, x_in.ctypes.data, i, ptrs, len(s.ctx), None if nz is None else nz.ctypes.data, eta,
                                          out.ctypes.data, B, H, W, s.pred, s.clip, _lib.CDC_MEM_HOST, None))
        np.testing.assert_array_equal(out, r.traj.x_t[k], err_msg=f"{case} {loop} step {i}")


# ---- 3. x0 against x0_out of cdc_solver_step ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("case", list(CASES))
def test_x0_is_the_x0_out_of_the_solver_step_on_the_recorded_input(case, loop):
    """cdc_solver_step runs the same U-Net program on the same bits and hands out the x0 its update used; with a zero x0_prev it needs
    nothing of the chain.  The solver tables are set on the schedule the loop ran on (they leave its own tables untouched)."""
    s, r = _setup(case), _record(case, loop)
    L, h = _lib.lib(), s.un._handle()
    s.diff.set_sample_schedule(s.steps, sampler="dpmpp_2m", spacing=r.sched.get("spacing", "index"))
    B, _, H, W = s.shape
    ptrs, zeros = _ptrs(s.ctx), np.zeros(s.shape, np.float32)
    for k, i in enumerate(r.traj.steps):
        x_in, out, x0 = _state_before(r, k), np.empty(s.shape, np.float32), np.full(s.shape, np.nan, np.float32)
        _lib.check(h, L.cdc_solver_step(h, x_in.ctypes.data, zeros.ctypes.data, i, ptrs, len(s.ctx), out.ctypes.data, x0.ctypes.data, B, H, W,
                                        s.pred, s.clip, _lib.CDC_MEM_HOST, None))
        np.testing.assert_array_equal(x0, r.traj.x0[k], err_msg=f"{case} {loop} step {i}")
    s.diff.set_sample_schedule(s.steps)


# ---- 4. uint8 slots ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,size", [("small_x", (30, 29)), ("small_x", (32, 32)), ("small_eps_half", (31, 32)), ("24x42", (23, 41)),
                                       ("odd_x", (24, 39))])
def test_uint8_slots_are_the_saved_bytes_of_the_float32_slots(case, size):
    """An image smaller than its frame: the float32 slots come back cropped as the reconstruction is, the uint8 slots were cropped and
    converted inside the tap kernel (x0) and by the crop kernel (x_t)."""
    s = _setup(case)
    h, dev = s.un._handle(), s.un.device_index
    H, W = size
    shape = (s.B, 3, H, W)
    args = dict(sample_steps=s.steps, clip_denoised=s.clip_denoised, init=s.init, trajectory=2, trajectory_of="both")
    rec, f32 = s.diff.decompress(s.ctx, shape, **args)
    rec8, u8 = s.diff.decompress(s.ctx, shape, **args, trajectory_dtype="uint8")
    np.testing.assert_array_equal(rec, rec8)
    np.testing.assert_array_equal(rec, s.diff.decompress(s.ctx, shape, sample_steps=s.steps, clip_denoised=s.clip_denoised, init=s.init))
    S = len(f32)
    assert f32.steps == u8.steps == list(range(s.steps - 1, -1, -2)) + ([0] if (s.steps - 1) % 2 else [])
    for a, b in ((f32.x0, u8.x0), (f32.x_t, u8.x_t)):
        assert a.shape == b.shape == (S, s.B, 3, H, W) and a.dtype == np.float32 and b.dtype == np.uint8
        want = frame.crop(h, a.reshape(S * s.B, 3, H, W), H, W, dev, as_uint8=True).reshape(b.shape)
        np.testing.assert_array_equal(b, want)
    np.testing.assert_array_equal(f32.x_t[-1], rec)
    assert len(np.unique(u8.x0)) > 16                                   # (real pictures, not a constant)


def test_torch_tensors_on_the_device_give_the_same_slots():
    import torch
    s, r = _setup("small_x"), _record("small_x", "ddim")
    dev = torch.device("cuda:0")
    ctx = [torch.from_numpy(c).to(dev) for c in s.ctx]
    rec, t = s.diff.decompress(ctx, s.shape, sample_steps=s.steps, init=torch.from_numpy(s.init).to(dev), trajectory=[0, 4],
                               trajectory_of="both", trajectory_dtype="float32")
    assert t.x0.is_cuda and t.x_t.is_cuda and t.steps == [4, 0]
    pick = [r.traj.steps.index(i) for i in t.steps]
    np.testing.assert_array_equal(t.x0.cpu().numpy(), r.traj.x0[pick])
    np.testing.assert_array_equal(t.x_t.cpu().numpy(), r.traj.x_t[pick])
    np.testing.assert_array_equal(rec.cpu().numpy(), r.plain)


# ---- 5. a subset -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", LOOPS)
def test_a_subset_holds_the_slots_of_the_full_recording(loop):
    s, r = _setup("small_x"), _record("small_x", loop)
    args, _ = _loop_args(s, loop)
    for of in ("both", "x0", "x_t"):
        rec, t = s.diff.decompress(s.ctx, s.shape, sample_steps=s.steps, **args, trajectory=[0, 4] if of == "both" else [4, 0], trajectory_of=of)
        assert t.steps == [4, 0]
        np.testing.assert_array_equal(t.train_index, np.asarray(s.diff.index)[[4, 0]])
        pick = [r.traj.steps.index(4), r.traj.steps.index(0)]
        np.testing.assert_array_equal(rec, r.plain)
        for got, full, on in ((t.x0, r.traj.x0, of != "x_t"), (t.x_t, r.traj.x_t, of != "x0")):
            if on:
                np.testing.assert_array_equal(got, full[pick])
            else:
                assert got is None
    # p_sample_loop takes the keywords too, on the schedule in force
    s.diff.set_sample_schedule(s.steps, **r.sched)
    if loop != "seeded":
        rec, t = s.diff.p_sample_loop(s.shape, s.ctx, True, init=s.init, trajectory=[4], trajectory_of="x0")
        np.testing.assert_array_equal(t.x0[0], r.traj.x0[r.traj.steps.index(4)])
        np.testing.assert_array_equal(rec, r.plain)


# ---- 6. the tap kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles():
    """The two handles of tests/test_gpu_ddim_update.py: small_x's model with sampler_ref.schedules()' tables (the U-Net never runs)."""
    out = {}
    for tree in ("x", "eps"):
        kw, man, sd, *_ = load_case("small_x")
        un = cdc.Unet(**kw)
        un.load_state_dict(sd)
        diff = _diff(un, tree, pred_mode="v")
        diff.set_sample_schedule(R.STEPS)
        np.testing.assert_array_equal(diff._sched.sqrt_recip, R.schedules()[tree].sqrt_recip)
        out[tree] = (un, diff, diff._sched)
    return out


def _tap(un, i, fx, x, pred, clip, planes=None, bias=None, pad=0, win=None):
    """cdc_op_trace_tap on host arrays -> x0 float32 of x's shape, or (win) the uint8 window."""
    L, h = _lib.lib(), un._handle()
    B, C, H, W = x.shape
    out = np.full(x.shape, np.nan, np.float32) if win is None else np.full((B, C) + tuple(win), 77, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data                # noqa: E731
    _lib.check(h, L.cdc_op_trace_tap(h, p(fx), x.ctypes.data, i, out.ctypes.data, B, C, H, W, pred, clip,
                                     _lib.CDC_ELEM_F32 if win is None else _lib.CDC_ELEM_U8, *(win or (0, 0)), p(planes), p(bias),
                                     0 if planes is None else planes.shape[2], pad, _lib.CDC_MEM_HOST, None))
    return out


@pytest.mark.parametrize("shape", R.SHAPES)
def test_tap_against_float64(handles, shape):
    """|x0 - float64| <= e0 of sampler_ref.predict_x0_f64 (two products and a difference, each rounded once; the clamp is exact), and
    the very bits of fx for pred_mode x."""
    fx, x, _ = R.inputs(shape)
    worst = 0.0
    for pred, clip, _eta in ([c for c in R.combos(shape) if c[2] == R.ETAS[0]] if tuple(shape) != R.BIG else R.BIG_COMBOS):
        un, _, s = handles[R.tree_of(pred)]
        for i in R.STEP_LIST:
            got = _tap(un, i, fx, x, pred, clip)
            ref, e0 = R.predict_x0_f64(s, i, fx.astype(np.float64), x.astype(np.float64), pred, clip)
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= e0), (pred, clip, i, float(err.max()))
            if pred == R.PRED_X:
                np.testing.assert_array_equal(got, ref.astype(np.float32))
            else:
                worst = max(worst, float((err / np.maximum(e0, 1e-300)).max()))
            nclip = R.n_clipped(shape[0], clip)
            assert np.abs(got[:nclip]).max(initial=0.0) <= 1.0
    print(f"{shape}: worst error / e0 = {worst:.3f}")


def test_tap_forms_and_traversals_hold_the_same_bits(handles):
    """fx against the planes of the fused combine; the four-pixel kernel (W = 44, and as two long rows) against the element loop (a width
    of 6; pointers one float off a 16-byte boundary); device tensors, in place (out = x) in either kernel; uint8 windows against
    frame.crop(as_uint8=True) of the float32 result, word stores (window width a multiple of 4) and byte stores."""
    import torch
    shape = (3, 3, 24, 44)
    B, C, H, W = shape
    n = int(np.prod(shape))
    KH, pad = 7, 3
    planes = synth.normal("planes", (B, C, KH, H, W), seed=8, std=0.5)
    bias = synth.normal("bias", (C,), seed=9, std=0.3)
    fx, _ = R.combine(planes, bias, pad)
    _, x, _ = R.inputs(shape, seed=6)
    flat, odd = (1, 1, 2, n // 2), (1, 1, n // 6, 6)
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for pred, clip in ((R.PRED_V, R.CLIP_HALF), (R.PRED_NOISE, R.CLIP_NONE), (R.PRED_X, R.CLIP_ALL), (R.PRED_NOISE_XTREE, R.CLIP_ALL)):
        un, _, s = handles[R.tree_of(pred)]
        h = un._handle()
        a = _tap(un, 2, fx, x, pred, clip)
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, _tap(un, 2, None, x, pred, clip, planes=planes, bias=bias, pad=pad))
        if clip != R.CLIP_HALF:                                        # (reshaped, "the first half of the batch" is another set)
            np.testing.assert_array_equal(a.ravel(), _tap(un, 2, fx.reshape(flat), x.reshape(flat), pred, clip).ravel())
            np.testing.assert_array_equal(a.ravel(), _tap(un, 2, fx.reshape(odd), x.reshape(odd), pred, clip).ravel())
        # the element loop over the same frame: planes and x one float off a 16-byte boundary; and in place
        for off in (0, 1):
            buf = [torch.zeros(n * k + 4, device=dev) for k in (KH, 1, 1)]
            assert all(t.data_ptr() % 16 == 0 for t in buf)
            tP, tx, tfx = (t[off:off + n * k] for t, k in zip(buf, (KH, 1, 1)))
            tP.copy_(torch.from_numpy(planes.ravel()))
            tx.copy_(torch.from_numpy(x.ravel()))
            tfx.copy_(torch.from_numpy(fx.ravel()))
            tb = torch.from_numpy(bias).to(dev)
            out = torch.full((n + 2,), 5.0, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(h, L.cdc_op_trace_tap(h, None, tx.data_ptr(), 2, out[1:].data_ptr(), B, C, H, W, pred, clip, _lib.CDC_ELEM_F32, 0, 0,
                                             tP.data_ptr(), tb.data_ptr(), KH, pad, _lib.CDC_MEM_DEVICE, st))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out[1:n + 1].cpu().numpy().reshape(shape), a)
            assert float(out[0]) == 5.0 and float(out[n + 1]) == 5.0     # nothing written beside the n elements
            _lib.check(h, L.cdc_op_trace_tap(h, tfx.data_ptr(), tx.data_ptr(), 2, tx.data_ptr(), B, C, H, W, pred, clip, _lib.CDC_ELEM_F32, 0, 0,
                                             None, None, 0, 0, _lib.CDC_MEM_DEVICE, st))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(tx.cpu().numpy().reshape(shape), a)
            assert float(buf[1][off + n:].abs().max()) == 0.0
        # uint8 windows
        for win in ((24, 44), (20, 24), (24, 41), (1, 1), (7, 3)):
            want = frame.crop(h, a.reshape(B * C // 3, 3, H, W), *win, un.device_index, as_uint8=True).reshape((B, C) + win)
            np.testing.assert_array_equal(_tap(un, 2, fx, x, pred, clip, win=win), want)
            np.testing.assert_array_equal(_tap(un, 2, None, x, pred, clip, planes=planes, bias=bias, pad=pad, win=win), want)
        # ... and from the element loop (a frame 42 wide)
    shape = (3, 3, 24, 42)
    fx, x, _ = R.inputs(shape, seed=7)
    un, _, s = handles["x"]
    a = _tap(un, 4, fx, x, R.PRED_V, R.CLIP_HALF)
    for win in ((24, 42), (24, 40), (5, 41)):
        want = frame.crop(un._handle(), a, *win, un.device_index, as_uint8=True)
        np.testing.assert_array_equal(_tap(un, 4, fx, x, R.PRED_V, R.CLIP_HALF, win=win), want)


# ---- 7. what a trace launches ------------------------------------------------------------------------------------------------------------
def _launches(h):
    L = _lib.lib()
    total, k = 0, ctypes.c_int64()
    for c in range(L.cdc_prof_num_classes()):
        _lib.check(h, L.cdc_prof_get(h, c, None, ctypes.byref(k), None, None))
        total += k.value
    return total


@pytest.mark.parametrize("loop", LOOPS)
def test_a_trace_adds_one_launch_per_x0_slot_and_the_x_t_captures(loop):
    """float32 x_t slots are device-to-device copies (no kernel); uint8 x_t slots are one launch of the crop kernel each."""
    s = _setup("small_x")
    L, h = _lib.lib(), s.un._handle()
    args, _ = _loop_args(s, loop)
    args = dict(sample_steps=s.steps, **args)
    L.cdc_prof_enable(h, 1)
    try:
        def count(**kw):
            L.cdc_prof_reset(h)
            s.diff.decompress(s.ctx, s.shape, **args, **kw)
            return _launches(h)
        plain = count()
        assert plain > s.steps * 10
        assert count() == plain
        assert count(trajectory=1) == plain + s.steps
        assert count(trajectory=[4, 0]) == plain + 2
        assert count(trajectory=[4, 0], trajectory_of="x_t") == plain
        assert count(trajectory=[4, 0], trajectory_of="both") == plain + 2
        assert count(trajectory=[4, 0], trajectory_of="both", trajectory_dtype="uint8") == plain + 4
        assert count(trajectory=2, trajectory_of="x_t", trajectory_dtype="uint8") == plain + len(range(s.steps - 1, -1, -2)) + (s.steps - 1) % 2
        assert count() == plain                                          # the trace is gone with the call
    finally:
        L.cdc_prof_enable(h, 0)
        L.cdc_prof_reset(h)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    s = _setup("small_x")
    L, h = _lib.lib(), s.un._handle()
    s.diff.set_sample_schedule(s.steps)
    B, _, H, W = s.shape
    ptrs = _ptrs(s.ctx)
    out = np.full(s.shape, 7.0, np.float32)
    sd = np.asarray(SEEDS[:B], dtype=np.uint64)
    ints = lambda v: (ctypes.c_int * len(v))(*v)                      # noqa: E731
    decode = lambda hh=H, ww=W: L.cdc_decode(h, s.init.ctypes.data, ptrs, len(s.ctx), out.ctypes.data, B, hh, ww, s.pred, s.clip,   # noqa: E731
                                             _lib.CDC_MEM_HOST, None)
    err = lambda: L.cdc_last_error(h).decode()                        # noqa: E731
    L.cdc_prof_enable(h, 1)
    L.cdc_prof_reset(h)
    try:
        # cdc_set_trace's own arguments
        assert L.cdc_set_trace(h, ints([0]), 1, 0, 0, 0) == _lib_err("INVALID") and L.cdc_set_trace(h, ints([0]), 1, U8, 0, 0) != 0
        assert L.cdc_set_trace(h, ints([0]), 1, 8 | X0, 0, 0) != 0 and L.cdc_set_trace(h, None, 1, X0, 0, 0) != 0
        assert L.cdc_set_trace(h, ints([0]), -1, X0, 0, 0) != 0 and L.cdc_set_trace(h, ints([0]), 1, X0, -1, 0) != 0
        # an index outside the schedule in force, and one given twice: refused at the decode, naming the index
        for bad, word in (([5, s.steps], f"index {s.steps} "), ([-1], "index -1 "), ([3, 1, 3], "index 3 ")):
            assert L.cdc_set_trace(h, ints(bad), len(bad), X0 | XT, 0, 0) == 0
            assert decode() == _lib_err("INVALID") and word in err(), err()
        # a window outside the frame
        assert L.cdc_set_trace(h, ints([0]), 1, X0 | U8, H + 1, W) == 0
        assert decode() == _lib_err("INVALID") and "window" in err()
        # cdc_decode_samples with a trace set
        assert L.cdc_set_trace(h, ints([0]), 1, X0, 0, 0) == 0
        two = np.full((2 * B,) + tuple(s.shape[1:]), 7.0, np.float32)
        sd2 = np.asarray(SEEDS[:B] * 2, dtype=np.uint64)
        rc = L.cdc_decode_samples(h, GAMMA, sd2.ctypes.data_as(U64P), ETA, ptrs, len(s.ctx), two.ctypes.data, B, 2, H, W, s.pred, s.clip, 0,
                                  _lib.CDC_MEM_HOST, None)
        assert rc == _lib_err("INVALID") and "trace" in err() and np.all(two == 7.0)
        # an oversize request, computed from the arguments and never allocated: every step of a 65536 x 65536 frame, both kinds
        big = 65536
        idx = list(range(s.steps))
        assert L.cdc_set_trace(h, ints(idx), len(idx), X0 | XT, 0, 0) == 0
        slot = B * 3 * big * big * 4
        total = slot * s.steps * 2
        assert total > 2 ** 40
        assert decode(big, big) == _lib_err("NOMEM"), err()
        assert str(total) in err() and str(slot) in err() and "2^40" in err(), err()
        # nothing ran, nothing is recorded
        assert _launches(h) == 0 and np.all(out == 7.0)
        info = [ctypes.c_int(-1) for _ in range(6)]
        assert L.cdc_trace_info(h, *[ctypes.byref(c) for c in info]) == 0 and info[0].value == 0
        assert L.cdc_trace_read(h, X0, 0, 1, out.ctypes.data, _lib.CDC_MEM_HOST, None) == _lib_err("STATE")
        # a good request after all that: it records, and cdc_trace_read checks its own arguments
        assert L.cdc_set_trace(h, ints([0, 4]), 2, X0, 0, 0) == 0
        assert decode() == 0 and np.isfinite(out).all()
        assert L.cdc_trace_info(h, *[ctypes.byref(c) for c in info]) == 0
        assert [c.value for c in info] == [2, B, 3, H, W, X0]
        slot0 = np.empty(s.shape, np.float32)
        assert L.cdc_trace_read(h, X0, 0, 1, slot0.ctypes.data, _lib.CDC_MEM_HOST, None) == 0
        np.testing.assert_array_equal(slot0, _record("small_x", "ddim").traj.x0[1])          # index 4 of 6 steps: the second slot
        for kind, a, n in ((XT, 0, 1), (X0 | XT, 0, 1), (X0, 2, 1), (X0, 1, 2), (X0, -1, 1), (X0, 0, 0)):
            assert L.cdc_trace_read(h, kind, a, n, slot0.ctypes.data, _lib.CDC_MEM_HOST, None) == _lib_err("INVALID"), (kind, a, n)
        assert L.cdc_set_trace(h, None, 0, 0, 0, 0) == 0
    finally:
        L.cdc_set_trace(h, None, 0, 0, 0, 0)
        L.cdc_prof_enable(h, 0)
        L.cdc_prof_reset(h)
    # the mirror clears the trace on error too: a decode that fails inside the library, then one that a set trace would refuse
    with pytest.raises(_lib.CdcError):
        s.diff.decompress(s.ctx[:1], s.shape, sample_steps=s.steps, init=s.init, trajectory=1)
    k = s.diff.decompress(s.ctx, s.shape, sample_steps=s.steps, seed=SEEDS[:B], gamma=GAMMA, samples=2)
    assert k.shape == (B, 2) + tuple(s.shape[1:])


def _lib_err(name):
    return {"INVALID": -1, "STATE": -2, "HIP": -3, "UNSUPPORTED": -4, "NOMEM": -5}[name]


# ---- 9. evaluate() ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["x", "eps"])
def test_evaluate_scores_every_slot_with_the_metric_calls(tag):
    import metrics_ref as MR
    from test_gpu_metrics import _bits, _small
    diff, kw = _small(tag)
    un = diff.denoise_fn
    images = MR.as_u8(MR.picture(2, 176, 203))
    ev = diff.evaluate(images, sample_steps=3, trajectory=[2, 0], **kw)
    rec, bpp, traj = diff.compress(images, sample_steps=3, bpp_return_mean=False, trajectory=[2, 0], **kw)
    plain, _ = diff.compress(images, sample_steps=3, bpp_return_mean=False, **kw)
    np.testing.assert_array_equal(rec, plain)
    np.testing.assert_array_equal(ev["reconstruction"], plain)
    tr = ev["trajectory"]
    assert tr["steps"] == traj.steps == [2, 0] and tr["of"] == "x0" and traj.x_t is None
    assert traj.x0.shape == (2, 2, 3, 176, 203)
    np.testing.assert_array_equal(tr["trajectory"].x0, traj.x0)
    for k in range(2):
        assert np.array_equal(_bits(tr["psnr"][k]), _bits(metrics.psnr(un, traj.x0[k], images, as_saved=True)))
        assert np.array_equal(_bits(tr["ms_ssim"][k]), _bits(metrics.ms_ssim(un, traj.x0[k], images, as_saved=True)))
        assert tr["psnr"][k].shape == (2,) and np.all(np.isfinite(tr["psnr"][k]))
    assert "lpips" not in tr
    small = diff.evaluate(images[:, :, :100, :120], sample_steps=3, trajectory=3, trajectory_of="x_t", **kw)
    assert small["trajectory"]["ms_ssim"] is None and small["trajectory"]["of"] == "x_t" and small["trajectory"]["steps"] == [2, 0]
    np.testing.assert_array_equal(small["trajectory"]["trajectory"].x_t[-1], small["reconstruction"])
    assert np.array_equal(_bits(small["trajectory"]["psnr"][-1]), _bits(small["psnr"]))
    assert sorted(diff.evaluate(images[:, :, :100, :120], sample_steps=3, **kw)) == ["bpp", "ms_ssim", "psnr", "reconstruction"]


# ---- 10. the example script ----------------------------------------------------------------------------------------------------------
def test_example_script_saves_the_previews_when_asked(tmp_path):
    """--trajectory 2 over 3 steps: name.step0002.png and name.step0000.png beside the image, the printed lines as without the flag
    (tests/test_gpu_metrics.py pins those).  At sample index 0 the DDIM update is x_t = 1 * x0 + 0 * eps (eta = 0), so the last preview
    is the saved image byte for byte."""
    import os
    import subprocess
    import sys
    import metrics_ref as MR
    Image = pytest.importorskip("PIL.Image")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(MR.as_u8(MR.picture(1, 70, 91))[0].transpose(1, 2, 0)).save(src / "a.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                        "--n_denoise_step", "3", "--img_dir", str(src), "--out_dir", str(out), "--trajectory", "2"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, CDC_SYNTHETIC_INIT="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0] == "image: a.png" and lines[1].startswith("bpp:")
    assert sorted(os.listdir(out)) == ["a.png", "a.step0000.png", "a.step0002.png"]
    img = {n: np.asarray(Image.open(out / n).convert("RGB")) for n in os.listdir(out)}
    assert all(v.shape == (70, 91, 3) for v in img.values())
    np.testing.assert_array_equal(img["a.step0000.png"], img["a.png"])
    assert not np.array_equal(img["a.step0002.png"], img["a.png"])


# ---- 11. the range guard ---------------------------------------------------------------------------------------------------------------
def test_the_bf16x3_repetition_records_again_from_the_start():
    """The heavy-tail "overflow" fixture leaves the fp16 range (tests/test_gpu_solver.py runs the same decode without a trace): the
    decode is repeated in CDC_ARITH_BF16X3 and the trace is that of the returned image -- slot for slot what a handle records that was
    in that arithmetic from the start."""
    from test_oracle import heavy_tail_case
    kw, sd, x, time, ctx, *_ = heavy_tail_case("overflow")
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    L = _lib.lib()
    args = dict(sample_steps=5, init=init, sampler="dpmpp_2m", spacing="logsnr", trajectory=1, trajectory_of="both")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    assert L.cdc_get_arith(un._handle()) == 1
    rec, t = _diff(un, "x").decompress(ctx, x.shape, **args)
    assert un.status() == {"arith": 0, "range_faults": 1, "nonfinite_results": 0}
    assert np.isfinite(rec).all() and np.isfinite(t.x0).all() and np.isfinite(t.x_t).all()
    np.testing.assert_array_equal(t.x_t[-1], rec)
    un2 = cdc.Unet(**kw)
    un2.load_state_dict(sd)
    _lib.check(un2._handle(), L.cdc_set_arith(un2._handle(), 0))
    rec2, t2 = _diff(un2, "x").decompress(ctx, x.shape, **args)
    assert un2.status()["range_faults"] == 0
    np.testing.assert_array_equal(rec, rec2)
    np.testing.assert_array_equal(t.x0, t2.x0)
    np.testing.assert_array_equal(t.x_t, t2.x_t)
