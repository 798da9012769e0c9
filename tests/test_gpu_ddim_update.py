"""The DDIM update of the sampler kernels alone (cdc_op_ddim_update) on the MI355X, against the float64 statement and the derived bound
of tests/sampler_ref.py: every pred_mode, clip and noise source, the steps a decode starts and ends with, both traversals and the
conditions that select them, the seeded rule, the in-kernel row combine of the final convolution's planes, and the refusals.

Two handles, both of small_x's model (the U-Net never runs): one holds a 5-step cosine x-tree schedule with the tables of pred_mode
"v", the other a 5-step linear eps-tree schedule.  pred_mode 1 (the eps tree's "noise") runs on the second, the rest on the first.

The frames: (3,3,24,44) four-pixel kernel, two blocks per plane; (3,3,24,42) scalar kernel; (2,3,4,4) less than one wave; (3,3,5,7)
105 elements per image: the last quad of an image's draws is partial; (3,3,344,342) the scalar kernel's grid-stride loop (more than
4096 * 256 elements); (1,65540,1,4) more than 65535 planes: a width of 4 in the scalar kernel."""
import ctypes

import numpy as np
import pytest

import cdc_compression_amd as cdc
import sampler_ref as R
from cdc_compression_amd import _lib, synth
from test_gpu_parity import make_unet

pytestmark = pytest.mark.gpu

U = R.U
U64P = ctypes.POINTER(ctypes.c_uint64)
LIBM = 1e-5           # include/cdc_hip.h: host (cdc_randn_host) and device draws differ by their libm only, by at most this


@pytest.fixture(scope="module")
def handles():
    """-> {"x": (unet, diffusion, schedule), "eps": ...}; the schedules are those of sampler_ref.schedules(), table for table."""
    out = {}
    for tree in ("x", "eps"):
        un, *_ = make_unet("small_x")
        if tree == "x":
            diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="v", var_schedule="cosine")
        else:
            diff = cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear")
        diff.set_sample_schedule(R.STEPS)
        want = R.schedules()[tree]
        for name in ("sqrt_recip", "sqrt_recipm1", "sqrt_ac_prev", "one_minus_ac_prev", "sigma", "sqrt_ac", "sqrt_one_minus_ac"):
            np.testing.assert_array_equal(getattr(diff._sched, name), getattr(want, name))
        out[tree] = (un, diff, diff._sched)
    return out


def _of(handles, pred):
    un, _, s = handles[R.tree_of(pred)]
    return un, s


def _op(un, i, fx, x, noise, eta, pred, clip, seeds=None, planes=None, bias=None, pad=0):
    """cdc_op_ddim_update on host arrays -> x_next."""
    L, h = _lib.lib(), un._handle()
    xn = np.full_like(x, np.nan)
    B, C, H, W = x.shape
    p = lambda a: None if a is None else a.ctypes.data                # noqa: E731
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
    _lib.check(h, L.cdc_op_ddim_update(h, p(fx), x.ctypes.data, p(noise), None if sd is None else sd.ctypes.data_as(U64P), eta, i,
                                       xn.ctypes.data, B, C, H, W, pred, clip, p(planes), p(bias),
                                       0 if planes is None else planes.shape[2], pad, _lib.CDC_MEM_HOST, None))
    return xn


def _op_dev(un, i, fx, x, noise, eta, pred, clip, xn, shape, seeds=None):
    """... on device tensors (torch), as they are: no copy, whatever their alignment."""
    import torch
    L, h = _lib.lib(), un._handle()
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(h, L.cdc_op_ddim_update(h, fx.data_ptr(), x.data_ptr(), None if noise is None else noise.data_ptr(),
                                       None if sd is None else sd.ctypes.data_as(U64P), eta, i, xn.data_ptr(), *shape, pred, clip,
                                       None, None, 0, 0, _lib.CDC_MEM_DEVICE, st))
    torch.cuda.synchronize()
    return xn.cpu().numpy().reshape(shape)


def _randn_host(seeds, shape, draw):
    z = np.empty(shape, np.float32)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert _lib.lib().cdc_randn_host(sd.ctypes.data_as(U64P), shape[0], int(np.prod(shape[1:])), draw, 1.0, z.ctypes.data) == 0
    return z


def _randn_dev(un, seeds, shape, draw):
    """The fill kernel's draws (cdc_randn): the device's own evaluation of the generator."""
    z = np.empty(shape, np.float32)
    h = un._handle()
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    _lib.check(h, _lib.lib().cdc_randn(h, sd.ctypes.data_as(U64P), shape[0], int(np.prod(shape[1:])), draw, 1.0, z.ctypes.data,
                                       _lib.CDC_MEM_HOST, None))
    return z


# ---- against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_update_against_float64(handles, shape):
    """|x_next - float64| <= sampler_ref.ddim_update_f64's bound, element by element; and -- nothing in the update is fused, the
    division and the square root round correctly -- the very bits of the float32 operation-by-operation evaluation, for one of the two
    ways the compiler may contract the step's scalar var = one_minus_ac_prev - sig^2."""
    fx, x, nz = R.inputs(shape)
    worst, which = 0.0, [0, 0]
    for pred, clip, eta in R.combos(shape):
        un, s = _of(handles, pred)
        for i in R.STEP_LIST:
            noise = nz if eta else None
            got = _op(un, i, fx, x, noise, eta, pred, clip)
            ref, bound = R.ddim_update_f64(s, i, fx, x, noise, eta, pred, clip)
            err = np.abs(got.astype(np.float64) - ref)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            assert np.all(err <= bound), (pred, clip, eta, i, ratio)
            worst = max(worst, ratio)
            cands = R.step_scalars(s, i, eta, pred)["c_eps"]
            same = [np.array_equal(got, R.ddim_update_f32(s, i, fx, x, noise, eta, pred, clip, c_eps=c)) for c in cands]
            assert any(same), (pred, clip, eta, i, "the bits of neither float32 evaluation")
            if cands[0] != cands[1]:
                which[same.index(True)] += 1
    print(f"{shape}: worst error / bound = {worst:.3f}; where the two contractions of var differ: the rounded product {which[0]} times, "
          f"the exact one {which[1]} times")


@pytest.mark.parametrize("shape", [(3, 3, 24, 44), (3, 3, 5, 7)])
def test_variance_below_zero(handles, shape):
    """eta > 1: var < 0.  The x tree clamps it (c_eps = 0 exactly: the statement with c_eps = 0), the eps tree takes the root of a
    negative number as the reference does: NaN everywhere, and nothing but NaN."""
    fx, x, nz = R.inputs(shape)
    i, eta = R.OVER_STEP, R.ETA_OVER
    for pred in R.PREDS:
        un, s = _of(handles, pred)
        for clip in R.CLIPS:
            got = _op(un, i, fx, x, nz, eta, pred, clip)
            if pred == R.PRED_NOISE:
                assert np.isnan(got).all(), (pred, clip)
                continue
            k = R.step_scalars(s, i, eta, pred)
            assert k["c_eps64"] == 0 and k["dc"] == 0
            ref, bound = R.ddim_update_f64(s, i, fx, x, nz, eta, pred, clip)
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= bound), (pred, clip, float((err / np.maximum(bound, 1e-300)).max()))
            np.testing.assert_array_equal(got, R.ddim_update_f32(s, i, fx, x, nz, eta, pred, clip))
    # the handle is as it was: an ordinary update after the NaN one
    un, s = _of(handles, R.PRED_NOISE)
    assert np.isfinite(_op(un, i, fx, x, nz, 0.5, R.PRED_NOISE, R.CLIP_NONE)).all()


# ---- the seeded rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 24, 44), (3, 3, 24, 42), (3, 3, 5, 7)])
def test_seeded_equals_the_tensor_of_its_draws(handles, shape):
    """seeds in the kernel against noise = z(seeds, draw i + 1) as a tensor.  Device kernels evaluate the generator to the same bits
    (include/cdc_hip.h), so against the fill kernel's tensor (cdc_randn) the update is the same bit for bit.  The host statement
    (cdc_randn_host) goes through another libm and is stated to differ by up to 1e-5 per draw: against its tensor the update differs by
    at most sig (|dz| + 2 U |z|) + 2 U |x_next| -- the draw's difference scaled, the product and the last sum rounded on either side --
    and where the two libms gave a draw the same bits, the update holds the same bits too."""
    fx, x, _ = R.inputs(shape)
    seeds = [(9 << 32) + 5, 2 ** 64 - 3, (1 << 40) + 123456789][:shape[0]]
    eta = 0.5
    for pred in R.PREDS:
        un, s = _of(handles, pred)
        for clip, i in ((R.CLIP_HALF, 4), (R.CLIP_ALL, 2), (R.CLIP_NONE, 0)):
            got = _op(un, i, fx, x, None, eta, pred, clip, seeds=seeds)
            zd = _randn_dev(un, seeds, shape, i + 1)
            np.testing.assert_array_equal(got, _op(un, i, fx, x, zd, eta, pred, clip))
            assert not np.array_equal(zd, _randn_dev(un, seeds, shape, i))              # (another draw is another tensor)
            zh = _randn_host(seeds, shape, i + 1)
            dz = np.abs(zd.astype(np.float64) - zh)
            assert dz.max() <= LIBM
            via_host = _op(un, i, fx, x, zh, eta, pred, clip)
            sig = float(R.step_scalars(s, i, eta, pred)["sig"])
            diff = np.abs(got.astype(np.float64) - via_host)
            moved = sig * (dz + 2 * U * (np.abs(zh) + dz))                       # |fl(sig z_device) - fl(sig z_host)|
            assert np.all(diff <= moved + 2 * U * (np.abs(via_host) + moved)), (pred, clip, i)
            np.testing.assert_array_equal(got[dz == 0], via_host[dz == 0])
            if pred == R.PRED_X:
                print(f"{shape} draw {i + 1}: host and device draws differ in {int((dz != 0).sum())} of {dz.size} elements, max {dz.max():.2e}")


# ---- the forms ---------------------------------------------------------------------------------------------------------------------
def test_forms_hold_the_same_bits(handles):
    """The same elements through the four-pixel kernel (W = 44, and as two long rows) and, at a width of 6, through the scalar one; the
    seeded rule, whose draws follow the image layout, through the four-pixel kernel and -- from pointers one float off a 16-byte
    boundary -- through the scalar one."""
    import torch
    shape = (2, 3, 24, 44)
    n = int(np.prod(shape))
    fx, x, nz = R.inputs(shape, seed=6)
    flat, odd = (1, 1, 2, n // 2), (1, 1, n // 6, 6)
    seeds = [(3 << 32) + 1, (1 << 63) + 2]
    dev = torch.device("cuda:0")
    for pred, clip in ((R.PRED_V, R.CLIP_ALL), (R.PRED_NOISE, R.CLIP_NONE), (R.PRED_X, R.CLIP_ALL)):
        un, s = _of(handles, pred)
        for eta in (0.0, 0.5):
            noise = nz if eta else None
            r = lambda t, sh: None if t is None else t.reshape(sh)        # noqa: E731
            a = _op(un, 2, fx, x, noise, eta, pred, clip)
            b = _op(un, 2, r(fx, flat), r(x, flat), r(noise, flat), eta, pred, clip)
            c = _op(un, 2, r(fx, odd), r(x, odd), r(noise, odd), eta, pred, clip)
            np.testing.assert_array_equal(a.ravel(), b.ravel())
            np.testing.assert_array_equal(a.ravel(), c.ravel())
        four = _op(un, 2, fx, x, None, 0.5, pred, clip, seeds=seeds)
        buf = [torch.zeros(n + 4, device=dev) for _ in range(3)]
        assert all(t.data_ptr() % 16 == 0 for t in buf)
        tfx, tx, tn = (t[1:n + 1] for t in buf)
        tfx.copy_(torch.from_numpy(fx.ravel()))
        tx.copy_(torch.from_numpy(x.ravel()))
        assert tx.data_ptr() % 16 == 4
        np.testing.assert_array_equal(four, _op_dev(un, 2, tfx, tx, None, 0.5, pred, clip, tn, shape, seeds=seeds))
        assert buf[2][0] == 0 and bool((buf[2][n + 1:] == 0).all())      # nothing written beside the n elements


def test_alignment_fallback_and_in_place_on_the_device(handles):
    """Each of x, x_next and noise in turn one float off a 16-byte boundary (the launch then takes the scalar kernel: the `& 15` test of
    sampler_launch), and x_next = x, which is what the decode loop does."""
    import torch
    shape = (2, 3, 24, 44)
    n = int(np.prod(shape))
    fx, x, nz = R.inputs(shape, seed=7)
    dev = torch.device("cuda:0")

    def tensor(a, off):
        t = torch.zeros(n + 4, device=dev)
        assert t.data_ptr() % 16 == 0
        v = t[off:off + n]
        if a is not None:
            v.copy_(torch.from_numpy(a.ravel()))
        return v
    for pred, clip in ((R.PRED_V, R.CLIP_HALF), (R.PRED_NOISE, R.CLIP_ALL)):
        un, s = _of(handles, pred)
        want = _op(un, 2, fx, x, nz, 0.5, pred, clip)
        for off in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            tfx, tx, tn, tz = tensor(fx, 0), tensor(x, off[0]), tensor(None, off[1]), tensor(nz, off[2])
            assert [t.data_ptr() % 16 for t in (tx, tn, tz)] == [4 * o for o in off]
            np.testing.assert_array_equal(_op_dev(un, 2, tfx, tx, tz, 0.5, pred, clip, tn, shape), want)
        for o in (0, 1):                                              # in place, in either kernel
            tfx, tx, tz = tensor(fx, 0), tensor(x, o), tensor(nz, 0)
            np.testing.assert_array_equal(_op_dev(un, 2, tfx, tx, tz, 0.5, pred, clip, tx, shape), want)


# ---- the row combine inside the sampler kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4, 44), (2, 3, 7, 42), (2, 3, 24, 44)])
@pytest.mark.parametrize("KH,pad", [(7, 3), (3, 1)])
def test_fused_combine_against_an_independent_sum(handles, shape, KH, pad):
    """planes [B][C][KH][H][W] (+ bias) in place of fx.  The expected fx is summed by NumPy in float32 -- the bias, then ky ascending over
    the rows inside the image: additions only, so its bits are defined -- and the update from the planes equals the update from that
    tensor bit for bit.  The float32 sum itself agrees with the float64 one to KH U sum |terms| (KH additions)."""
    B, C, H, W = shape
    planes = synth.normal("planes", (B, C, KH, H, W), seed=8, std=0.5)
    bias = synth.normal("bias", (C,), seed=9, std=0.3)
    _, x, nz = R.inputs(shape, seed=8)
    for b in (bias, None):
        fx, _ = R.combine(planes, b, pad)
        fx64, mag = R.combine(planes, b, pad, np.float64)
        assert fx.dtype == np.float32 and np.all(np.abs(fx.astype(np.float64) - fx64) <= KH * U * mag)
        for pred, clip, eta, i in ((R.PRED_X, R.CLIP_ALL, 0.5, 2), (R.PRED_NOISE, R.CLIP_HALF, 0.0, 4), (R.PRED_V, R.CLIP_NONE, 1.0, 0)):
            un, s = _of(handles, pred)
            noise = nz if eta else None
            want = _op(un, i, fx, x, noise, eta, pred, clip)
            got = _op(un, i, None, x, noise, eta, pred, clip, planes=planes, bias=b, pad=pad)
            np.testing.assert_array_equal(got, want)
            assert np.isfinite(got).all()
    # the seeded rule reads the planes too
    un, s = _of(handles, R.PRED_X)
    seeds = [(5 << 32) + 7, (6 << 32) + 8]
    fx, _ = R.combine(planes, bias, pad)
    np.testing.assert_array_equal(_op(un, 2, None, x, None, 0.5, R.PRED_X, R.CLIP_ALL, seeds=seeds, planes=planes, bias=bias, pad=pad),
                                  _op(un, 2, fx, x, None, 0.5, R.PRED_X, R.CLIP_ALL, seeds=seeds))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(handles):
    L = _lib.lib()
    un, s = _of(handles, R.PRED_X)
    un_e, _ = _of(handles, R.PRED_NOISE)
    z = np.zeros((1, 3, 4, 4), np.float32)
    P = np.zeros((1, 3, 3, 4, 4), np.float32)
    out = np.full_like(z, 7.0)
    sd = np.array([1], np.uint64).ctypes.data_as(U64P)
    p = z.ctypes.data

    def call(h=None, fx=p, noise=None, seeds=None, eta=0.0, i=2, pred=0, clip=0, planes=None, KH=0, pad=0, B=1):
        return L.cdc_op_ddim_update(un._handle() if h is None else h, fx, p, noise, seeds, eta, i, out.ctypes.data, B, 3, 4, 4, pred, clip,
                                    planes, None, KH, pad, _lib.CDC_MEM_HOST, None)
    assert call() == 0 and np.all(out == 0)
    out[:] = 7.0
    assert call(i=R.STEPS) != 0 and call(i=-1) != 0                                   # step index out of range
    assert call(eta=0.5) != 0 and b"eta" in L.cdc_last_error(un._handle())            # eta != 0 without noise
    assert call(eta=0.5, noise=p, seeds=sd) != 0 and call(noise=p, seeds=sd) != 0    # both noise sources
    assert call(eta=float("nan"), noise=p) != 0 and call(eta=float("inf"), noise=p) != 0
    assert call(planes=P.ctypes.data, KH=3, pad=1) != 0                               # planes together with fx
    assert call(fx=None) != 0                                                         # neither
    assert call(fx=None, planes=P.ctypes.data, KH=3, pad=3) != 0                      # pad >= KH
    assert call(fx=None, planes=P.ctypes.data, KH=3, pad=-1) != 0 and call(fx=None, planes=P.ctypes.data, KH=0, pad=0) != 0
    assert call(pred=4) != 0 and call(clip=3) != 0
    assert call(h=un_e._handle(), pred=_lib.CDC_PRED_V) != 0                          # "v" without its tables
    assert b"cdc_set_schedule_v" in L.cdc_last_error(un_e._handle())
    fresh, *_ = make_unet("small_x")                                                  # a handle without a schedule
    assert call(h=fresh._handle()) != 0 and b"cdc_set_schedule" in L.cdc_last_error(fresh._handle())
    assert np.all(out == 7.0)                                                         # nothing ran
    assert call(fx=None, planes=P.ctypes.data, KH=3, pad=1) == 0 and call(eta=0.5, seeds=sd) == 0 and call(eta=0.5, noise=p) == 0
    # seeds serve at most 65535 images
    big = np.zeros((65536, 1, 1, 1), np.float32)
    sds = np.zeros(65536, np.uint64).ctypes.data_as(U64P)
    h = un._handle()
    args = (big.ctypes.data, big.ctypes.data, None, sds, 0.5, 2, big.ctypes.data, 65536, 1, 1, 1, 0, 0, None, None, 0, 0, _lib.CDC_MEM_HOST, None)
    assert L.cdc_op_ddim_update(h, *args) != 0 and b"65535" in L.cdc_last_error(h)
