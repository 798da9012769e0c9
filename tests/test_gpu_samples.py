"""K seeded samples per image on the MI355X: the repeated context staging of cdc_decode_samples, the three kernels of
csrc/sample_kernels.hip (cdc_repeat_images, cdc_sample_moments, cdc_sample_select), and `decompress(samples=K)` / `compress_best_of`.

What ties the new entry points to what is already pinned: a decode of K samples per image is the seeded decode (tests/test_gpu_stochastic.py)
of the context repeated by hand, bit for bit; the moments are the float32 restatement of tests/samples_ref.py, bit for bit, which
tests/test_samples_host.py bounds against float64."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, metrics, samples, synth
from cdc_compression_amd.parallel import sample_seeds
from helpers import GOLDEN, load_case
from samples_ref import welford32
from test_gpu_parity import TOL_DEC, make_unet, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = ctypes.POINTER(ctypes.c_uint64)
HOST, DEVICE = _lib.CDC_MEM_HOST, _lib.CDC_MEM_DEVICE


def _diff(un, tree, comp=None):
    if tree == "x":
        return cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    return cdc.GaussianDiffusionEps(un, comp, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(a, misalign=False):
    """The array on the device; misalign: at an address that is a multiple of 4 bytes (1 byte for uint8) but not of 16."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    if not misalign:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 != 0
    return out


def _handle():
    """Any handle serves the three kernels' entry points (device, stream and error state only)."""
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    return un, un._handle()


# ---- 1. repeated staging is explicit repetition ----------------------------------------------------------------------------------------
def _decode(un, entry, ctx, seeds, rows, K, H, W, gamma, eta, pred, clip, where, solver=0, misalign=False):
    """cdc_decode_samples (entry "samples": ctx of rows / K images), cdc_decode_seeded or cdc_decode_solver (ctx of `rows` images)."""
    L, h = _lib.lib(), un._handle()
    sd = np.asarray(seeds, dtype=np.uint64)
    if where == "device":
        import torch
        keep = [_cuda(c, misalign) for c in ctx]
        ptrs = (ctypes.c_void_p * len(ctx))(*[t.data_ptr() for t in keep])
        out = torch.full((rows, 3, H, W), float("nan"), device="cuda:0")
        optr, mem, st = out.data_ptr(), DEVICE, _stream()
    else:
        keep = [np.ascontiguousarray(c) for c in ctx]
        ptrs = (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in keep])
        out = np.full((rows, 3, H, W), np.nan, np.float32)
        optr, mem, st = out.ctypes.data, HOST, None
    if entry == "samples":
        rc = L.cdc_decode_samples(h, gamma, sd.ctypes.data_as(U64P), eta, ptrs, len(ctx), optr, rows // K, K, H, W, pred, clip, solver, mem, st)
    elif entry == "seeded":
        rc = L.cdc_decode_seeded(h, None, gamma, sd.ctypes.data_as(U64P), eta, ptrs, len(ctx), optr, rows, H, W, pred, clip, mem, st)
    else:
        rc = L.cdc_decode_solver(h, None, gamma, sd.ctypes.data_as(U64P), ptrs, len(ctx), optr, rows, H, W, pred, clip, mem, st)
    _lib.check(h, rc)
    return out if where == "host" else out.cpu().numpy()


def _case(name):
    """(unet, diffusion, context of B = 2 images, H, W) of a staging case."""
    if name == "odd_x_24x42":            # odd_x's model on a 24 x 42 frame (its golden frame is 40 wide and holds one image)
        kw, man, sd, *_ = load_case("odd_x")
        un = cdc.Unet(**kw)
        un.load_state_dict(sd)
        return un, _diff(un, "x"), synth.context_pyramid([5], 2, 24, 42, seed=3), 24, 42
    un, _, _, x, _, ctx, _ = make_unet(name)
    return un, _diff(un, "x" if name.endswith("_x") else "eps"), [c[:2] for c in ctx], x.shape[2], x.shape[3]


SEEDS6 = [3, (3 << 33) + 17, 2 ** 64 - 1, 0, (1 << 50) + 7, 12345678901234567]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["small_x", "small_eps", "odd_x_24x42"])
def test_decode_samples_is_the_seeded_decode_of_the_repeated_context(name, where):
    """odd_x_24x42 on the device: the context tensor sits at an address that is no multiple of 16, so the repeat kernel stages it
    by its element path (every level of these models is a whole number of 16-byte units)."""
    un, diff, ctx, H, W = _case(name)
    diff.set_sample_schedule(3)
    pred, clip = diff._pred_flag(), diff._clip_flag(True if diff._param == "x" else diff.clip_noise)
    got = _decode(un, "samples", ctx, SEEDS6, 6, 3, H, W, 0.8, 0.5, pred, clip, where, misalign=name == "odd_x_24x42")
    want = _decode(un, "seeded", [np.repeat(c, 3, axis=0) for c in ctx], SEEDS6, 6, 1, H, W, 0.8, 0.5, pred, clip, where)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert float(np.abs(got[0] - got[1]).max()) > 0.05                        # two samples of image 0 are two pictures
    # K = 1 is the existing entry point
    one = _decode(un, "samples", ctx, SEEDS6[:2], 2, 1, H, W, 0.8, 0.5, pred, clip, where)
    np.testing.assert_array_equal(_bits(one), _bits(_decode(un, "seeded", ctx, SEEDS6[:2], 2, 1, H, W, 0.8, 0.5, pred, clip, where)))


def test_decode_samples_in_the_full_range_arithmetic():
    un, diff, ctx, H, W = _case("small_x")
    h = un._handle()
    _lib.check(h, _lib.lib().cdc_set_arith(h, 0))                             # CDC_ARITH_BF16X3
    diff.set_sample_schedule(3)
    got = _decode(un, "samples", ctx, SEEDS6, 6, 3, H, W, 0.8, 0.5, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, "host")
    want = _decode(un, "seeded", [np.repeat(c, 3, axis=0) for c in ctx], SEEDS6, 6, 1, H, W, 0.8, 0.5, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, "host")
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert _lib.lib().cdc_get_arith(h) == 0


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_samples_with_the_multistep_update(where):
    un, diff, ctx, H, W = _case("small_x")
    diff.set_sample_schedule(4, sampler="dpmpp_2m", spacing="logsnr")
    args = (H, W, 0.8, 0.0, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, where)
    got = _decode(un, "samples", ctx, SEEDS6, 6, 3, *args, solver=1)
    want = _decode(un, "solver", [np.repeat(c, 3, axis=0) for c in ctx], SEEDS6, 6, 1, *args)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert not np.array_equal(got, _decode(un, "samples", ctx, SEEDS6, 6, 3, *args, solver=0))
    one = _decode(un, "samples", ctx, SEEDS6[:2], 2, 1, *args, solver=1)
    np.testing.assert_array_equal(_bits(one), _bits(_decode(un, "solver", ctx, SEEDS6[:2], 2, 1, *args)))


# ---- 2. cdc_repeat_images ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("per", [3 * 8 * 12, 3 * 7 * 9, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_repeat_images_is_np_repeat(dtype, per, K):
    """288 floats: 16-byte units; 288 bytes too; 189 and 1: the element forms (the second image starts off a 16-byte boundary)."""
    un, h = _handle()
    L, B = _lib.lib(), 2
    rng = np.random.default_rng(per + K)
    src = rng.integers(0, 256, (B, per)).astype(np.uint8) if dtype == np.uint8 else rng.standard_normal((B, per)).astype(np.float32)
    if dtype == np.float32:
        src.view(np.uint32)[0, 0] = 0x7FC12345                                # a NaN with a payload
    want = np.repeat(src, K, axis=0)
    eb = src.dtype.itemsize
    host = np.zeros((B * K, per), dtype)
    _lib.check(h, L.cdc_repeat_images(h, src.ctypes.data, host.ctypes.data, B, K, per, eb, HOST, None))
    np.testing.assert_array_equal(_bits(host), _bits(want))
    import torch
    for misalign in (False, True):
        ts = _cuda(src, misalign)
        td = torch.zeros((B * K, per), dtype=ts.dtype, device="cuda:0")
        _lib.check(h, L.cdc_repeat_images(h, ts.data_ptr(), td.data_ptr(), B, K, per, eb, DEVICE, _stream()))
        np.testing.assert_array_equal(_bits(td.cpu().numpy()), _bits(want))
    out = samples.repeat_images(un, src.reshape(B, 1, per), K)                # the Python wrapper keeps the container family
    assert out.shape == (B * K, 1, per) and out.dtype == dtype
    np.testing.assert_array_equal(_bits(out.reshape(B * K, per)), _bits(want))


# ---- 3. cdc_sample_moments ---------------------------------------------------------------------------------------------------------------
def _moment_inputs(B, K, per):
    rng = np.random.default_rng(per)
    x = np.clip(rng.standard_normal((B, K, per)), -1, 1).astype(np.float32)
    for b, k, e, v in ((0, 1, 5, 1e4), (1, 3, per - 1, -1e4), (0, 4, 17, 1e4), (1, 0, 0, -1e4)):
        x[b, k, e] = v
    return x


def _fold(h, x, cuts, where, with_m2=True, finish=False):
    """The chunks of x [B][K][per] through cdc_sample_moments -> (mean, m2) as NumPy arrays."""
    L = _lib.lib()
    B, K, per = x.shape
    if where == "device":
        import torch
        mean = torch.full((B, per), float("nan"), device="cuda:0")
        m2 = torch.full((B, per), float("nan"), device="cuda:0") if with_m2 else None
        ptr, mem, st = (lambda t: t.data_ptr()), DEVICE, _stream()
    else:
        mean = np.full((B, per), np.nan, np.float32)
        m2 = np.full((B, per), np.nan, np.float32) if with_m2 else None
        ptr, mem, st = (lambda a: a.ctypes.data), HOST, None
    k0 = 0
    for c in cuts:
        chunk = np.ascontiguousarray(x[:, k0:k0 + c])
        keep = _cuda(chunk) if where == "device" else chunk
        _lib.check(h, L.cdc_sample_moments(h, ptr(keep), B, c, per, k0, ptr(mean), ptr(m2) if with_m2 else None,
                                           int(finish and k0 + c == K), mem, st))
        k0 += c
    assert k0 == K
    get = (lambda t: t.cpu().numpy()) if where == "device" else (lambda a: a)
    return get(mean), (get(m2) if with_m2 else None)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("per", [288, 189])
def test_sample_moments_hold_the_bits_of_the_restatement_whatever_the_chunking(per, where):
    """per_image 189: the images start off the 16-byte boundary, the element form runs."""
    un, h = _handle()
    B, K = 2, 5
    x = _moment_inputs(B, K, per)
    want = [welford32(x[b]) for b in range(B)]
    want_mean, want_m2 = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert np.isfinite(want_m2).all() and float(want_m2.max()) > 1e7
    for cuts in ((5,), (2, 3), (1, 1, 1, 1, 1)):
        mean, m2 = _fold(h, x, cuts, where)
        np.testing.assert_array_equal(_bits(mean), _bits(want_mean), err_msg=str(cuts))
        np.testing.assert_array_equal(_bits(m2), _bits(want_m2), err_msg=str(cuts))
    mean, none = _fold(h, x, (2, 3), where, with_m2=False)                    # m2 = NULL: the mean only
    assert none is None
    np.testing.assert_array_equal(_bits(mean), _bits(want_mean))
    with np.errstate(all="ignore"):
        want_var = want_m2 / np.float32(K - 1)
    for cuts in ((5,), (2, 3)):
        mean, var = _fold(h, x, cuts, where, finish=True)
        np.testing.assert_array_equal(_bits(mean), _bits(want_mean))
        np.testing.assert_array_equal(_bits(var), _bits(want_var))
    same = np.repeat(x[:, :1], K, axis=1)                                     # K identical samples: the variance is exactly 0
    mean, var = _fold(h, same, (2, 3), where, finish=True)
    np.testing.assert_array_equal(_bits(mean), _bits(same[:, 0]))
    assert not var.any()


# ---- 4. cdc_sample_select and the refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("per", [288, 189])
def test_sample_select_copies_the_picked_samples_bit_for_bit(per, where):
    un, h = _handle()
    L, B, Kc = _lib.lib(), 3, 4
    rng = np.random.default_rng(per)
    x = rng.standard_normal((B, Kc, per)).astype(np.float32)
    x.view(np.uint32)[0, 2, 3] = 0xFFC0BEEF                                   # a NaN with a payload, an Inf
    x[0, 2, 4] = np.inf
    x.view(np.uint32)[2, 0, per - 1] = 0x7F800001                             # a signalling NaN
    x[2, 0, 0] = -np.inf
    before = rng.standard_normal((B, per)).astype(np.float32)
    pick = (ctypes.c_int * B)(2, -1, 0)
    if where == "device":
        tx, tb = _cuda(x), _cuda(before)
        _lib.check(h, L.cdc_sample_select(h, tx.data_ptr(), pick, tb.data_ptr(), B, Kc, per, DEVICE, _stream()))
        best = tb.cpu().numpy()
    else:
        best = before.copy()
        _lib.check(h, L.cdc_sample_select(h, x.ctypes.data, pick, best.ctypes.data, B, Kc, per, HOST, None))
    np.testing.assert_array_equal(_bits(best[0]), _bits(x[0, 2]))
    np.testing.assert_array_equal(_bits(best[1]), _bits(before[1]))           # untouched
    np.testing.assert_array_equal(_bits(best[2]), _bits(x[2, 0]))
    bad = (ctypes.c_int * B)(0, 4, 0)                                         # pick = Kc
    keep = best.copy()
    assert L.cdc_sample_select(h, x.ctypes.data, bad, best.ctypes.data, B, Kc, per, HOST, None) == -1
    assert b"pick[1]" in L.cdc_last_error(h)
    np.testing.assert_array_equal(_bits(best), _bits(keep))


def test_entry_point_refusals():
    un, h = _handle()
    L = _lib.lib()
    f = np.zeros(64, np.float32)
    p, z = f.ctypes.data, None
    seeds = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    pick = (ctypes.c_int * 2)(0, 0)
    ctx = (ctypes.c_void_p * 2)(p, p)
    big = (ctypes.c_uint64 * 1)(1)
    calls = {
        "repeat: null src": lambda: L.cdc_repeat_images(h, z, p, 2, 2, 4, 4, HOST, None),
        "repeat: null dst": lambda: L.cdc_repeat_images(h, p, z, 2, 2, 4, 4, HOST, None),
        "repeat: B < 1": lambda: L.cdc_repeat_images(h, p, p, 0, 2, 4, 4, HOST, None),
        "repeat: K < 1": lambda: L.cdc_repeat_images(h, p, p, 2, 0, 4, 4, HOST, None),
        "repeat: per_image < 1": lambda: L.cdc_repeat_images(h, p, p, 2, 2, 0, 4, HOST, None),
        "repeat: elem_bytes 2": lambda: L.cdc_repeat_images(h, p, p, 2, 2, 4, 2, HOST, None),
        "repeat: mem kind": lambda: L.cdc_repeat_images(h, p, p, 2, 2, 4, 4, 7, None),
        "moments: null samples": lambda: L.cdc_sample_moments(h, z, 2, 2, 4, 0, p, p, 0, HOST, None),
        "moments: null mean": lambda: L.cdc_sample_moments(h, p, 2, 2, 4, 0, z, p, 0, HOST, None),
        "moments: Kc < 1": lambda: L.cdc_sample_moments(h, p, 2, 0, 4, 0, p, p, 0, HOST, None),
        "moments: B < 1": lambda: L.cdc_sample_moments(h, p, 0, 2, 4, 0, p, p, 0, HOST, None),
        "moments: per_image < 1": lambda: L.cdc_sample_moments(h, p, 2, 2, -3, 0, p, p, 0, HOST, None),
        "moments: count_before < 0": lambda: L.cdc_sample_moments(h, p, 2, 2, 4, -1, p, p, 0, HOST, None),
        "moments: finish at count 1": lambda: L.cdc_sample_moments(h, p, 2, 1, 4, 0, p, p, 1, HOST, None),
        "select: null samples": lambda: L.cdc_sample_select(h, z, pick, p, 2, 2, 4, HOST, None),
        "select: null pick": lambda: L.cdc_sample_select(h, p, None, p, 2, 2, 4, HOST, None),
        "select: null best": lambda: L.cdc_sample_select(h, p, pick, z, 2, 2, 4, HOST, None),
        "select: Kc < 1": lambda: L.cdc_sample_select(h, p, pick, p, 2, 0, 4, HOST, None),
        "select: per_image < 1": lambda: L.cdc_sample_select(h, p, pick, p, 2, 2, 0, HOST, None),
        "samples: null seeds": lambda: L.cdc_decode_samples(h, 0.8, None, 0.5, ctx, 2, p, 2, 2, 32, 32, 0, 1, 0, HOST, None),
        "samples: K < 1": lambda: L.cdc_decode_samples(h, 0.8, seeds, 0.5, ctx, 2, p, 2, 0, 32, 32, 0, 1, 0, HOST, None),
        "samples: B < 1": lambda: L.cdc_decode_samples(h, 0.8, seeds, 0.5, ctx, 2, p, 0, 2, 32, 32, 0, 1, 0, HOST, None),
        "samples: B * K > 65535": lambda: L.cdc_decode_samples(h, 0.8, big, 0.5, ctx, 2, p, 256, 256, 32, 32, 0, 1, 0, HOST, None),
        "samples: solver 2": lambda: L.cdc_decode_samples(h, 0.8, seeds, 0.0, ctx, 2, p, 2, 2, 32, 32, 0, 1, 2, HOST, None),
        "samples: solver with eta": lambda: L.cdc_decode_samples(h, 0.8, seeds, 0.5, ctx, 2, p, 2, 2, 32, 32, 0, 1, 1, HOST, None),
        "samples: eta not finite": lambda: L.cdc_decode_samples(h, 0.8, seeds, float("nan"), ctx, 2, p, 2, 2, 32, 32, 0, 1, 0, HOST, None),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == -1 and L.cdc_last_error(h), (what, rc)
    # a finish at the final count 2 and a pick of -1 everywhere are fine
    acc = np.zeros((2, 2, 4), np.float32)
    _lib.check(h, L.cdc_sample_moments(h, acc.ctypes.data, 2, 1, 4, 1, acc[0].ctypes.data, acc[1].ctypes.data, 1, HOST, None))
    none = (ctypes.c_int * 2)(-1, -5)
    _lib.check(h, L.cdc_sample_select(h, acc.ctypes.data, none, acc[0].ctypes.data, 2, 2, 4, HOST, None))
    # the decode needs a U-Net handle with weights and a schedule, as cdc_decode_seeded does
    assert L.cdc_decode_samples(h, 0.8, seeds, 0.5, ctx, 2, p, 2, 2, 32, 32, 0, 1, 0, HOST, None) == -2


# ---- 5. decompress(samples=K) ------------------------------------------------------------------------------------------------------------
def _three_level():
    """The model of test_rows_of_a_seeded_batch_match_their_batch1_decodes, B = 2 at 32 x 32."""
    un = cdc.Unet(dim=32, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    return _diff(un, "x"), synth.context_pyramid([8, 32], 2, 32, 32, seed=3)


def test_decompress_samples_are_the_single_seeded_decodes():
    diff, ctx = _three_level()
    args = dict(gamma=0.8, eta=0.5, sample_steps=4)
    rec = diff.decompress(ctx, samples=4, seed=7, **args)
    assert rec.shape == (2, 4, 3, 32, 32) and rec.dtype == np.float32 and np.isfinite(rec).all()
    seeds = sample_seeds(7, 2, 4)
    for b in range(2):
        for k in range(4):
            one = diff.decompress([c[b:b + 1] for c in ctx], seed=[seeds[b][k]], **args)
            e = relerr(one[0], rec[b, k])
            assert e < TOL_DEC, (b, k, e)
    assert float(np.abs(rec[0, 0] - rec[0, 1]).max()) > 0.05
    # sample 0 is today's seeded decode of the same seed (same batch -> same launch plans only at K = 1: the batch-row bound)
    plain = diff.decompress(ctx, seed=7, **args)
    assert max(relerr(plain[b], rec[b, 0]) for b in range(2)) < TOL_DEC
    import torch
    trec = diff.decompress([torch.from_numpy(c).to("cuda:0") for c in ctx], samples=4, seed=7, **args)
    assert trec.is_cuda and tuple(trec.shape) == (2, 4, 3, 32, 32)
    np.testing.assert_array_equal(_bits(trec.cpu().numpy()), _bits(rec))


def test_decompress_mean_and_variance_are_the_restatement_of_the_samples():
    diff, ctx = _three_level()
    args = dict(samples=4, seed=7, gamma=0.8, eta=0.5, sample_steps=4)
    by_chunk = {}
    for chunk in (None, 2, 1, 3):
        rec = diff.decompress(ctx, sample_chunk=chunk, **args)
        mean, var = diff.decompress(ctx, reduce="mean_var", sample_chunk=chunk, **args)
        assert mean.shape == var.shape == (2, 3, 32, 32)
        for b in range(2):
            m, m2 = welford32(rec[b])
            np.testing.assert_array_equal(_bits(mean[b]), _bits(m), err_msg=str(chunk))
            np.testing.assert_array_equal(_bits(var[b]), _bits(m2 / np.float32(3)), err_msg=str(chunk))
        np.testing.assert_array_equal(_bits(diff.decompress(ctx, reduce="mean", sample_chunk=chunk, **args)), _bits(mean))
        by_chunk[chunk] = (rec, mean, var)
    assert float(by_chunk[None][2].max()) > 1e-4                               # the samples do differ
    # Launch plans depend on the rows of a call (B * Kc = 2, 4, 8), so two chunkings agree to the project's batch-row bound, not bit
    # for bit: every sample within d = TOL_DEC of its twin (max |x| <= 1: the x-tree clips), hence the mean within d, and the
    # variance within K / (K - 1) * 2 max|x - mean| d <= 4 / 3 * 2 * 2 d < 6 d.
    for a, b in ((1, 2), (None, 1)):
        assert relerr(by_chunk[a][0], by_chunk[b][0]) < TOL_DEC
        assert relerr(by_chunk[a][1], by_chunk[b][1]) < TOL_DEC
        assert float(np.abs(by_chunk[a][2] - by_chunk[b][2]).max()) < 6 * TOL_DEC


def test_decompress_samples_of_an_image_that_is_not_its_frame():
    """A 23 x 41 image on odd_x's 24 x 42 frame: the moments are folded on the frame and cropped once, which equals the moments of the
    cropped samples (element-wise operations); as_uint8 gives the saved form of the samples and of the mean."""
    un, diff, ctx, Hp, Wp = _case("odd_x_24x42")
    H, W = 23, 41
    args = dict(shape=(2, 3, H, W), samples=3, seed=[5, 2 ** 64 - 1], gamma=0.8, eta=0.5, sample_steps=3)
    rec = diff.decompress(ctx, **args)
    assert rec.shape == (2, 3, 3, H, W)
    mean, var = diff.decompress(ctx, reduce="mean_var", **args)
    assert mean.shape == var.shape == (2, 3, H, W)
    for b in range(2):
        m, m2 = welford32(rec[b])
        np.testing.assert_array_equal(_bits(mean[b]), _bits(m))
        np.testing.assert_array_equal(_bits(var[b]), _bits(m2 / np.float32(2)))
    u8 = diff.decompress(ctx, as_uint8=True, **args)
    assert u8.dtype == np.uint8 and u8.shape == (2, 3, 3, H, W)
    h, dev = un._handle(), un.device_index
    np.testing.assert_array_equal(u8.reshape(6, 3, H, W), cdc.frame.crop(h, rec.reshape(6, 3, H, W), H, W, dev, as_uint8=True))
    mu8 = diff.decompress(ctx, reduce="mean", as_uint8=True, **args)
    assert mu8.dtype == np.uint8
    np.testing.assert_array_equal(mu8, cdc.frame.crop(h, mean, H, W, dev, as_uint8=True))


# ---- 6. compress_best_of -----------------------------------------------------------------------------------------------------------------
def _small(tag, with_lpips=False):
    """A small model with its compressor, as tests/test_gpu_metrics.py builds it (with_lpips: the synthetic LPIPS-VGG weights of
    tests/test_gpu_lpips.py on board)."""
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))[tag]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    comp = (cdc.ResnetCompressor if tag == "x" else cdc.BigCompressor)(**meta["comp_kwargs"])
    diff = _diff(un, tag, comp)
    sd = {"denoise_fn." + k: v for k, v in
          synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0 if tag == "x" else 0.2).items()}
    sd.update({"context_fn." + k: v for k, v in synth.unet_state_dict([(k, tuple(v)) for k, v in meta["comp_manifest"]], seed=meta["seed"]).items()})
    if with_lpips:
        sd.update(synth.lpips_vgg_state_dict(seed=0, prefix="loss_fn_vgg.", with_duplicates=True))
    return diff.load_state_dict(sd), ({} if tag == "x" else {"sample_mode": "ddim"})


def _pictures(B, H, W):
    return np.clip(synth.normal("pictures", (B, 3, H, W), seed=2, std=0.4), -1, 1)


@pytest.mark.parametrize("tag", ["x", "eps"])
def test_compress_best_of_returns_the_best_sample_and_its_seed(tag):
    diff, kw = _small(tag)
    images = _pictures(2, 32, 32)
    args = dict(seed=11, gamma=0.8, eta=0.5, sample_steps=3)
    res = diff.compress_best_of(images, 4, metric="psnr", sample_chunk=2, **args)
    assert sorted(res) == ["bpp", "reconstruction", "sample", "score", "scores", "seed"]
    scores = res["scores"]
    assert scores.shape == (2, 4) and scores.dtype == np.float64 and np.isfinite(scores).all()
    assert len(set(scores[0])) > 1
    seeds = sample_seeds(11, 2, 4)
    for b in range(2):
        assert res["score"][b] == scores[b].max()
        assert res["sample"][b] == int(np.argmax(scores[b]))
        assert res["seed"][b] == seeds[b][res["sample"][b]]
    assert res["seed"].dtype == np.uint64
    rec, bpp = diff.compress(images, sample_steps=3, bpp_return_mean=False, **kw)
    np.testing.assert_array_equal(np.asarray(res["bpp"]), np.asarray(bpp))
    # the same context, the same chunking: that sample of decompress(samples=4), bit for bit
    q = diff.context_fn(images)
    every = diff.decompress(q["output"], samples=4, sample_chunk=2, **args)
    assert res["reconstruction"].shape == (2, 3, 32, 32)
    for b in range(2):
        np.testing.assert_array_equal(_bits(res["reconstruction"][b]), _bits(every[b, res["sample"][b]]))
    # the scores are those of the samples against the originals
    for k in range(4):
        np.testing.assert_array_equal(scores[:, k], metrics.psnr(diff.denoise_fn, np.ascontiguousarray(every[:, k]), images, as_saved=True))
    # the decoder's side: the transmitted seed reproduces the picture (another batch -> the batch-row bound)
    again = diff.decompress(q["output"], **{**args, "seed": [int(s) for s in res["seed"]]})
    assert relerr(again, res["reconstruction"]) < TOL_DEC
    # the default chunk: one call of 8 rows
    whole = diff.compress_best_of(images, 4, **args)
    every = diff.decompress(q["output"], samples=4, **args)
    for b in range(2):
        assert whole["sample"][b] == int(np.argmax(whole["scores"][b]))
        np.testing.assert_array_equal(_bits(whole["reconstruction"][b]), _bits(every[b, whole["sample"][b]]))


def test_compress_best_of_selection_rule_with_a_stubbed_metric(monkeypatch):
    diff, _ = _small("x")
    images = _pictures(2, 32, 32)
    nan = float("nan")
    table = np.asarray([[nan, 5.0, 5.0, nan, 5.0, 4.0],          # a tie across chunks: the lowest k; a NaN never beats a number
                        [nan, nan, nan, nan, nan, nan]])         # all NaN: sample 0
    calls = []

    def fake_psnr(model, a, b, size=None, as_saved=False):
        k0 = 2 * len(calls)
        calls.append((tuple(a.shape), tuple(b.shape), size, as_saved))
        return table[:, k0:k0 + 2].reshape(-1).copy()

    monkeypatch.setattr(metrics, "psnr", fake_psnr)
    args = dict(seed=3, gamma=0.8, sample_steps=2)
    res = diff.compress_best_of(images, 6, metric="psnr", sample_chunk=2, **args)
    assert calls == [((4, 3, 32, 32), (4, 3, 32, 32), (32, 32), True)] * 3
    assert list(res["sample"]) == [1, 0]
    np.testing.assert_array_equal(res["scores"], table)
    assert res["score"][0] == 5.0 and np.isnan(res["score"][1])
    seeds = sample_seeds(3, 2, 6)
    assert list(res["seed"]) == [seeds[0][1], seeds[1][0]]
    every = diff.decompress(diff.context_fn(images)["output"], samples=6, sample_chunk=2, **args)
    for b, k in ((0, 1), (1, 0)):
        np.testing.assert_array_equal(_bits(res["reconstruction"][b]), _bits(every[b, k]))
    # lower is better: the first 4.0 wins; NaNs still lose
    calls.clear()
    monkeypatch.setattr(samples, "METRICS", dict(samples.METRICS, psnr=False))
    low = diff.compress_best_of(images, 6, metric="psnr", sample_chunk=2, **args)
    assert list(low["sample"]) == [5, 0]


def test_compress_best_of_by_lpips_takes_the_lowest_distance():
    diff, _ = _small("x", with_lpips=True)
    images = _pictures(2, 32, 32)
    args = dict(seed=11, gamma=0.8, eta=0.5, sample_steps=3)
    res = diff.compress_best_of(images, 4, metric="lpips", **args)
    scores = res["scores"]
    assert scores.shape == (2, 4) and np.isfinite(scores).all() and (scores > 0).all() and len(set(scores[0])) > 1
    for b in range(2):
        assert res["score"][b] == scores[b].min() and res["sample"][b] == int(np.argmin(scores[b]))
    every = diff.decompress(diff.context_fn(images)["output"], samples=4, **args)
    for b in range(2):
        np.testing.assert_array_equal(_bits(res["reconstruction"][b]), _bits(every[b, res["sample"][b]]))
    # (a pair's LPIPS does not depend on the batch it sits in)
    np.testing.assert_array_equal(res["score"], metrics.lpips(diff.loss_fn_vgg, res["reconstruction"], images, as_saved=True))
    plain, _ = _small("x")
    with pytest.raises(ValueError, match="lpips"):
        plain.compress_best_of(images, 4, metric="lpips", **args)
    with pytest.raises(ValueError, match="160"):
        plain.compress_best_of(images, 4, metric="ms_ssim", **args)


# ---- 7. the example script ---------------------------------------------------------------------------------------------------------------
def test_example_script_selects_a_seed_only_when_asked(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    src = tmp_path / "in"
    src.mkdir()
    u8 = np.round((_pictures(1, 64, 64)[0] * 0.5 + 0.5) * 255).astype(np.uint8)
    Image.fromarray(u8.transpose(1, 2, 0)).save(src / "a.png")
    outs = []
    for n, flags in enumerate(([], ["--samples", "3", "--select", "psnr"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                            "--n_denoise_step", "2", "--img_dir", str(src), "--out_dir", str(tmp_path / f"out{n}")] + flags,
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, CDC_SYNTHETIC_INIT="1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout.splitlines())
    plain, best = outs
    assert len(plain) == 2 and plain[0] == "image: a.png" and plain[1].startswith("bpp:")        # today's output
    assert best[:2] == plain and len(best) == 5
    assert best[2].startswith("scores: ") and best[3].startswith("sample: ") and best[4].startswith("chosen seed: ")
    scores = [float(v) for v in best[2].split()[1:]]
    assert len(scores) == 3 and all(np.isfinite(scores)) and len(set(scores)) > 1
    k = int(best[3].split()[1])
    assert k == samples.argbest(scores, True)
    assert int(best[4].split()[2]) == sample_seeds(0, 1, 3)[0][k]
    saved = np.asarray(Image.open(tmp_path / "out1" / "a.png").convert("RGB")).transpose(2, 0, 1)[None]
    got = metrics.psnr(_handle()[0], saved, u8[None])
    assert abs(got[0] - scores[k]) <= 1e-9 * scores[k]                         # the saved picture is the selected sample
