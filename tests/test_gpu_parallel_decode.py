"""Parallel-in-time decode (include/cdc_hip.h: cdc_decode_parallel): Picard sweeps over a window of sampler steps, the
window's states as rows of one batch program.  The small U-Net of the golden cases at 64 x 64, 7 steps, a window of 4.

tol = 0 accepts a row only when it did not change at all, so every sweep finalises exactly its first row, which is Phi(y) + 0 on the
exact y: the decode IS the sequential chain of the same B * 4-row program -- rows never interact, no kernel has atomics
(tests/test_gpu_split_decode.py) -- bit for bit, and close to the batch-1 decode as any two batch sizes are (TOL_DEC)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth, tiles, trajectory
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

TOL_DEC = 5e-5     # the bound of the rows-against-batch-1 decode tests (test_gpu_parity.py: TOL_DEC, the same relerr)
H = W = 64
STEPS, P = 7, 4
MJ = json.load(open(os.path.join(GOLDEN, "manifest_small_x.json")))
KW = {k: v for k, v in MJ["unet_kwargs"].items() if k != "embd_type"}
MAN = [(a, tuple(b)) for a, b in MJ["manifest"]]
BMAX = 2
INIT = synth.normal("init", (BMAX, 3, H, W), seed=1, std=0.8)
CTX = synth.context_pyramid(MJ["context_channels_per_level"], BMAX, H, W, seed=3)
SEEDS = [11, 2 ** 40 + 5]
CASES = {"plain": dict(), "seeded": dict(eta=0.7, gamma=0.8)}


def relerr(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


def model(steps=STEPS):
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(MAN, seed=0))
    un.set_decode_chains(1)            # the sequential references run the one B * P-row program the sweeps run
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    diff.set_sample_schedule(steps)
    return un, diff


@pytest.fixture(scope="module")
def md():
    return model()


def decode(diff, B, case, rep=1, ctx=CTX, lo=0, **kw):
    """The images [lo, lo + B), each `rep` times in a row, through p_sample_loop."""
    kw = dict(CASES[case], **kw)
    if "eta" in kw:
        kw["seed"] = [s for s in SEEDS[lo:lo + B] for _ in range(rep)]
    else:
        kw["init"] = np.repeat(INIT[lo:lo + B], rep, axis=0)
    return diff.p_sample_loop((B * rep, 3, H, W), [np.repeat(c[lo:lo + B], rep, axis=0) for c in ctx], clip_denoised=True, **kw)


@pytest.fixture(scope="module")
def sequential(md):
    """{(case, B): the sequential decode of the B * P-row program, its rows b * P}; computed once."""
    return {(case, B): decode(md[1], B, case, rep=P)[::P].copy() for case in CASES for B in (1, 2)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("B", [1, 2])
def test_tol_zero_is_the_sequential_chain_of_the_same_program(md, sequential, case, B):
    un, diff = md
    got, info = decode(diff, B, case, parallel=P, parallel_tol=0, return_info=True)
    print(f"{case} B={B}: {info}")
    np.testing.assert_array_equal(got, sequential[(case, B)])
    assert info["sweeps"] == STEPS and info["strides"] == [1] * STEPS and info["max_stride"] == 1 and info["max_residual"] == 0
    assert info["rows_evaluated"] == STEPS * B * P and info["window"] == P and info["tol"] == 0
    one = np.concatenate([decode(diff, 1, case, lo=b) for b in range(B)])
    e = relerr(got, one)
    print(f"{case} B={B}: against the batch-1 decode of every image: relerr {e:.3e}")
    assert e < TOL_DEC, e
    assert un.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}


@pytest.mark.parametrize("case", list(CASES))
def test_sweep_counts(md, sequential, case):
    """A tolerance nothing misses: every live row is accepted, ceil(steps / p) sweeps, and a picture that is finite (and not the
    chain's: one sweep per window is one Picard iteration).  A moderate tolerance lies between and comes closer."""
    _, diff = md
    got, info = decode(diff, 2, case, parallel=P, parallel_tol=1e30, return_info=True)
    assert info["sweeps"] == math.ceil(STEPS / P) == 2 and info["strides"] == [4, 3] and sum(info["strides"]) == STEPS
    assert info["max_stride"] == P and info["max_residual"] > 0 and np.isfinite(got).all()
    mid, minfo = decode(diff, 2, case, parallel=P, parallel_tol=1e-3, return_info=True)
    assert 2 <= minfo["sweeps"] <= STEPS and sum(minfo["strides"]) == STEPS and minfo["max_residual"] <= 1e-3
    seq = sequential[(case, 2)]
    print(f"{case}: tol 1e30 {info['sweeps']} sweeps relerr {relerr(got, seq):.3e}; tol 1e-3 {minfo['sweeps']} sweeps {minfo['strides']} "
          f"relerr {relerr(mid, seq):.3e}")
    # a window of the whole schedule: one program of STEPS rows, and the last window never shorter than the schedule's rest
    full, finfo = decode(diff, 1, case, parallel=True, parallel_tol=0, return_info=True)
    assert finfo["window"] == STEPS and finfo["sweeps"] == STEPS
    assert relerr(full, sequential[(case, 1)]) < TOL_DEC


def test_device_tensors_on_the_callers_stream(md, sequential):
    import torch
    un, diff = md
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        init = torch.from_numpy(INIT).to(dev, non_blocking=True) * 1.0
        ctx = [torch.from_numpy(c).to(dev, non_blocking=True) * 1.0 for c in CTX]
        rec = diff.p_sample_loop((2, 3, H, W), ctx, clip_denoised=True, init=init, parallel=P, parallel_tol=0)
        got = (rec * 1.0).cpu().numpy()
    np.testing.assert_array_equal(got, sequential[("plain", 2)])
    assert un.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}


def test_decompress_passes_the_keywords_through(md, sequential):
    _, diff = md
    rec, info = diff.decompress([c[:1] for c in CTX], (1, 3, H, W), sample_steps=STEPS, init=INIT[:1], parallel=P, parallel_tol=0,
                                return_info=True)
    np.testing.assert_array_equal(rec, sequential[("plain", 1)])
    assert info["sweeps"] == STEPS


def test_range_fault_repeats_the_whole_call_once():
    """The context leaves the fp16 range: the sweeps are repeated in bf16x3 from the start, counted once."""
    ctx = [c * np.float32(3.0e5) for c in CTX]
    un, diff = model()
    got, info = decode(diff, 1, "plain", ctx=ctx, parallel=P, parallel_tol=0, return_info=True)
    assert np.isfinite(got).all() and info["sweeps"] == STEPS
    assert un.status() == {"arith": 0, "range_faults": 1, "nonfinite_results": 0}, un.status()
    np.testing.assert_array_equal(got, decode(diff, 1, "plain", rep=P, ctx=ctx)[::P])


def test_refusals(md):
    un, diff = md
    ctx = [c[:1] for c in CTX]
    loop = lambda **k: diff.p_sample_loop((1, 3, H, W), ctx, clip_denoised=True, init=INIT[:1], **k)      # noqa: E731
    with pytest.raises(ValueError, match="needs a seed"):
        loop(parallel=P, eta=0.5)
    with pytest.raises(ValueError, match="excludes trajectory"):
        loop(parallel=P, trajectory=[0])
    with pytest.raises(ValueError, match="at least 2 steps"):
        loop(parallel=1)
    with pytest.raises(ValueError, match="parallel_tol"):
        loop(parallel=P, parallel_tol=-1.0)
    with pytest.raises(ValueError, match="history"):
        loop(parallel=P, sampler="dpmpp_2m")
    diff.set_sample_schedule(STEPS)
    # the library's own: a window above the schedule, a trace or noise frames set on the handle
    L, h = _lib.lib(), un._handle()
    out = np.zeros((1, 3, H, W), np.float32)
    ptrs = (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in ctx])

    def call(window=P):
        rc = L.cdc_decode_parallel(h, INIT.ctypes.data, 0.0, None, 0.0, ptrs, len(ctx), out.ctypes.data, 1, H, W, _lib.CDC_PRED_X,
                                   _lib.CDC_CLIP_ALL, window, 0.0, None, None, _lib.CDC_MEM_HOST, None)
        return rc, L.cdc_last_error(h).decode()

    rc, err = call(STEPS + 1)
    assert rc != 0 and f"window {STEPS + 1}" in err and f"steps = {STEPS}" in err, err
    with trajectory.active(h, trajectory.check_args([0], "x0", "float32", STEPS, None, 0, None), H, W):
        rc, err = call()
        assert rc != 0 and "a trace is set" in err, err
    with tiles.noise_frames(h, [(H + 16, W + 16, 8, 4)]):
        rc, err = call()
        assert rc != 0 and "noise frames are set" in err, err
    assert call()[0] == 0
