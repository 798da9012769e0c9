"""Split decode (include/cdc_hip.h: cdc_set_decode_chains): a batch as two half-batch chains on two streams, rows
[0, ceil(B / 2)) on the handle's program and the rest on its twin's.  Images never interact and no kernel has atomics, so a split
decode IS the two single-chain decodes of its halves, bit for bit, through every entry point; against the unsplit decode of the same
batch it differs as any two launch plans do.  The small U-Net of the golden cases at 64 x 64, 3 steps, the split forced by the
setter."""
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth, tiles
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

TOL_DEC = 5e-5     # the bound of the rows-against-batch-1 decode tests (test_gpu_parity.py: TOL_DEC, the same relerr)
H = W = 64
STEPS = 3
MJ = json.load(open(os.path.join(GOLDEN, "manifest_small_x.json")))
KW = {k: v for k, v in MJ["unet_kwargs"].items() if k != "embd_type"}
MAN = [(a, tuple(b)) for a, b in MJ["manifest"]]
BMAX = 4
INIT = synth.normal("init", (BMAX, 3, H, W), seed=1, std=0.8)
CTX = synth.context_pyramid(MJ["context_channels_per_level"], BMAX, H, W, seed=3)
SEEDS = [11, 7, 2 ** 40 + 5, 3]


def relerr(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


def model(chains, seed=0, sampler="ddim", steps=STEPS, arith=None):
    un = cdc.Unet(**KW)
    un.load_state_dict(synth.unet_state_dict(MAN, seed=seed))
    un.set_decode_chains(chains)
    if arith is not None:
        _lib.check(un._handle(), _lib.lib().cdc_set_arith(un._handle(), arith))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    diff.set_sample_schedule(steps, sampler=sampler)
    return un, diff


def decode(diff, lo, hi, ctx=CTX, **kw):
    """Rows [lo, hi) of the shared inputs through p_sample_loop (clip_denoised as decompress() of the x tree has it)."""
    if "seed" in kw:
        kw["seed"] = kw["seed"][lo:hi]
    if kw.pop("with_init", True):
        kw["init"] = INIT[lo:hi]
    return diff.p_sample_loop((hi - lo, 3, H, W), [c[lo:hi] for c in ctx], clip_denoised=True, **kw)


def halves(diff1, B, **kw):
    b0 = (B + 1) // 2
    return np.concatenate([decode(diff1, 0, b0, **kw), decode(diff1, b0, B, **kw)])


@pytest.fixture(scope="module")
def split():
    return model(2)


@pytest.fixture(scope="module")
def single():
    return model(1)


@pytest.mark.parametrize("B", [2, 3, 4])
def test_split_decode_is_its_two_halves_bitwise_and_close_to_the_unsplit_decode(B, split, single):
    un2, d2 = split
    assert un2.decode_chains(B, H, W) == 2
    got = decode(d2, 0, B)
    np.testing.assert_array_equal(got, halves(single[1], B))
    whole = decode(single[1], 0, B)
    e = relerr(got, whole)
    print(f"split vs unsplit, B={B}: relerr {e:.3e}")
    assert e < TOL_DEC, e
    assert un2.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}


def test_split_decode_of_device_tensors_on_the_callers_stream(split, single):
    """Device memory: the chains fork from and join the caller's stream, here a side stream with work queued in front (the inputs
    are made on it) and behind (the result is read on it)."""
    import torch
    dev = torch.device("cuda", 0)
    want = halves(single[1], 4)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        init = torch.from_numpy(INIT).to(dev, non_blocking=True) * 1.0
        ctx = [torch.from_numpy(c).to(dev, non_blocking=True) * 1.0 for c in CTX]
        rec = split[1].p_sample_loop((4, 3, H, W), ctx, clip_denoised=True, init=init)
        got = (rec * 1.0).cpu().numpy()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("B", [3, 4])
def test_seeded_and_solver_entry_points_offset_seeds_and_history_by_rows(B, split, single):
    """cdc_decode_seeded with eta != 0, a generated start image and distinct per-row seeds; cdc_decode_solver (its history x0 is per
    chain): a wrong row offset of either shows as a half that differs."""
    kw = dict(eta=0.7, seed=SEEDS, gamma=0.8, with_init=False)
    got = decode(split[1], 0, B, **kw)
    np.testing.assert_array_equal(got, halves(single[1], B, **kw))
    assert float(np.abs(got[0] - got[B - 1]).max()) > 0.05
    _, s2 = model(2, sampler="dpmpp_2m")
    _, s1 = model(1, sampler="dpmpp_2m")
    np.testing.assert_array_equal(decode(s2, 0, B), halves(s1, B))
    np.testing.assert_array_equal(decode(s2, 0, B, seed=SEEDS, gamma=0.8, with_init=False), halves(s1, B, seed=SEEDS, gamma=0.8, with_init=False))


def test_range_fault_in_the_twin_repeats_the_whole_call_once():
    """The last row's context alone leaves the fp16 range: the twin's chain flags it, the whole call is repeated in bf16x3 (both
    chains), counted once; the first half is what a handle in bf16x3 from the start decodes of that half."""
    B = 4
    ctx = [c.copy() for c in CTX]
    for c in ctx:
        c[B - 1] *= np.float32(3.0e5)
    un, d2 = model(2)
    got = decode(d2, 0, B, ctx=ctx)
    assert np.isfinite(got).all()
    assert un.status() == {"arith": 0, "range_faults": 1, "nonfinite_results": 0}, un.status()
    un1, d1 = model(1, arith=0)
    np.testing.assert_array_equal(got[:2], decode(d1, 0, 2, ctx=ctx))
    np.testing.assert_array_equal(got[2:], decode(d1, 2, 4, ctx=ctx))
    assert un1.range_faults == 0
    # ... and the handle goes on splitting, in the arithmetic it is left in
    np.testing.assert_array_equal(decode(d2, 0, B), halves(d1, B))
    assert un.range_faults == 1


def _prof_classes(un):
    L, h = _lib.lib(), un._handle()
    import ctypes
    out = {}
    for c in range(L.cdc_prof_num_classes()):
        ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.check(h, L.cdc_prof_get(h, c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)))
        out[L.cdc_prof_name(c).decode()] = (ms.value, n.value, fl.value, by.value)
    ops = []
    for i in range(L.cdc_prof_num_ops(h)):
        lab, ms, n, fl = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(h, L.cdc_prof_op(h, i, ctypes.byref(lab), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        ops.append((lab.value.decode(), ms.value, n.value, fl.value))
    return out, ops


def test_profiling_tables_sum_the_two_chains():
    """Profiling on: per class, the flops of the two half-batch chains sum to those of the unsplit batch (the same layers over the
    same images) and the launches double; no class the unsplit decode fills is empty.  The per-op table lists the half-batch program
    once, its flops summed over the chains, n = the sampled iterations."""
    B = 4
    res = {}
    for chains in (1, 2):
        un, d = model(chains)
        _lib.check(un._handle(), _lib.lib().cdc_prof_enable(un._handle(), 1))
        decode(d, 0, B)
        res[chains] = _prof_classes(un)
    (c1, ops1), (c2, ops2) = res[1], res[2]
    filled = [k for k, v in c1.items() if v[1] > 0]
    assert "conv3x3" in filled and "layernorm" in filled and "small" in filled
    for k in c1:
        assert (c2[k][1] > 0) == (c1[k][1] > 0), k
        assert c2[k][2] == pytest.approx(c1[k][2], rel=1e-9), (k, c1[k], c2[k])
        if c1[k][1] > 0:
            assert c2[k][0] > 0
    iter_ops = [o for o in ops2 if o[2] > 0]
    assert iter_ops and all(o[2] == STEPS for o in iter_ops), {o[2] for o in ops2}
    assert sum(o[3] for o in iter_ops) == pytest.approx(sum(o[3] for o in ops1 if o[2] > 0), rel=1e-9)


def test_fall_backs_run_the_single_chain_bit_for_bit(split, single):
    """A traced decode, a decode with noise frames and B = 1 run one chain whatever the setter says."""
    (un2, d2), (un1, d1) = split, single
    B = 4
    a, ta = decode(d2, 0, B, trajectory=[0, 2])
    b, tb = decode(d1, 0, B, trajectory=[0, 2])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ta.x0, tb.x0)
    frames = [(H + 16, W + 16, 8 * (r % 2), 4 * r) for r in range(B)]
    kw = dict(eta=0.7, seed=SEEDS, gamma=0.8, with_init=False)
    with tiles.noise_frames(un2._handle(), frames):
        assert un2.decode_chains(B, H, W) == 1
        a = decode(d2, 0, B, **kw)
    with tiles.noise_frames(un1._handle(), frames):
        b = decode(d1, 0, B, **kw)
    np.testing.assert_array_equal(a, b)
    assert un2.decode_chains(B, H, W) == 2
    np.testing.assert_array_equal(decode(d2, 1, 2), decode(d1, 1, 2))
    # ... and a split decode after them is its halves again (the twin's program was dropped and comes back)
    np.testing.assert_array_equal(decode(d2, 0, 3), halves(d1, 3))


@pytest.mark.parametrize("change", ["weights", "arith", "steps"])
def test_twin_is_rebound_after_what_it_borrows_changed(change):
    """Decode split, change what the twin borrows -- other weights, the arithmetic, the schedule -- and decode again: the bits of a
    fresh handle that was given the same from the start."""
    B = 4
    un, d = model(2)
    decode(d, 0, B)
    seed, arith, steps = 0, None, STEPS
    if change == "weights":
        seed = 5
        un.load_state_dict(synth.unet_state_dict(MAN, seed=seed))
    elif change == "arith":
        arith = 0
        _lib.check(un._handle(), _lib.lib().cdc_set_arith(un._handle(), 0))
    else:
        steps = 4
        d.set_sample_schedule(steps)
    got = decode(d, 0, B)
    fresh = decode(model(2, seed=seed, arith=arith, steps=steps)[1], 0, B)
    np.testing.assert_array_equal(got, fresh)
    np.testing.assert_array_equal(got, halves(model(1, seed=seed, arith=arith, steps=steps)[1], B))


def test_destroying_a_handle_with_a_twin_frees_what_it_owns_and_nothing_else():
    """Device memory in use after a handle is gone: the same whether it never split, split (a twin with a program), or split and
    then dropped the twin's program -- the twin frees all it owns and no borrowed pointer (a double free would fail the destroy or
    the next allocation; a leak shows in the count)."""
    import torch

    def free_after(chains, then_unsplit=False):
        un, d = model(chains)
        decode(d, 0, 4)
        if then_unsplit:
            un.set_decode_chains(1)
            decode(d, 0, 4)
        un._lh.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    free_after(2)                       # (first use of the device: code objects, the runtime's own pools)
    never = free_after(1)
    assert free_after(2) == never
    assert free_after(2, then_unsplit=True) == never
    assert free_after(1) == never
