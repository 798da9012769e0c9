"""Decode trajectory without a GPU: the argument rules of the three keywords (all ValueError, before anything runs), the expansion of
`trajectory=n`, and the agreement of include/cdc_hip.h and _lib.py on the new symbols."""
import os
import re

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, trajectory as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cdc_set_trace", "cdc_trace_info", "cdc_trace_read", "cdc_op_trace_tap"]


@pytest.mark.parametrize("steps,n,want", [
    (1, 1, [0]), (1, 3, [0]),
    (2, 1, [1, 0]), (2, 2, [1, 0]), (2, 5, [1, 0]),
    (5, 1, [4, 3, 2, 1, 0]), (5, 2, [4, 2, 0]), (5, 3, [4, 1, 0]), (5, 4, [4, 0]), (5, 8, [4, 0]),
    (6, 1, [5, 4, 3, 2, 1, 0]), (6, 2, [5, 3, 1, 0]), (6, 3, [5, 2, 0]), (6, 5, [5, 0]), (6, 6, [5, 0])])
def test_every_nth_step_from_the_first_plus_index_0(steps, n, want):
    got = T.expand(n, steps)
    assert got == want
    assert got[0] == steps - 1 and got[-1] == 0 and len(set(got)) == len(got)
    assert T.expand(np.int64(n), steps) == want


def test_a_sequence_is_taken_in_execution_order():
    assert T.expand([0, 4], 6) == [4, 0]
    assert T.expand((3,), 6) == [3]
    assert T.expand(np.array([1, 5, 2]), 6) == [5, 2, 1]
    assert T.expand(range(6), 6) == [5, 4, 3, 2, 1, 0]


@pytest.mark.parametrize("bad", [[6], [-1], [0, 0], [4, 2, 4], 0, -2, True, False, [True], [1.0], "x0", 2.5, []])
def test_indices_outside_the_schedule_repeated_or_of_the_wrong_kind(bad):
    with pytest.raises(ValueError):
        T.expand(bad, 6)


def test_check_args():
    assert T.check_args(None, "x0", "float32", 6) is None
    s = T.check_args(2, "both", "uint8", 6)
    assert s.indices == [5, 3, 1, 0] and s.u8
    assert s.what == _lib.CDC_TRACE_X0 | _lib.CDC_TRACE_XT | _lib.CDC_TRACE_U8
    assert T.check_args([0], "x_t", "float32", 6).what == _lib.CDC_TRACE_XT
    assert T.check_args(1, "x0", "float32", 2, eta=0.5, seed=3).indices == [1, 0]
    for kw in (dict(trajectory_of="x"), dict(trajectory_dtype="float16"), dict(samples=4), dict(eta=0.5), dict(samples=1, seed=1)):
        args = dict(trajectory=1, trajectory_of="x0", trajectory_dtype="float32", steps=6)
        args.update(kw)
        with pytest.raises(ValueError):
            T.check_args(**args)
    with pytest.raises(ValueError):                     # the other two keywords belong to trajectory=
        T.check_args(None, "both", "float32", 6)
    with pytest.raises(ValueError):
        T.check_args(None, "x0", "uint8", 6)


def test_the_calls_refuse_before_anything_runs():
    """No library handle is made: the Unet mirror creates it on first use, and every rule is checked before that."""
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    ctx = [np.zeros((2, 8, 32, 32), np.float32), np.zeros((2, 16, 16, 16), np.float32)]
    shape = (2, 3, 32, 32)
    for diff, loop_args in ((cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine"), (True,)),
                            (cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, pred_mode="noise", var_schedule="linear"), ("ddim",))):
        for kw in (dict(trajectory=[6]), dict(trajectory=[0, 0]), dict(trajectory=0), dict(trajectory=True),
                   dict(trajectory=1, samples=2, seed=1, gamma=1.0), dict(trajectory=1, eta=0.5), dict(trajectory=1, trajectory_of="x1"),
                   dict(trajectory=1, trajectory_dtype="int8"), dict(trajectory_of="both")):
            with pytest.raises(ValueError):
                diff.decompress(ctx, shape, sample_steps=6, **kw)
        images = np.zeros(shape, np.float32)
        for kw in (dict(trajectory=[6]), dict(trajectory=1, eta=0.5), dict(trajectory=False)):
            with pytest.raises(ValueError):
                diff.compress(images, sample_steps=6, **kw)
            with pytest.raises(ValueError):
                diff.evaluate(images, sample_steps=6, **kw)
        with pytest.raises(ValueError):                 # p_sample_loop follows set_sample_schedule, which gives the number of steps
            diff.p_sample_loop(shape, ctx, *loop_args, trajectory=1)
        diff.sample_steps = 6                           # (what set_sample_schedule records)
        for kw in (dict(trajectory=[6]), dict(trajectory=[1, 1]), dict(trajectory=1, eta=0.5), dict(trajectory=-1)):
            with pytest.raises(ValueError):
                diff.p_sample_loop(shape, ctx, *loop_args, **kw)
    assert un._lh.raw is None                           # nothing reached the library


def test_header_and_binding_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "cdc_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTS
    for name, value in (("CDC_TRACE_X0", 1), ("CDC_TRACE_XT", 2), ("CDC_TRACE_U8", 4)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr), name
        assert getattr(_lib, name) == value
    L = _lib.lib()
    # argument counts: the header's parameter list against the binding's argtypes
    for name in NEW:
        params = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
        assert len(params.split(",")) == len(getattr(L, name).argtypes), name
