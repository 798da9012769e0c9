"""Residual(PreNorm(LinearAttention)) on the GPU against the float64 restatement of tests/attention_ref.py (which
tests/test_attention_host.py pins to the real reference's float64 run), on the inputs where a softmax kernel goes wrong and on every
attention path that Builder::attention (csrc/cdc_planner.hip) can choose: attention_ref.PATHS x (BASE_CASES, and `peak@n` where a
split holds more than one 32-pixel tile).  The planner's labels of every call are checked, so a case cannot end up on another kernel
than the one it names.

Bound, per case: max |got - ref64| / max(1, max |ref64|) <= max(5e-6, 3 e32).  5e-6 is the operator bound of tests/test_gpu_parity.py;
e32 (tests/golden/attention_edges.npz) is what the reference's own float32 evaluation loses on that case against float64, and 3x is
the project's margin over a measured figure: the kernels' operands carry 22-23 significant bits and their exponential is good to
2 ulp, so they are granted what float32 is and no more.  No bound exceeds 2.6e-5.

`background` is the case that a two-plane fp16 softmax weight with an absolute error gets wrong (csrc/attn_kernels.hip: kPScale); on
the fused kernels it needs splits of many tiles, which the planner makes at a large batch, and the feature first in its split
(`background@n` on the 16-tile path).  Every figure is printed and, with CDC_TEST_OBS=<file>, appended there; the worst per path and
case on an MI355X are in profiles/attention_edges.md."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import attention_ref as A
from cdc_compression_amd import _lib
from cdc_compression_amd.ops import Ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_edges.npz")
KINDS = ("kvctx", "kstats", "ctxp", "ctxr", "ctxf", "ctx1")


def _obs(what, err, bound):
    print(f"[attention] {what}: {err:.3g} (bound {bound:.3g})")
    obs = os.environ.get("CDC_TEST_OBS")
    if obs:
        with open(obs, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "what": what, "relerr": err, "bound": bound}) + "\n")
    return err


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=2)          # the paths that share a shape follow each other below: a reference is computed once
def _case(case, shape):
    args = A.build(case, shape)
    assert np.array_equal(A.checksum(args), _golden()[f"{A.entry_key(case, shape)}/sha"]), "the builder gives other inputs on this host"
    ref = A.reference(args)
    ref.setflags(write=False)
    return args, ref


def _labels(ops, first):
    L, out = _lib.lib(), []
    for i in range(first, L.cdc_prof_num_ops(ops._h)):
        lab = ctypes.c_char_p()
        L.cdc_prof_op(ops._h, i, ctypes.byref(lab), None, None, None)
        out.append(lab.value.decode())
    return out


def _params():
    shapes = []
    for _, shape, _, _, _ in A.PATHS:
        if shape not in shapes:
            shapes.append(shape)
    out = []
    for shape in shapes:
        rows = [p for p in A.PATHS if p[1] == shape]
        for case in sorted({c for p in rows for c in A.cases_of(p[0], shape, p[4])}, key=lambda c: ("@" in c, c)):
            for path, _, env, kinds, nsplit in rows:
                if case in A.cases_of(path, shape, nsplit):
                    tag = path + ("" if not env else "[" + ",".join(f"{k}={v}" for k, v in env.items()) + "]")
                    out.append(pytest.param(path, shape, env, kinds, nsplit, case, id=f"{tag}-{'x'.join(map(str, shape))}-{case}"))
    return out


@pytest.mark.parametrize("path,shape,env,kinds,nsplit,case", _params())
def test_attention_edge_case(path, shape, env, kinds, nsplit, case, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args, ref = _case(case, shape)
    B, C, H, W = shape
    ops = Ops(0)                               # (the arithmetic and the switches are read when the handle is created)
    arith = ops.status()["arith"]
    assert arith == (0 if env.get("CDC_ARITH") == "0" else 1)
    first = _lib.lib().cdc_prof_num_ops(ops._h)
    got = ops.linear_attention(*args)
    # the kernels that were planned: the kinds of this path, once each, with the split count that `peak@n` was built around
    planned = [l for l in _labels(ops, first) if l.split(" ")[0] in KINDS]
    assert planned == [f"{k} C={C} N={H * W} nsplit={nsplit}" for k in kinds], planned
    st = ops.status()
    assert st["nonfinite_results"] == 0 and st["range_faults"] == 0 and st["arith"] == arith, st
    assert got.shape == shape and got.dtype == np.float32 and np.isfinite(got).all()
    amax = float(np.abs(ref).max())
    assert amax < 1000.0
    e32 = float(_golden()[f"{A.entry_key(case, shape)}/e32"])
    bound = max(5e-6, 3 * e32)
    what = f"{path} {'x'.join(map(str, shape))} {case}"
    err = _obs(what, A.relerr(got, ref), bound)
    rows = np.abs(got.astype(np.float64) - ref).reshape(B, -1).max(1) / max(1.0, amax)          # a large batch repeats images: every row counts
    assert rows.max() == err
    if case == "flat":
        closed = _obs(what + " (closed form)", A.relerr(got, A.reference(args, A.flat_closed_form)), bound)
        assert closed <= bound, (what, closed, bound)
    assert err <= bound, (what, err, bound, "worst image", int(rows.argmax()))
