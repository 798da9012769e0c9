"""What tests/test_gpu_ln_edges.py leans on, asserted without a GPU: float32 restatements of the three LayerNorm kernels' summation
orders stay inside the bound of tests/ln_ref.py on every class, `constant` and `index` have their exact closed forms, the slices keep
their promises, wrong variants of the arithmetic leave the bound on the class that is there for them, Ops.ln_form is the rule
ln_launch held before ln_form owned it, and the new entry points refuse what they say they refuse."""
import itertools

import numpy as np
import pytest

from cdc_compression_amd import _lib
from cdc_compression_amd.ops import Ops
from ln_ref import (CLASSES, NUMERIC_CLASSES, bits, constant_closed_form, final_stats_f64, fraction, index_closed_form, ln_bound, ln_case,
                    ln_f32, ln_f64, old_form, sum_slices32, worst_fraction)

FORMS = ((0, 64), (1, 8), (1, 32), (2, 2), (2, 4), (2, 8))           # (kind, width) of the restatements


def _shape(cls, C):
    return 2, (64 if cls == "constant" else C), 12


def _call(case, **kw):
    return dict(g=case["g"], b=case["b"], relu=True, shift=case["shift"], resid=case["resid"], **kw)


@pytest.mark.parametrize("cls,C,K", [(cls, C, K) for cls in CLASSES for C in (48, 384) for K in (1, 3, 6)
                                     if not (cls == "offset" and C > 64)])       # (offset is used at C <= 64)
def test_float32_restatements_stay_inside_the_bound(cls, C, K):
    B, C, HW = _shape(cls, C)
    case = ln_case(cls, B, C, HW, K)
    ref, bnd = ln_f64(case["slices"], **_call(case)), ln_bound(case["slices"], **_call(case))
    worst = {}
    for kind, width in FORMS:
        got = ln_f32(case["slices"], kind, width, **_call(case))
        tag = f"{cls} C={C} K={K} kind {kind} width {width}"
        worst["y"] = max(worst.get("y", 0), worst_fraction(got["y"], ref["y"], bnd["y"], tag + " y"))
        worst["mean"] = max(worst.get("mean", 0), worst_fraction(got["mean"], ref["mean"], bnd["mean"], tag + " mean"))
        worst["rstd"] = max(worst.get("rstd", 0), worst_fraction(got["rstd"], ref["rstd"], bnd["rstd"], tag + " rstd"))
        fin = ln_f32(case["slices"], kind, width, **_call(case, want_final_stats=True))
        m, r, bm, br = final_stats_f64(fin["y"])
        worst_fraction(fin["mean"], m, bm, tag + " mean of the final values")
        worst_fraction(fin["rstd"], r, br, tag + " rstd of the final values")
    print(f"[ln-ref] {cls} C={C} K={K}: worst fractions {worst}")


@pytest.mark.parametrize("C", (32, 64, 256, 512))
def test_constant_has_its_closed_form(C):
    case = ln_case("constant", 2, C, 9)
    want = constant_closed_form(case)
    for kind, width in (FORMS if C <= 384 else FORMS[:1]):           # (the cached kernels end at 384 channels)
        got = ln_f32(case["slices"], kind, width, **_call(case))
        assert np.array_equal(bits(got["mean"]), bits(np.full_like(got["mean"], 0.75)))
        assert np.array_equal(bits(got["y"]), bits(want))
    assert np.abs(ln_f64(case["slices"], **_call(case))["y"] - want).max() < 1e-6


@pytest.mark.parametrize("K", (1, 4))
def test_index_is_exact_and_moves_by_at_least_one(K):
    B, C, HW = 3, 40, 12
    case = ln_case("index", B, C, HW, K)
    want = index_closed_form(case)
    assert want.max() < 2 ** 24 and np.array_equal(want, np.round(want))
    assert np.array_equal(ln_f64(case["slices"], **_call(case))["y"], want.astype(np.float64))
    for kind, width in FORMS:
        assert np.array_equal(bits(ln_f32(case["slices"], kind, width, **_call(case))["y"]), bits(want))
    flat = want.reshape(-1)
    assert len(np.unique(flat)) > 0.9 * flat.size                    # (channels 0 ... 8 share relu(b_c) = 0 but not shift and resid)
    for wrong in (np.roll(want, 1, axis=0), np.roll(want, 1, axis=1), np.roll(want, 1, axis=3)):
        assert (np.abs(wrong - want) >= 1).all()
    bnd = ln_bound(case["slices"], **_call(case))["y"]
    assert bnd.max() < 0.5                                           # the bound itself sees an error of 1


@pytest.mark.parametrize("cls", CLASSES)
def test_slices_and_results_meet_their_preconditions(cls):
    for C in ((48,) if cls == "offset" else (48, 384)):
        B, C, HW = _shape(cls, C)
        for K in (1, 2, 6):
            case = ln_case(cls, B, C, HW, K)
            s = case["slices"]
            x = ln_case(cls, B, C, HW, 1)["slices"][0]
            assert s.dtype == np.float32 and np.isfinite(s).all()
            assert (np.abs(s) <= np.abs(x)[None]).all()              # no slice exceeds |x|
            assert (np.sign(s) * np.sign(x)[None] >= 0).all()        # ... nor changes side
            assert np.abs(s.astype(np.float64).sum(0) - x).max() <= 2 * K * 2.0 ** -24 * np.abs(x).max()
            nz = np.abs(x[x != 0])
            assert nz.max() < 2.0 ** 127 and nz.min() > 2.0 ** -126
            y = ln_f64(s, **_call(case))["y"]
            assert np.isfinite(y).all() and np.abs(y).max() < 2.0 ** 127
    if cls == "offset":
        case = ln_case(cls, 2, 48, 12)
        bnd = ln_bound(case["slices"], **_call(case))["y"]               # yhat has unit variance: the bound still sees 2 % of it
        print(f"[ln-ref] offset C=48: bound at most {float(bnd.max()):.2e}, median {float(np.median(bnd)):.2e} (yhat has unit variance)")
        assert bnd.max() < 0.02 and np.median(bnd) < 0.01


def test_sum_slices32_is_the_serial_float32_sum():
    s = ln_case("wide", 2, 5, 7, 4)["slices"]
    want = ((s[0] + s[1]) + s[2]) + s[3]
    assert want.dtype == np.float32 and np.array_equal(bits(sum_slices32(s)), bits(want))
    assert not np.array_equal(bits(want), bits(s[0] + (s[1] + (s[2] + s[3]))))      # the order is visible


WRONG = (        # (variant, class, C, what must leave the bound)
    ("one-pass variance", dict(one_pass=True), "offset", 48, "y"),
    ("eps outside the root", dict(eps_outside=True), "small", 48, "y"),
    ("eps = 1e-6", dict(eps=np.float32(1e-6)), "small", 48, "y"),
    ("division by C - 1", dict(ddof=1), "normal", 48, "y"),
    ("final statistics before the residual", dict(want_final_stats=True, stats_before_resid=True), "normal", 48, "final"),
)


@pytest.mark.parametrize("name,kw,cls,C,what", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_variants_leave_the_bound(name, kw, cls, C, what):
    case = ln_case(cls, 2, C, 12)
    ref, bnd = ln_f64(case["slices"], **_call(case)), ln_bound(case["slices"], **_call(case))
    for kind, width in FORMS:
        got = ln_f32(case["slices"], kind, width, **_call(case, **kw))
        if what == "final":
            m, r, bm, br = final_stats_f64(got["y"])
            f = max(fraction(got["mean"], m, bm), fraction(got["rstd"], r, br))
        else:
            f = fraction(got["y"], ref["y"], bnd["y"])
        print(f"[ln-ref] {name} on {cls} C={C}, kind {kind} width {width}: {f:.3g} of the bound")
        assert f > 10.0, (name, kind, width, f)


GRID_B = (1, 2, 7, 8, 16, 17, 32, 86, 256)
GRID_C = (1, 40, 384, 385)
GRID_HW = (1, 4, 8, 9, 16, 17, 63, 64, 65, 68, 256, 257, 4096)
SWITCHES = ({}, {"CDC_NO_LN_VEC": "1"}, {"CDC_LN_VEC_COLS": "8"}, {"CDC_LN_VEC_COLS": "4"}, {"CDC_LN_VEC_COLS": "2"}, {"CDC_LN_VEC_COLS": "3"},
            {"CDC_LN_NO_IMG_MAJOR": "1"}, {"CDC_LN_VEC_COLS": "2", "CDC_LN_NO_IMG_MAJOR": "1"})


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: "+".join(f"{k}={v}" for k, v in e.items()) or "unset")
def test_ln_form_is_the_former_rule(monkeypatch, env):
    assert all(n in _lib.EXPORTS and hasattr(_lib.lib(), n) for n in ("cdc_op_ln_form", "cdc_op_chan_layernorm_ex", "cdc_op_sum_slices"))
    for k in ("CDC_NO_LN_VEC", "CDC_LN_VEC_COLS", "CDC_LN_NO_IMG_MAJOR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(no_vec="CDC_NO_LN_VEC" in env, vec_cols=int(env.get("CDC_LN_VEC_COLS", 0)), no_img_major="CDC_LN_NO_IMG_MAJOR" in env)
    G, seen = Ops(0), set()
    for B, C, HW, nparts, aligned in itertools.product(GRID_B, GRID_C, GRID_HW, range(1, 8), (True, False)):
        if C > 384 and nparts > 1:
            continue
        got = G.ln_form(B, C, HW, nparts, aligned)
        assert got == old_form(B, C, HW, nparts, aligned, **kw), (B, C, HW, nparts, aligned, got)
        seen.add(got)
    print(f"[ln-ref] {env or 'unset'}: {len(seen)} distinct forms over the grid")
    if not env:                                                      # every instantiation but the forced ones is in the grid
        assert {(2, c, n) for c in (2, 4, 8) for n in (1, 2, 3, 4)} | {(2, 2, 5), (2, 2, 6)} <= {s[:3] for s in seen}
        assert {(1, p, n) for p in (8, 32) for n in range(5)} | {(0, 64, 1), (0, 256, 1)} <= {s[:3] for s in seen}
        assert {s[3] for s in seen} == {0, 1}


def test_ln_form_at_the_shapes_the_gpu_file_names():
    from ln_ref import RULE_SHAPES
    G = Ops(0)
    for B, HW, (kind, width, img) in RULE_SHAPES:
        for C in (40, 24):
            assert G.ln_form(B, C, HW) == (kind, width, 1, img), (B, C, HW)


def test_the_new_entry_points_refuse_before_any_launch():
    G, L = Ops(0), _lib.lib()
    h = G._h
    f = np.zeros(64, np.float32)
    p, N = f.ctypes.data, None

    def ex(x=p, nparts=1, g=p, b=p, in_place=0, y=p, sm=N, sr=N, B=1, C=4, HW=4):
        return L.cdc_op_chan_layernorm_ex(h, x, nparts, g, b, 0, N, N, in_place, y, sm, sr, B, C, HW)
    for bad, word in ((dict(x=N), b"x is null"), (dict(y=N), b"no output"), (dict(g=N), b"g and b"), (dict(b=N), b"g and b"),
                      (dict(in_place=1, nparts=2), b"in_place"), (dict(in_place=1, y=N, sm=p, sr=p), b"in_place"),
                      (dict(nparts=2, C=385), b"384"), (dict(B=0), b"start at 1"), (dict(C=0), b"start at 1"), (dict(HW=0), b"start at 1"),
                      (dict(nparts=0), b"start at 1")):
        assert ex(**bad) == -1 and word in L.cdc_last_error(h), (bad, L.cdc_last_error(h))
    assert L.cdc_op_chan_layernorm_ex(None, p, 1, p, p, 0, N, N, 0, p, N, N, 1, 4, 4) == -1
    for args in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 385, 4, 2)):
        assert L.cdc_op_ln_form(h, *args, 1, N, N, N, N) == -1, args
    assert L.cdc_op_ln_form(h, 1, 385, 4, 1, 1, N, N, N, N) == 0 and L.cdc_op_ln_form(h, 1, 384, 4, 7, 1, N, N, N, N) == 0
    assert L.cdc_op_ln_form(None, 1, 4, 4, 1, 1, N, N, N, N) == -1
    for args in ((N, 1, p, 1, 4), (p, 1, N, 1, 4), (p, 0, p, 1, 4), (p, 1, p, 0, 4), (p, 1, p, 1, 0)):
        assert L.cdc_op_sum_slices(h, *args) == -1, args
    assert G.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}
