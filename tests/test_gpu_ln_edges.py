"""The stand-alone channel LayerNorm (csrc/aux_kernels.hip: ln_kernel, ln_kernel_sliced<PL, NP>, ln_kernel_vec<COLS, NP>, 25
instantiations behind ln_form) and the split-K sum pass (copy_kernel<PARTS, V>) on the MI355X, against the float64 statement and the
derived element-wise bound of tests/ln_ref.py: every instantiation, the production rule's own choices, ragged channel and pixel
counts, the slices summed on load, the statistics-only pass, the statistics of the final values, the in-place call, the ReLU / shift /
residual epilogue, the image-major grid, and the range-guard flag.  Every test first asserts through Ops.ln_form that it runs the form
it names.  What is not a rounding question is bit for bit: slices against their float32 sum, a pixel permutation, in place against
out of place, the two grid orders, the `constant` and `index` closed forms, repetitions, the sum pass.

The preconditions are tests/test_ln_ref_host.py's.  Every figure is printed before it is asserted (run with -s); the module prints the
worst fraction of the bound per group, the distance to the float32 restatement of each kind's summation order (a figure, not a
check) and its wall time at the end; the figures of the MI355X are in profiles/ln_edges.md.

Shapes: B = 2 and the smallest C / HW that reach the path, except ln_kernel_sliced<32, .>, which the rule picks only for HW > 64 and
ceil(HW / 32) B >= 256 and no switch forces: its cases run B = 86 images of 65 pixels (B = 32 / 29 at 256 / 260 pixels)."""
import time

import numpy as np
import pytest

from cdc_compression_amd.ops import Ops
from ln_ref import (CHANNEL_EDGES, PIXEL_EDGES, RULE_SHAPES, bits, constant_closed_form, final_stats_f64, index_closed_form, ln_bound, ln_case,
                    ln_f32, ln_f64, ln_x, sum_slices32, ulp_distance, worst_fraction)

pytestmark = pytest.mark.gpu

SWITCHES = ("CDC_NO_LN_VEC", "CDC_LN_VEC_COLS", "CDC_LN_NO_IMG_MAJOR")
CLEAN = {"arith": 1, "range_faults": 0, "nonfinite_results": 0}
WORST, RESTATED = {}, {}


@pytest.fixture(scope="module")
def G():
    return Ops(0)


@pytest.fixture(scope="module", autouse=True)
def summary():
    t0 = time.time()
    yield
    for group in sorted(WORST):
        print(f"[ln-edges] summary {group}: worst fraction of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST[group].items())))
    for kind, cls in sorted(RESTATED):
        print(f"[ln-edges] summary kind {kind}, {cls}: largest distance of y to the float32 restatement {RESTATED[kind, cls][0]} ulp, "
              f"{RESTATED[kind, cls][1]:.3f} of the bound")
    print(f"[ln-edges] summary wall time of the module {time.time() - t0:.1f} s")


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def force(monkeypatch, kind, width):
    """The switches that make the rule choose (kind, width) where it can be forced; ln_kernel_sliced<32> and ln_kernel are reached by shape."""
    if kind == 2:
        monkeypatch.setenv("CDC_LN_VEC_COLS", str(width))
    elif kind == 1:
        monkeypatch.setenv("CDC_NO_LN_VEC", "1")


def runs(G, case, want):
    """Asserts the form (kind, width, np, img_major) of the launch over `case`; -> it."""
    K, B, C, _, HW = case["slices"].shape
    form = G.ln_form(B, C, HW, K)
    print(f"[ln-edges] form of B={B} C={C} HW={HW} K={K}: kind {form[0]} width {form[1]} np {form[2]} img_major {form[3]}")
    assert form == tuple(want), (form, want)
    return form


def call(G, case, mode, in_place=False):
    """-> {"y", "mean", "rstd"} (what the mode has) of Ops.chan_layernorm_ex with ReLU, shift and residual."""
    s = case["slices"]
    x = s if len(s) > 1 else s[0]
    if mode == "stats":
        sm, sr = G.chan_layernorm_ex(x, want_y=False)
        return {"mean": sm, "rstd": sr}
    out = G.chan_layernorm_ex(x, case["g"], case["b"], True, case["shift"], case["resid"], in_place=in_place, want_stats=mode == "y+stats")
    return dict(zip(("y", "mean", "rstd"), out)) if mode == "y+stats" else {"y": out}


def note(group, key, f):
    WORST.setdefault(group, {})[key] = max(WORST.setdefault(group, {}).get(key, 0.0), f)


def held(G, case, mode, group, tag, form=None, in_place=False, cls=""):
    """One call against float64: y, the statistics of x (mode "stats") or of the final values (mode "y+stats")."""
    got = call(G, case, mode, in_place)
    s = case["slices"]
    tag = f"{group} {tag} {mode}"
    if mode == "stats":
        ref, bnd = ln_f64(s), ln_bound(s)
        note(group, "mean", worst_fraction(got["mean"], ref["mean"], bnd["mean"], tag + ": mean"))
        note(group, "rstd", worst_fraction(got["rstd"], ref["rstd"], bnd["rstd"], tag + ": rstd"))
        return got
    kw = dict(g=case["g"], b=case["b"], relu=True, shift=case["shift"], resid=case["resid"])
    bnd = ln_bound(s, **kw)["y"]
    note(group, "y", worst_fraction(got["y"], ln_f64(s, **kw)["y"], bnd, tag + ": y"))
    if mode == "y+stats":
        m, r, bm, br = final_stats_f64(got["y"])
        note(group, "final mean", worst_fraction(got["mean"], m, bm, tag + ": mean of the final values"))
        note(group, "final rstd", worst_fraction(got["rstd"], r, br, tag + ": rstd of the final values"))
    if form is not None:                                              # a figure: the float32 restatement in this kind's order
        r32 = ln_f32(s, form[0], form[1], **kw)["y"]
        d = (ulp_distance(got["y"], r32), float((np.abs(got["y"].astype(np.float64) - r32) / bnd).max()))
        RESTATED[form[0], cls] = max(RESTATED.get((form[0], cls), (0, 0.0)), d)
        print(f"[ln-edges] {tag}: y is {d[0]} ulp = {d[1]:.3f} of the bound from the float32 restatement of kind {form[0]} width {form[1]}")
    return got


def exact_index(got, case, tag):
    want = index_closed_form(case)
    same = bool(np.array_equal(bits(got["y"]), bits(want)))
    print(f"[ln-edges] {tag}: index closed form {'bit-equal' if same else 'NOT bit-equal, largest error %g' % np.abs(got['y'] - want).max()}")
    assert same, tag


def same_bits(a, b, tag):
    for k in a:
        same = bool(np.array_equal(bits(a[k]), bits(b[k])))
        print(f"[ln-edges] {tag}: {k} {'bit-equal' if same else 'NOT bit-equal, %d ulp' % ulp_distance(a[k], b[k])}")
        assert same, (tag, k)


def both_classes(G, B, C, HW, K, form, group, tag, modes=("y", "stats", "y+stats"), restate=True):
    for cls in ("normal", "index"):
        case = ln_case(cls, B, C, HW, K)
        runs(G, case, form)
        for mode in modes:
            got = held(G, case, mode, group, f"{tag} {cls} B={B} C={C} HW={HW} K={K}", form if restate and mode == "y" else None, cls=cls)
            if cls == "index" and mode != "stats":
                exact_index(got, case, f"{group} {tag} K={K} {mode}")
    assert G.status() == CLEAN, G.status()


# ---- (a) every instantiation ----------------------------------------------------------------------------------------------------
VEC = [(cols, n) for cols in (8, 4, 2) for n in (1, 2, 3, 4)] + [(2, 5), (2, 6)]


@pytest.mark.parametrize("cols,K", VEC, ids=["vec%d-np%d" % v for v in VEC])
def test_every_vec_instantiation(G, monkeypatch, cols, K):
    """ln_kernel_vec<COLS, NP>: 200 channels (two to seven rows per thread, the last partial), 72 pixels (a partial last workgroup)."""
    force(monkeypatch, 2, cols)
    both_classes(G, 2, 200, 72, K, (2, cols, K, 0), "(a)", f"vec<{cols},{K}>")


SLICED = [(pl, n) for pl in (8, 32) for n in (1, 2, 3, 4, 5)]


@pytest.mark.parametrize("pl,K", SLICED, ids=["pl%d-np%d" % v for v in SLICED])
def test_every_sliced_instantiation(G, pl, K):
    """ln_kernel_sliced<PL, NP>, five slices on the run-time loop (NP = 0); HW % 4 != 0 keeps the call off the 16-byte kernels."""
    B, C, HW = (2, 200, 70) if pl == 8 else (86, 27, 65)
    both_classes(G, B, C, HW, K, (1, pl, K if K <= 4 else 0, 0), "(a)", f"sliced<{pl},{K if K <= 4 else 0}>")


@pytest.mark.parametrize("HW", (5, 257))
@pytest.mark.parametrize("C", (385, 512))
def test_ln_kernel_both_blocks(G, C, HW):
    """ln_kernel (C > 384): 64-thread workgroups at 5 pixels, 256-thread ones at 257 (one pixel in the second)."""
    both_classes(G, 2, C, HW, 1, (0, 256 if HW >= 256 else 64, 1, 0), "(a)", "ln_kernel")


# ---- (b) the production rule with no switch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,want", RULE_SHAPES, ids=["B%d-HW%d" % s[:2] for s in RULE_SHAPES])
def test_the_forms_the_rule_picks(G, B, HW, want):
    kind, width, img = want
    both_classes(G, B, 24 if B >= 32 else 40, HW, 1, (kind, width, 1, img), "(b)", "rule", modes=("stats", "y+stats"), restate=False)


# ---- (c) channel edges ----------------------------------------------------------------------------------------------------------
WIDTHS = ((2, 8), (2, 4), (2, 2), (1, 8), (1, 32))


@pytest.mark.parametrize("kind,width", WIDTHS, ids=["kind%d-w%d" % w for w in WIDTHS])
@pytest.mark.parametrize("C", CHANNEL_EDGES)
def test_channel_edges(G, monkeypatch, C, kind, width):
    """The masks c < C of empty and partial channel rows: 12 pixels on the 16-byte kernels, 9 on ln_kernel_sliced<8>, 86 x 65 on <32>."""
    force(monkeypatch, kind, width)
    B, HW = (2, 12) if kind == 2 else ((2, 9) if width == 8 else (86, 65))
    both_classes(G, B, C, HW, 1, (kind, width, 1, 0), "(c)", f"kind {kind} width {width}", modes=("y+stats",), restate=False)


# ---- (d) pixel edges ------------------------------------------------------------------------------------------------------------
def pixel_edge_forms(HW):
    """[(B, switches' target or None, form)]: the form the rule picks at B = 2, then every other width this pixel count can run."""
    if HW % 4 == 0:
        out = [(2, None, (2, 2, 1, 0)), (2, (2, 4), (2, 4, 1, 0)), (2, (2, 8), (2, 8, 1, 0)), (2, (1, 8), (1, 8, 1, 0))]
    else:
        out = [(2, None, (1, 8, 1, 0))]
    if HW > 64:
        out.append((-(-256 // -(-HW // 32)), (1, 32), (1, 32, 1, 0)))
    return out


@pytest.mark.parametrize("C", (48, 384))
@pytest.mark.parametrize("HW", PIXEL_EDGES)
def test_pixel_edges(G, monkeypatch, HW, C):
    """The masks p < HW: one pixel, a partial float4 column block, whole and partial workgroups of every width."""
    for B, target, form in pixel_edge_forms(HW):
        with monkeypatch.context() as m:
            if target:
                force(m, *target)
            both_classes(G, B, C, HW, 1, form, "(d)", f"kind {form[0]} width {form[1]}", modes=("y+stats",), restate=False)


# ---- (e) numerics ---------------------------------------------------------------------------------------------------------------
NUMERIC_FORMS = ((0, 64), (1, 8), (1, 32), (2, 2), (2, 8))         # one form of each kind, and the other width of the two cached kernels


@pytest.mark.parametrize("kind,width", NUMERIC_FORMS, ids=["kind%d-w%d" % f for f in NUMERIC_FORMS])
@pytest.mark.parametrize("cls", ("offset", "small", "wide", "big"))
def test_numerics(G, monkeypatch, cls, kind, width):
    """Cancellation in x - mean, eps against a vanishing variance, 32 binades in one sum, squares near 1e30; one and three slices."""
    force(monkeypatch, kind, width)
    B, HW = (86, 65) if (kind, width) == (1, 32) else (2, 12 if kind == 2 else 10)
    C = 385 if kind == 0 else (48 if cls == "offset" or B > 2 else 200)
    for K in ((1,) if kind == 0 else (1, 3)):
        case = ln_case(cls, B, C, HW, K)
        form = runs(G, case, (kind, width, K, 0))
        for mode in ("y", "stats", "y+stats"):
            held(G, case, mode, "(e)", f"{cls} kind {kind} width {width} C={C} K={K}", form if mode == "y" else None, cls=cls)
    assert G.status() == CLEAN, G.status()


# ---- (f) bit for bit ------------------------------------------------------------------------------------------------------------
SUMMED = [(kind, width, K) for kind, width in ((2, 2), (2, 4), (2, 8), (1, 8), (1, 32)) for K in (2, 3, 4, 5, 6)
          if not (kind == 2 and width > 2 and K > 4)]               # (five and six slices exist at COLS 2 only)


@pytest.mark.parametrize("kind,width,K", SUMMED, ids=["kind%d-w%d-K%d" % s for s in SUMMED])
def test_slices_equal_their_float32_sum(G, monkeypatch, kind, width, K):
    """K slices summed on load (compiled counts and the run-time loop) against the one pre-summed slice on the same kind, width and grid.

    (Found by this test: left to the compiler's choice of fused pairs, ln_kernel_vec<4, 1> and <8, 1> differed from their NP > 1
    siblings by a rounding, up to 256 ulp at a result near zero; the kernel now fuses nothing, profiles/ln_edges.md.)"""
    force(monkeypatch, kind, width)
    B, C, HW = (86, 27, 65) if (kind, width) == (1, 32) else (2, 200, 72 if kind == 2 else 70)
    case = ln_case("normal", B, C, HW, K)
    one = dict(case, slices=sum_slices32(case["slices"])[None])
    runs(G, case, (kind, width, K if (kind == 2 or K <= 4) else 0, 0))
    runs(G, one, (kind, width, 1, 0))
    for mode in ("y+stats", "stats"):
        same_bits(call(G, case, mode), call(G, one, mode), f"(f) K={K} kind {kind} width {width} {mode} against the pre-summed slice")
    assert G.status() == CLEAN, G.status()


FORMS3 = ((0, 64, 2, 385, 9), (1, 8, 3, 200, 70), (1, 32, 86, 27, 65), (2, 2, 3, 200, 72), (2, 8, 3, 200, 72))


@pytest.mark.parametrize("kind,width,B,C,HW", FORMS3, ids=["kind%d-w%d" % f[:2] for f in FORMS3])
def test_pixel_permutation_and_in_place(G, monkeypatch, kind, width, B, C, HW):
    """A pixel is on its own: permuting the pixels of the input permutes the bits of the output, in every image; and the in-place
    call the model makes gives the bits of the out-of-place one."""
    force(monkeypatch, kind, width)
    case = ln_case("normal", B, C, HW)
    form = runs(G, case, (kind, width, 1, 0))
    base = held(G, case, "y+stats", "(f)", f"kind {kind} width {width}")
    perm = np.random.default_rng(HW).permutation(HW)
    assert (perm != np.arange(HW)).mean() > 0.9
    moved = dict(case, slices=case["slices"][..., perm].copy(), resid=case["resid"][..., perm].copy())
    assert runs(G, moved, form) == form
    got = call(G, moved, "y+stats")
    same_bits(got, {k: v[..., perm] for k, v in base.items()}, f"(f) kind {kind} width {width}: pixels permuted")
    same_bits(call(G, case, "y+stats", in_place=True), base, f"(f) kind {kind} width {width}: in place")
    same_bits(call(G, moved, "stats"), {k: v[..., perm] for k, v in call(G, case, "stats").items()},
              f"(f) kind {kind} width {width}: statistics only, pixels permuted")
    assert G.status() == CLEAN, G.status()


@pytest.mark.parametrize("B,HW,cols", ((8, 16, 2), (16, 256, 4), (8, 72, 4)))
def test_image_major_grid_equals_the_other_order(G, monkeypatch, B, HW, cols):
    if (B, HW) == (8, 72):
        monkeypatch.setenv("CDC_LN_VEC_COLS", "4")
    case = ln_case("normal", B, 40, HW, 2)
    runs(G, case, (2, cols, 2, 1))
    a = held(G, case, "y+stats", "(f)", f"image-major B={B} HW={HW}")
    exact_index(call(G, ln_case("index", B, 40, HW, 2), "y"), ln_case("index", B, 40, HW, 2), f"(f) image-major B={B} HW={HW}")
    monkeypatch.setenv("CDC_LN_NO_IMG_MAJOR", "1")
    runs(G, case, (2, cols, 2, 0))
    same_bits(call(G, case, "y+stats"), a, f"(f) B={B} HW={HW} COLS {cols}: CDC_LN_NO_IMG_MAJOR=1 against the image-major grid")
    assert G.status() == CLEAN, G.status()


CONSTANT = ((0, 64, 512, 9), (0, 256, 512, 257), (1, 8, 64, 9), (1, 32, 64, 65), (2, 2, 64, 12), (2, 4, 256, 12), (2, 8, 32, 36))


@pytest.mark.parametrize("kind,width,C,HW", CONSTANT, ids=["kind%d-w%d" % f[:2] for f in CONSTANT])
def test_constant_has_its_closed_form(G, monkeypatch, kind, width, C, HW):
    force(monkeypatch, kind, width)
    B = 86 if (kind, width) == (1, 32) else 2
    case = ln_case("constant", B, C, HW)
    runs(G, case, (kind, width, 1, 0))
    st = held(G, case, "stats", "(f)", f"constant kind {kind} width {width}")
    same_bits({"mean": st["mean"]}, {"mean": np.full_like(st["mean"], 0.75)}, f"(f) constant kind {kind} width {width}")
    got = held(G, case, "y+stats", "(f)", f"constant kind {kind} width {width}")
    same_bits({"y": got["y"]}, {"y": constant_closed_form(case)}, f"(f) constant kind {kind} width {width}: b, ReLU, + shift, + resid")
    assert G.status() == CLEAN, G.status()


REPEATED = ((2, 385, 9, 1, (0, 64, 1, 0)), (2, 200, 70, 5, (1, 8, 0, 0)), (2, 200, 70, 1, (1, 8, 1, 0)), (8, 200, 72, 3, (2, 2, 3, 1)),
            (8, 200, 72, 1, (2, 2, 1, 1)))


@pytest.mark.parametrize("B,C,HW,K,form", REPEATED, ids=["kind%d-K%d" % (r[4][0], r[3]) for r in REPEATED])
def test_repetitions_reproduce_their_bits(G, B, C, HW, K, form):
    """200 repetitions on the device, each against the first (cdc_op_stress); the in-place program starts from x every time."""
    kind = form[0]
    case = ln_case("normal", B, C, HW, K)
    runs(G, case, form)
    G.stress(200)
    try:
        for mode, in_place in (("y+stats", False), ("stats", False)) + ((("y+stats", True),) if K == 1 else ()):
            call(G, case, mode, in_place)
            print(f"[ln-edges] (f) stress kind {kind} {mode}{' in place' if in_place else ''}: {G.stress_result()}")
            assert G.stress_result() == (200, 0)
    finally:
        G.stress(0)
    assert G.status() == CLEAN, G.status()


# ---- (g) the sum pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("parts", (1, 2, 3, 4, 5))
def test_sum_pass_equals_the_serial_float32_sum(G, parts, B):
    """copy_kernel<PARTS, float4> (n % 4 == 0), <0, float4> (five slices) and <0, float> (every other n), slice order."""
    for n in (1, 3, 4, 5, 1024, 1027):
        x = ln_x("wide", parts * B, 1, n).reshape(parts, B, n)
        same_bits({"sum": G.sum_slices(x)}, {"sum": sum_slices32(x)}, f"(g) parts={parts} B={B} n={n}")
    assert G.status() == CLEAN, G.status()


def test_sum_pass_second_trip_of_the_grid_stride_loop(G):
    n = 4 * (2048 * 256) + 8                                         # 2048 workgroups of 256 float4: two more float4 on a second trip
    x = ln_x("normal", 2, 1, n).reshape(2, 1, n)
    got = G.sum_slices(x)
    same_bits({"sum": got}, {"sum": sum_slices32(x)}, f"(g) parts=2 B=1 n={n}")
    assert np.array_equal(bits(got[0, -8:]), bits(x[0, 0, -8:] + x[1, 0, -8:]))
    assert G.status() == CLEAN, G.status()


# ---- (h) the range-guard flag ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C,HW", ((0, 386, 9), (1, 48, 18), (2, 48, 16)))
def test_range_guard_flag_and_the_other_pixels(G, kind, C, HW):
    """A numeric flag, no GPU fault: one pixel of +-2^64 (finite input, variance 2^128 overflows; y stays finite, so only the kernel's
    flag can tell) and one pixel with a NaN channel (NaN statistics; in y the ReLU's fmaxf turns it into 0, so the flag again).  Each call is counted once in nonfinite_results, the handle is back in F16X2 with
    range_faults unchanged, and every other pixel holds the bits of the run without the hostile pixel."""
    B = 2
    case = ln_case("normal", B, C, HW)
    form = runs(G, case, ((0, 64, 1, 0), (1, 8, 1, 0), (2, 2, 1, 0))[kind])
    clean = {mode: call(G, case, mode) for mode in ("y", "stats")}
    assert G.status() == CLEAN
    F, count = Ops(0), 0
    for what in ("overflow", "nan"):
        s = case["slices"].copy()
        if what == "overflow":
            s[0, 1, :, 0, HW - 1] = np.where(np.arange(C) % 2 == 0, 2.0 ** 64, -(2.0 ** 64)).astype(np.float32)
        else:
            s[0, 0, C // 2, 0, 2] = np.nan
        b, p = (1, HW - 1) if what == "overflow" else (0, 2)
        hostile = dict(case, slices=s)
        assert runs(F, hostile, form) == form
        for mode in ("y", "stats"):
            got = call(F, hostile, mode)
            count += 1
            print(f"[ln-edges] (h) kind {kind} {what} {mode}: status {F.status()}")
            assert F.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": count}, F.status()
            for k, v in got.items():
                keep = np.ones(v.shape, bool)
                keep[b, ..., p] = False
                same = bool(np.array_equal(bits(v)[keep], bits(clean[mode][k])[keep]))
                print(f"[ln-edges] (h) kind {kind} {what} {mode}: other pixels of {k} bit-equal to the clean run: {same}")
                assert same and np.isfinite(v[keep]).all()
                if what == "nan" and mode == "stats":                 # (in y, fmaxf(NaN, 0) = 0: the ReLU hides it, the flag does not)
                    assert np.isnan(v[b, ..., p]).all()
    assert G.status() == CLEAN
