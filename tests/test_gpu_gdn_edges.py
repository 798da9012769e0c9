"""gdn_kernel (csrc/gdn_kernels.hip) against float64 where the suite did not reach: all sixteen instantiations, the pixel counts around
the tile and MFMA-column edges, second and later trips of the tile walk (forced through CDC_GDN_WGS and by the production rule, each
proven by per_image < tiles), a 0/1 gamma' that localises operand indexing, and the three promises of the kernel's header: a result
depends on its own pixel only, the fault flag on an overflowing inverse, the handle's counters after a non-finite input.

Bound (tests/gdn_ref.py, as tests/test_gpu_simple.py): element-wise relative error <= (C + 2) 2^-24 against the float64 evaluation of
the float32-reparametrised parameters; zeros are zeros of the same sign; everything else stated here is bit for bit.  The
preconditions (normal-range results, exact 0/1 and 0 gamma', the float32 restatement inside the bound) are tests/test_gdn_ref_host.py's.
Every figure is printed before it is asserted (run with -s); the figures of the MI355X are in profiles/gdn_edges.md.

The `perm` closed form x_i / fl(beta'_i + |x_pi(i)|) is the kernel's result bit for bit on the MI355X (profiles/gdn_edges.md): the
fp32 MFMA adds an exact-zero product without changing the accumulator and rounds the one non-zero accumulation as an fmaf does.  The
first run showed it at every width, both directions, so it is asserted."""
import os

import numpy as np
import pytest

from cdc_compression_amd.ops import Ops
from gdn_ref import (HOSTILE_SHAPE, PIXEL_EDGES, WALK_SHAPES, WIDTHS, below_closed_form, gdn_edge_case, gdn_f32_chain, gdn_f64, nonfinite_agree,
                     old_workgroups, perm_closed_form, ulp_distance, with_nonfinite, with_overflow, worst_fraction, zeros_agree)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return Ops(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def held(got, want, C, what, where=None):
    """Prints, then asserts: the float64 bound over `where` (default: everything), zeros of the same sign."""
    if where is not None:
        got, want = got[where], want[where]
    f = worst_fraction(got, want, C)
    print(f"[gdn-edges] {what}: worst error {f:.3f} of (C + 2) 2^-24")
    assert got.dtype == np.float32
    assert zeros_agree(got, want), what
    assert f <= 1.0, (what, f)


def closed_form(got, want32, what):
    d = ulp_distance(got, want32)
    print(f"[gdn-edges] {what}: closed form {'bit-equal' if np.array_equal(bits(got), bits(want32)) else 'NOT bit-equal'}, largest distance {d} ulp")
    np.testing.assert_array_equal(bits(got), bits(want32))


def run_both(G, cls, B, C, HW, what):
    """Forward and inverse of one case against float64 (and the closed form of its class); -> {inverse: result}."""
    x, beta, gamma = gdn_edge_case(cls, B, C, HW)
    out = {}
    for inverse in (False, True):
        tag = f"{what} {cls} B={B} C={C} HW={HW}{' inv' if inverse else ''}"
        got = G.gdn(x, beta, gamma, inverse)
        assert got.shape == x.shape
        held(got, gdn_f64(x, beta, gamma, inverse), C, tag)
        if cls == "perm":
            closed_form(got, perm_closed_form(x, beta, inverse), tag)
        if cls == "below":
            closed_form(got, below_closed_form(x, beta, inverse), tag)
        out[inverse] = got
    return out


# ---- (a) every instantiation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["dense", "perm"])
@pytest.mark.parametrize("C", WIDTHS)
def test_every_instantiation_against_float64(G, C, cls):
    """gdn_kernel<1> ... gdn_kernel<16> at one whole tile and a tail of 6 pixels: above 204 channels the tile needs more than 64 KB of
    LDS (ensure_dynamic_lds), C = 256 runs 1024-thread workgroups."""
    got = run_both(G, cls, 2, C, 70, "(a)")
    assert G.status()["nonfinite_results"] == 0 and G.status()["range_faults"] == 0
    if cls == "dense":      # a figure, not a check: how far the fp32 MFMA's sum is from an fmaf chain in ascending j (gdn_ref.gdn_f32_chain)
        x, beta, gamma = gdn_edge_case(cls, 2, C, 70)
        d = [ulp_distance(got[inv], gdn_f32_chain(x, beta, gamma, inv)) for inv in (False, True)]
        print(f"[gdn-edges] (a) dense C={C}: largest distance to the CPU's ascending-j fmaf chain {d[0]} ulp, inverse {d[1]} ulp")


@pytest.mark.parametrize("cls", ["wide", "below"])
@pytest.mark.parametrize("C", [16, 48, 256])
def test_wide_range_and_vanishing_gamma(G, C, cls):
    """`wide`: thirty decades in one sum.  `below`: gamma' = 0, the result is x / beta' (x * beta') bit for bit."""
    run_both(G, cls, 2, C, 70, "(a)")
    assert G.status()["nonfinite_results"] == 0 and G.status()["range_faults"] == 0


# ---- (b) pixel-count edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [48, 256])
@pytest.mark.parametrize("HW", PIXEL_EDGES)
def test_pixel_count_edges(G, HW, C):
    """The `ok` predicates of the staging and of the epilogue decide everything at 1, 16 +- 1, 64 +- 1 and 128 +- 1 pixels."""
    run_both(G, "normal", 2, C, HW, "(b)")
    assert G.status()["nonfinite_results"] == 0


# ---- (c) the tile walk, forced --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_workgroup_per_tile(G):
    """{(cls, B, C, HW): {inverse: result}} of the walk shapes by the default rule, where every tile has its own workgroup."""
    out = {}
    assert "CDC_GDN_WGS" not in os.environ
    for B, C, HW in WALK_SHAPES:
        assert G.gdn_workgroups(B, HW) == (-(-HW // 64),) * 2
        for cls in ("dense", "perm"):
            out[cls, B, C, HW] = run_both(G, cls, B, C, HW, "(c) one workgroup per tile")
    return out


@pytest.mark.parametrize("cls", ["dense", "perm"])
@pytest.mark.parametrize("shape", WALK_SHAPES, ids=lambda s: "B%d-C%d-HW%d" % s)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_forced_tile_walk(G, one_workgroup_per_tile, monkeypatch, n, shape, cls):
    """n workgroups per image walk 8 (4) tiles: the restaged LDS tile behind its barrier, gamma' and beta' kept in registers, p0 of a
    later trip.  Within the float64 bound, and the bits of the launch that gives every tile its own workgroup."""
    B, C, HW = shape
    monkeypatch.setenv("CDC_GDN_WGS", str(n))
    per_image, tiles = G.gdn_workgroups(B, HW)
    print(f"[gdn-edges] (c) CDC_GDN_WGS={n} B={B} C={C} HW={HW}: {per_image} workgroups per image over {tiles} tiles")
    assert per_image == n and per_image < tiles                       # not vacuous: some workgroup runs a second trip
    got = run_both(G, cls, B, C, HW, f"(c) {n} workgroups per image")
    for inverse in (False, True):
        np.testing.assert_array_equal(bits(got[inverse]), bits(one_workgroup_per_tile[cls, B, C, HW][inverse]))


# ---- (d) the tile walk, by the production rule ----------------------------------------------------------------------------------
def test_tile_walk_by_the_production_rule(G, monkeypatch):
    """No switch: B = ceil(4 CUs / 3) images leave each image 3 workgroups for its 8 tiles."""
    import torch
    monkeypatch.delenv("CDC_GDN_WGS", raising=False)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    B, C, HW = -(-4 * cus // 3), 16, 64 * 7 + 9
    per_image, tiles = G.gdn_workgroups(B, HW)
    print(f"[gdn-edges] (d) {cus} CUs, B={B} C={C} HW={HW}: {per_image} workgroups per image over {tiles} tiles")
    assert (per_image, tiles) == old_workgroups(HW, B, cus) and 1 < per_image < tiles
    x, beta, gamma = gdn_edge_case("dense", B, C, HW)
    picks = [0, B // 2, B - 1]
    for inverse in (False, True):
        got = G.gdn(x, beta, gamma, inverse)
        for b in picks:
            tag = f"(d) dense image {b} of {B}{' inv' if inverse else ''}"
            held(got[b:b + 1], gdn_f64(x[b:b + 1], beta, gamma, inverse), C, tag)
            assert G.gdn_workgroups(1, HW) == (tiles, tiles)
            np.testing.assert_array_equal(bits(got[b:b + 1]), bits(G.gdn(x[b:b + 1], beta, gamma, inverse)))
    assert G.status()["nonfinite_results"] == 0


# ---- (e) reproducibility of the walk --------------------------------------------------------------------------------------------
def test_one_workgroup_walk_reproduces_its_bits(G, monkeypatch):
    B, C, HW = WALK_SHAPES[0]
    monkeypatch.setenv("CDC_GDN_WGS", "1")
    assert G.gdn_workgroups(B, HW) == (1, 8)
    x, beta, gamma = gdn_edge_case("dense", B, C, HW)
    G.stress(200)
    try:
        G.gdn(x, beta, gamma)
        print(f"[gdn-edges] (e) stress under CDC_GDN_WGS=1: {G.stress_result()}")
        assert G.stress_result() == (200, 0)
    finally:
        G.stress(0)


# ---- (f) a pixel is on its own --------------------------------------------------------------------------------------------------
def test_a_non_finite_pixel_stays_on_its_own_and_is_counted(G):
    """+inf in the whole tile of image 0, NaN in the tail tile of image 1: every other pixel keeps the bits of the clean run; the two
    pixels hold what IEEE arithmetic gives them; a fresh handle counts each call in nonfinite_results and keeps its arithmetic."""
    B, C, HW = HOSTILE_SHAPE
    x0, beta, gamma = gdn_edge_case("normal", B, C, HW)
    x, hostile = with_nonfinite(x0)
    F = Ops(0)
    for k, inverse in enumerate((False, True)):
        tag = f"(f) normal B={B} C={C} HW={HW}{' inv' if inverse else ''}"
        clean = G.gdn(x0, beta, gamma, inverse)
        got = F.gdn(x, beta, gamma, inverse)
        want = gdn_f64(x, beta, gamma, inverse)
        same = bool(np.array_equal(bits(got)[~hostile], bits(clean)[~hostile]))
        print(f"[gdn-edges] {tag}: other pixels bit-equal to the clean run: {same}; hostile pixels: {int(np.isnan(got[hostile]).sum())} NaN, "
              f"{int(np.isinf(got[hostile]).sum())} inf, {int((got[hostile] == 0).sum())} zeros; status {F.status()}")
        assert same
        assert np.isfinite(got[~hostile]).all()
        assert nonfinite_agree(got, want)
        held(got, want, C, tag + ", hostile pixels", where=hostile)
        assert F.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": k + 1}, F.status()


# ---- (g) overflow of the inverse with finite inputs -----------------------------------------------------------------------------
def test_overflowing_inverse_sets_the_flag_and_touches_its_pixel_only(G):
    B, C, HW = HOSTILE_SHAPE
    x0, beta, gamma = gdn_edge_case("dense", B, C, HW)
    x, hostile = with_overflow(x0)
    F = Ops(0)
    fwd = F.gdn(x, beta, gamma, False)
    held(fwd, gdn_f64(x, beta, gamma, False), C, f"(g) dense B={B} C={C} HW={HW}, x = 1e30, forward")
    assert np.isfinite(fwd).all()
    assert F.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}, F.status()
    clean = G.gdn(x0, beta, gamma, True)
    got = F.gdn(x, beta, gamma, True)
    want = gdn_f64(x, beta, gamma, True)
    same = bool(np.array_equal(bits(got)[~hostile], bits(clean)[~hostile]))
    print(f"[gdn-edges] (g) inverse: other pixels bit-equal to the clean run: {same}; the pixel: {int(np.isinf(got[hostile]).sum())} inf of {C}; "
          f"status {F.status()}")
    assert same
    assert np.isposinf(got[0, 5, 0, 3]) and nonfinite_agree(got, want)
    with np.errstate(over="ignore"):
        fits = np.isfinite(want.astype(np.float32))
    held(got, want, C, "(g) inverse, the finite results of the pixel", where=hostile & fits)
    assert F.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 1}, F.status()


# ---- (h) in the model -----------------------------------------------------------------------------------------------------------
def test_model_results_do_not_depend_on_the_walk(monkeypatch):
    """simple_small: analysis(x) and decode(q) with 1 and 3 workgroups per image, from a freshly built model each, are the bits of
    the default run (which tests/test_gpu_simple.py holds to the goldens)."""
    from test_gpu_simple import _inputs, _load, _model
    meta, _ = _load("simple_small")
    x, q, _ = _inputs(meta)

    def run():
        m = _model(meta)
        return [np.asarray(a) for a in m.analysis(x)] + [np.asarray(a) for a in m.decode(q)]
    monkeypatch.delenv("CDC_GDN_WGS", raising=False)
    base = run()
    B, G = meta["image_shape"][0], Ops(0)
    for n in ("1", "3"):
        monkeypatch.setenv("CDC_GDN_WGS", n)
        grids = [G.gdn_workgroups(B, HW) for HW in (2048, 512, 128)]  # the three GDN levels (test_simple_programs_run_the_gdn_kernel)
        print(f"[gdn-edges] (h) CDC_GDN_WGS={n}: (workgroups per image, tiles) of the levels {grids}")
        assert sum(p < t for p, t in grids) >= 2                      # the walk runs in the model, in both programs
        for k, (a, b) in enumerate(zip(run(), base)):
            same = bool(np.array_equal(bits(a), bits(b)))
            print(f"[gdn-edges] (h) CDC_GDN_WGS={n}, tensor {k} {a.shape}: bit-equal to the default run: {same}")
            assert same
