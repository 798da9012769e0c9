"""What tests/test_gpu_gdn_edges.py leans on, asserted without a GPU: the input classes of tests/gdn_ref.py are what they claim to be,
every tolerance-tested result lies in the normal float32 range, a float32 restatement of the kernel's arithmetic meets the bound
(C + 2) 2^-24 against float64 on every class, and the workgroup rule (gdn_workgroups, cdc_op_gdn_workgroups) with CDC_GDN_WGS unset
is the expression gdn_launch held before."""
import numpy as np
import pytest

from cdc_compression_amd import _lib
from cdc_compression_amd.ops import Ops
from gdn_ref import (CLASSES, HOSTILE_SHAPE, WIDTHS, below_closed_form, bound, gdn_edge_case, gdn_f32_chain, gdn_f64, gdn_params,
                     nonfinite_agree, old_workgroups, perm_closed_form, perm_of, tolerance_cases, ulp_distance, with_nonfinite,
                     with_overflow, worst_fraction, zeros_agree)
from simple_ref import gdn_reparam_np


@pytest.mark.parametrize("C", WIDTHS)
def test_perm_gamma_reparametrises_to_exactly_zero_and_one(C):
    beta, gamma = gdn_params("perm", C)
    _, gr = gdn_reparam_np(beta, gamma)
    pi = perm_of(C)
    want = np.zeros((C, C), np.float32)
    want[np.arange(C), pi] = 1.0
    np.testing.assert_array_equal(gr.view(np.uint32), want.view(np.uint32))
    assert (pi != np.arange(C)).all()                                # no fixed point: an output never reads its own channel
    assert (pi[pi] != np.arange(C)).any()                            # not its own inverse: a transposed operand reads another channel
    assert (gr != gr.T).any()
    assert (len(set(pi.tolist())) == C) == (C % 3 != 0)              # a permutation unless 3 divides C (gdn_ref's docstring)


@pytest.mark.parametrize("C", (16, 48, 256))
def test_below_gamma_reparametrises_to_exactly_zero(C):
    beta, gamma = gdn_params("below", C)
    assert (gamma <= np.float32(2.0 ** -18)).all() and (gamma < 0).mean() > 0.3
    assert (gamma == np.float32(2.0 ** -18)).any() and ((gamma > 0) & (gamma < np.float32(2.0 ** -18))).any()
    _, gr = gdn_reparam_np(beta, gamma)
    assert (gr.view(np.uint32) == 0).all()                           # +0, every entry


@pytest.mark.parametrize("C", (16, 256))
def test_dense_gamma_is_dense_and_not_symmetric(C):
    beta, gamma = gdn_params("dense", C)
    br, gr = gdn_reparam_np(beta, gamma)
    assert gamma.min() >= 0 and gamma.max() < 0.3 and abs(float(gamma.mean()) - 0.15) < 0.02
    assert (gr > 0).mean() > 0.999 and (np.abs(gr - gr.T) > 1e-3).mean() > 0.5
    assert beta[0] == 0 and abs(float(br[0]) - 1e-6) < 1e-9
    assert np.array_equal(gdn_params("wide", C)[1], gamma)


def test_every_tolerance_tested_result_is_a_normal_float32():
    """Largest magnitude below 2^127 and smallest nonzero magnitude above 2^-126, forward and inverse, for every case of the GPU
    file: no overflow, and no subnormal result whose relative error the bound could not hold."""
    lo, hi = np.inf, 0.0
    for cls, B, C, HW in tolerance_cases():
        x, beta, gamma = gdn_edge_case(cls, B, C, HW)
        assert np.isfinite(x).all()
        for inverse in (False, True):
            a = np.abs(gdn_f64(x, beta, gamma, inverse))
            assert np.isfinite(a).all()
            nz = a[a != 0]
            lo, hi = min(lo, float(nz.min())), max(hi, float(nz.max()))
            assert nz.max() < 2.0 ** 127 and nz.min() > 2.0 ** -126, (cls, B, C, HW, inverse, float(nz.min()), float(nz.max()))
    print(f"[gdn-ref] float64 magnitudes over all cases: {lo:.3e} ... {hi:.3e}")
    assert hi > 1e25 and lo < 1e-25                                  # `wide` does reach far into both ends


@pytest.mark.parametrize("C", (16, 256))
@pytest.mark.parametrize("cls", CLASSES)
def test_float32_restatement_meets_the_bound(cls, C):
    x, beta, gamma = gdn_edge_case(cls, 2, C, 70)
    for inverse in (False, True):
        want = gdn_f64(x, beta, gamma, inverse)
        got = gdn_f32_chain(x, beta, gamma, inverse)
        f = worst_fraction(got, want, C)
        print(f"[gdn-ref] float32 chain, {cls} C={C}{' inv' if inverse else ''}: worst error {f:.3f} of (C + 2) 2^-24")
        assert f <= 1.0, f
        assert zeros_agree(got, want) and ((want == 0).any() or cls == "wide")      # (`wide` draws no zero)
        if cls == "perm":                                            # the closed forms are this chain's bits
            assert ulp_distance(got, perm_closed_form(x, beta, inverse)) == 0
        if cls == "below":
            assert ulp_distance(got, below_closed_form(x, beta, inverse)) == 0


def test_perm_moves_every_element_by_order_one_when_an_index_is_wrong():
    """The point of the class: evaluated with a transposed or a rotated gamma', (almost) every element misses the bound by orders of
    magnitude -- where the `normal` class moves by about 1e-3 relative.  (C = 64: where 3 divides C, rows 16 apart hold the same
    column, 3 * 16 = 0 mod 48, and a wave that took another wave's rows of gamma' would not show in this class at that width; every
    width runs, so the widths that 3 does not divide see it.)"""
    C = 64
    x, beta, gamma = gdn_edge_case("perm", 2, C, 70)
    want = gdn_f64(x, beta, gamma, False)
    for wrong in (gamma.T.copy(), np.roll(gamma, 4, axis=1), np.roll(gamma, 16, axis=0)):
        bad = gdn_f64(x, beta, wrong, False)
        m = want != 0
        rel = np.abs(bad[m] - want[m]) / np.abs(want[m])
        assert (rel > 1e3 * bound(C)).mean() > 0.95, float((rel > 1e3 * bound(C)).mean())


def test_hostile_inputs_are_what_the_gpu_tests_take_them_for():
    B, C, HW = HOSTILE_SHAPE
    x0, beta, gamma = gdn_edge_case("normal", B, C, HW)
    x, hostile = with_nonfinite(x0)
    assert hostile.sum() == 2 * C and HW % 64 == 6 and 66 >= 64      # one pixel in the whole tile, one in the tail
    for inverse in (False, True):
        want = gdn_f64(x, beta, gamma, inverse)
        assert np.isfinite(want[~hostile]).all() and np.isnan(want[hostile]).any()
        assert np.array_equal(want[~hostile], gdn_f64(x0, beta, gamma, inverse)[~hostile])      # float64 itself: own pixel only
        assert nonfinite_agree(want.astype(np.float32), want)
    assert np.isinf(gdn_f64(x, beta, gamma, True)[hostile]).any()    # x * inf
    assert (gdn_f64(x, beta, gamma, False)[hostile] == 0).any()      # x / inf: zeros whose sign the kernel must keep
    x0, beta, gamma = gdn_edge_case("dense", B, C, HW)
    x, hostile = with_overflow(x0)
    with np.errstate(over="ignore"):
        inv = gdn_f64(x, beta, gamma, True).astype(np.float32)
    assert np.isinf(inv[0, 5, 0, 3]) and np.isfinite(inv[~hostile]).all() and not np.isnan(inv).any()
    assert np.isfinite(inv[hostile]).any()                           # ... and finite where gamma' and the own value allow
    fwd = np.abs(gdn_f64(x, beta, gamma, False))
    assert fwd.max() < 2.0 ** 127 and fwd[fwd != 0].min() > 2.0 ** -126


def _cus():
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        pass
    return 256                                                       # the library's stand-in on a host without a device


def test_workgroup_rule_unset_is_the_former_expression_and_the_switch_caps_it(monkeypatch):
    assert "cdc_op_gdn_workgroups" in _lib.EXPORTS and hasattr(_lib.lib(), "cdc_op_gdn_workgroups")
    G, cus = Ops(0), _cus()
    monkeypatch.delenv("CDC_GDN_WGS", raising=False)
    shapes = [(B, HW) for B in (1, 2, 3, 4, 7, 32, 341, 342, 343, 1023, 1024, 1025, 5000)
              for HW in (1, 63, 64, 65, 128, 457, 2048, 128 * 128, 128 * 128 + 1, 512 * 512)]
    for B, HW in shapes:
        assert G.gdn_workgroups(B, HW) == old_workgroups(HW, B, cus), (B, HW)
    assert G.gdn_workgroups(32, 128 * 128) == (-(-4 * cus // 32), 256)          # the production case: 8 trips at 256 CUs
    for n in (1, 2, 3, 1000):
        monkeypatch.setenv("CDC_GDN_WGS", str(n))
        for B, HW in shapes:
            tiles = -(-HW // 64)
            assert G.gdn_workgroups(B, HW) == (min(tiles, n), tiles), (n, B, HW)
    for junk in ("0", "-3", "", "x"):                                 # n >= 1 or the rule as it is
        monkeypatch.setenv("CDC_GDN_WGS", junk)
        assert G.gdn_workgroups(3, 457) == old_workgroups(457, 3, cus)
    monkeypatch.delenv("CDC_GDN_WGS")
    L = _lib.lib()
    assert L.cdc_op_gdn_workgroups(G._h, 0, 64, None, None) == -1 and L.cdc_op_gdn_workgroups(G._h, 1, 0, None, None) == -1
    assert L.cdc_op_gdn_workgroups(G._h, 1, 64, None, None) == 0
