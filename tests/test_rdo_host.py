"""Rate-distortion optimised quantisation, the part that needs no GPU: the argument rules of the Python surface and of cdc_set_rdo, the
float64 reference of tests/rdo_ref.py against itself (monotone moved set, dD as a difference of squares, mu = 0, the band and the share
of undecided symbols of every op-level case tests/test_gpu_rdo.py runs), and the ladder selection of compress_to_bytes(target_bpp=) on
hand-made sweep tables."""
import ctypes

import numpy as np
import pytest

import cdc_compression_amd as cdc
import rdo_ref as R
from cdc_compression_amd import _lib, compressor as C

SMALL = dict(dim=8, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3)


# ---- argument rules ----------------------------------------------------------------------------------------------------------------

def test_rdo_target_bpp_and_max_bytes_exclude_each_other():
    comp = cdc.BigCompressor(**SMALL)
    img = np.zeros((2, 3, 64, 64), np.float32)
    for kw in (dict(rdo=1.0, target_bpp=0.3), dict(rdo=1.0, max_bytes=500), dict(target_bpp=0.3, max_bytes=500),
               dict(rdo=0.0, target_bpp=0.3, max_bytes=500)):
        with pytest.raises(ValueError, match="exclude each other"):
            comp.compress_to_bytes(img, **kw)
        with pytest.raises(ValueError, match="exclude each other"):
            C.rdo_exclusive(**kw)
    C.rdo_exclusive()
    C.rdo_exclusive(rdo=0.0)
    C.rdo_exclusive(max_bytes=10)


@pytest.mark.parametrize("bad", [-1.0, [0.5, -0.0001], float("nan"), float("inf"), [1.0, float("-inf")]])
def test_negative_or_non_finite_mu_is_refused(bad):
    comp = cdc.BigCompressor(**SMALL)
    img = np.zeros((2, 3, 64, 64), np.float32)
    with pytest.raises(ValueError, match="finite and >= 0"):
        C.rdo_values(bad, 2)
    for call in (lambda: comp.compress_to_bytes(img, rdo=bad), lambda: comp.encode(img, rdo=bad), lambda: comp.forward(img, rdo=bad),
                 lambda: comp.rate_sweep(img, bad), lambda: comp.latents_to_bytes(np.zeros((2, 32, 4, 4), np.float32), np.zeros((2, 32, 1, 1), np.float32), rdo=bad)):
        with pytest.raises(ValueError):
            call()


def test_mu_vector_of_neither_1_nor_B_entries_is_refused():
    comp = cdc.BigCompressor(**SMALL)
    img = np.zeros((3, 3, 64, 64), np.float32)
    assert C.rdo_values(0.5, 3).tolist() == [0.5] and C.rdo_values([0, 1, 2], 3).dtype == np.float32
    for n in (2, 4):
        with pytest.raises(ValueError, match="1 or 3 expected"):
            comp.compress_to_bytes(img, rdo=np.ones(n, np.float32))
        with pytest.raises(ValueError, match="1 or 3 expected"):
            comp.encode(img, rdo=[1.0] * n)
        with pytest.raises(ValueError, match="1 or 3 expected"):
            comp.compress_to_bytes(img, target_bpp=[0.3] * n)
        with pytest.raises(ValueError, match="1 or 3 expected"):
            comp.compress_to_bytes(img, max_bytes=[300] * n)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            comp.compress_to_bytes(img, target_bpp=bad)


def test_ladders_of_0_or_more_than_32_values_are_refused():
    comp = cdc.BigCompressor(**SMALL)
    img = np.zeros((1, 3, 64, 64), np.float32)
    assert C.RDO_MAX_LADDER == 32 and C.RDO_LADDER.size == 17 and C.RDO_LADDER[0] == 2.0 ** -8 and C.RDO_LADDER[-1] == 2.0 ** 8
    for n in (0, 33, 64):
        with pytest.raises(ValueError, match="ladder"):
            comp.rate_sweep(img, np.ones(n, np.float32))
        with pytest.raises(ValueError, match="ladder"):
            C.rdo_values(np.ones(n, np.float32), None)
    assert C.rdo_values(np.ones(32), None).size == 32


def test_diffusion_checks_the_arguments_before_the_library_is_touched():
    """GaussianDiffusion.compress / compress_to_bytes / compress_best_of refuse the same combinations on models with no weights loaded:
    the refusal is the argument's, not a missing state dict's."""
    kw = dict(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    diff = cdc.GaussianDiffusionEps(cdc.Unet(**kw), cdc.BigCompressor(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3),
                                    num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")
    img = np.zeros((2, 3, 32, 32), np.float32)
    for call in (lambda **k: diff.compress(img, sample_steps=2, sample_mode="ddim", **k), lambda **k: diff.compress_to_bytes(img, **k),
                 lambda **k: diff.compress_best_of(img, 2, seed=1, **k)):
        with pytest.raises(ValueError, match="exclude each other"):
            call(rdo=1.0, target_bpp=0.2)
        with pytest.raises(ValueError, match="finite and >= 0"):
            call(rdo=-2.0)
        with pytest.raises(ValueError, match="1 or 2 expected"):
            call(rdo=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError):
            call(target_bpp=float("nan"))


def test_cdc_set_rdo_argument_rules():
    """The C entry point on handles that never touch a device: kinds, n, values; n = 0 turns it off with or without a pointer."""
    L = _lib.lib()
    assert all(s in _lib.EXPORTS and hasattr(L, s) for s in ("cdc_set_rdo", "cdc_entropy_rate_sweep", "cdc_op_rdo_quantize"))
    comp = cdc.BigCompressor(**SMALL)
    h = comp._hyper_handle()
    ok = np.array([0.0, 0.5, 8.0], np.float32)
    assert L.cdc_set_rdo(h, ok.ctypes.data, 3) == 0 and L.cdc_set_rdo(h, ok.ctypes.data, 1) == 0
    assert L.cdc_set_rdo(h, ok.ctypes.data, 0) == 0 and L.cdc_set_rdo(h, None, 0) == 0
    assert L.cdc_set_rdo(h, None, 1) == -1 and L.cdc_set_rdo(h, ok.ctypes.data, -1) == -1
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        a = np.array([0.5, bad, 1.0], np.float32)
        assert L.cdc_set_rdo(h, a.ctypes.data, 3) == -1 and b"mu[1]" in L.cdc_last_error(h)
        assert L.cdc_set_rdo(h, a.ctypes.data, 1) == 0                   # (only the first n values are read)
    assert L.cdc_set_rdo(h, None, 0) == 0
    assert L.cdc_set_rdo(None, ok.ctypes.data, 1) == -1
    for other in (comp._handle(), comp._enc_handle()):                   # a context decoder, an encoder: not the hyper decoder
        assert L.cdc_set_rdo(other, ok.ctypes.data, 1) == -2 and b"hyper decoder" in L.cdc_last_error(other)


# ---- the reference against itself -----------------------------------------------------------------------------------------------------

def _big_case():
    return R.op_case(R.PER_IMAGE[-1])


def test_reference_moved_set_is_monotone_in_mu():
    y, m, s = _big_case()
    t = R.terms64(y, m, s)
    ladder = np.concatenate([[0.0], C.RDO_LADDER, [1e6]]).astype(np.float32)
    prev = np.zeros(y.shape, bool)
    counts = []
    for mu in ladder:
        mv = R.decide64(t, mu)
        assert not np.any(prev & ~mv), mu                                # a symbol that moved at a smaller mu still moves
        prev = mv
        counts.append(int(mv.sum()))
    assert counts[0] == 0 and counts[-1] > counts[1] and counts == sorted(counts)
    assert not np.any(prev & (t["k0"] == 0))
    bits, sse, moved = R.sweep64(y[0], m[0], s[0], ladder)
    assert np.all(np.diff(bits) <= 0) and np.all(np.diff(sse) >= 0) and np.all(np.diff(moved) >= 0) and moved[0] == 0


def test_reference_dD_is_the_difference_of_squares():
    y, m, s = _big_case()
    t = R.terms64(y, m, s)
    d, k0, k1 = (t[k].astype(np.float64) for k in ("d", "k0", "k1"))
    nz = k0 != 0
    want = (d - k1) ** 2 - (d - k0) ** 2
    # (the squares round at 2^-52 d^2, their difference is of order 1: the bound carries d^2)
    assert np.all(np.abs(t["dD"][nz] - want[nz]) <= 8 * np.finfo(np.float64).eps * np.maximum(d[nz] ** 2, 1.0))
    assert np.all(t["dD"] >= 0) and np.all(t["dD"] <= 2)
    assert np.any(t["dD"] == 0) and np.any(t["dD"] == 2)                 # the +-1.5 and +-2.5 ties are in
    q, _ = R.quantise64(y, m, s, 1e6)
    assert np.max(np.abs(q.astype(np.float64) - y.astype(np.float64)) - 1.5) <= np.max(np.spacing(np.abs(y)))


def test_reference_mu_0_moves_nothing_and_the_clamp_moves_nothing():
    y, m, s = _big_case()
    t = R.terms64(y, m, s)
    assert not R.decide64(t, 0.0).any()
    q, mv = R.quantise64(y, m, s, 0.0)
    assert not mv.any() and np.array_equal(q, t["x0"])
    both = (t["bits0"] > 29.89) & (t["bits1"] > 29.89)
    assert both.sum() >= 6 and np.all(t["dR"][both] == 0) and not R.decide64(t, 1e30)[both].any()


@pytest.mark.parametrize("per_image", R.PER_IMAGE)
def test_band_and_undecided_share_of_the_op_cases(per_image):
    """The two figures the GPU cases rest on, from the references alone: the band (10 x the float32 method's own loss in mu dR - dD over
    the case's inputs) and the share of symbols inside it (at most 1 %).  The loss is dominated by the scale point 2048, where the
    float32 difference of two values near 0.5 cancels to a relative 3e-4: 1.8e-3 at mu = 8, so the band is 1.8e-2 wherever that point
    is in (every case but per_image = 1)."""
    y, m, s = R.op_case(per_image)
    assert y.shape == (3, per_image) and np.all(np.isfinite(y)) and s.min() >= np.float32(0.1)
    band, worst = R.method_band(y, m, s, R.MUS)
    t = R.terms64(y, m, s)
    und = sum(int(R.undecided({k: v[b] for k, v in t.items()}, mu, band).sum()) for b, mu in enumerate(R.MUS))
    print(f"[rdo] per_image {per_image}: float32 method off by {worst:.3g}, band {band:.3g}, undecided {und} of {3 * per_image}")
    assert 0 < band < 0.05
    assert und <= R.UNDECIDED_CAP * 3 * per_image
    if per_image >= 63:                                                 # every edge class is in every image
        for b in range(3):
            tb = {k: v[b] for k, v in t.items()}
            assert np.any(np.abs(tb["k0"]) == 1) and np.any(tb["k0"] == 0) and np.any((tb["bits0"] > 29.89) & (tb["bits1"] > 29.89))
            assert np.any(np.abs(m[b]) >= 1e4) and np.any(s[b] == 2048) and np.any(s[b] == np.float32(0.1))
            assert np.any(tb["dD"] == 2) and (b == 0 or np.any(tb["dD"] == 0))


# ---- ladder selection -------------------------------------------------------------------------------------------------------------------

LADDER = np.concatenate([np.zeros(1, np.float32), C.RDO_LADDER])


def test_select_takes_the_smallest_mu_that_meets_the_target():
    cost = np.linspace(1.0, 0.1, LADDER.size)                            # non-increasing, as a sweep's row
    for j in (1, 5, 17):
        target = 0.5 * (cost[j] + cost[j - 1])
        assert C.rdo_select(cost, target) == (j, True)
        assert C.rdo_select(cost, cost[j]) == (j, True)                  # (<=: an entry that equals the target meets it)
    flat = np.array([3.0, 2.0, 2.0, 2.0, 1.0])
    assert C.rdo_select(flat, 2.0) == (1, True)                          # the first of equal entries: the smallest mu


def test_select_gives_mu_0_when_the_target_is_already_met():
    cost = np.linspace(1.0, 0.1, LADDER.size)
    assert C.rdo_select(cost, 1.0) == (0, True) and C.rdo_select(cost, 7.0) == (0, True)
    assert LADDER[0] == 0.0


def test_select_reports_met_false_past_the_end_of_the_ladder():
    cost = np.linspace(1.0, 0.1, LADDER.size)
    assert C.rdo_select(cost, 0.0999) == (LADDER.size - 1, False)
    assert C.rdo_select([5.0], 1.0) == (0, False)


def test_refinement_interval():
    """Between the entry found and the one below it: 17 float32 values, ascending, both ends exact; linear above mu = 0."""
    for j in (2, 9, 17):
        lo, hi = LADDER[j - 1], LADDER[j]
        r = C.rdo_refine_ladder(lo, hi)
        assert r.dtype == np.float32 and r.size == 17 and r[0] == lo and r[-1] == hi and np.all(np.diff(r) > 0)
        assert np.allclose(r[1:] / r[:-1], 2.0 ** (1 / 16), rtol=1e-6)
    r = C.rdo_refine_ladder(LADDER[0], LADDER[1])
    assert r[0] == 0 and r[-1] == LADDER[1] and r.size == 17 and np.allclose(np.diff(r), LADDER[1] / 16, rtol=1e-6)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            C.rdo_refine_ladder(lo, hi)
    # two selections in a row, as compress_to_bytes runs them: the refined mu lies in (lo, hi] and meets the target
    cost = np.linspace(1.0, 0.1, LADDER.size)
    j, met = C.rdo_select(cost, 0.52)
    r = C.rdo_refine_ladder(LADDER[j - 1], LADDER[j])
    fine = np.linspace(cost[j - 1], cost[j], r.size)
    k, met2 = C.rdo_select(fine, 0.52)
    assert met and met2 and 0 < k <= 16 and fine[k] <= 0.52 < fine[k - 1] and LADDER[j - 1] < r[k] <= LADDER[j]
