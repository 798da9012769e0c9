"""CPU checks of tests/rate_ref.py: the two references of the rate estimate against the reference's golden bpp and against each
other's owner, and the conditions on the inputs that tests/test_gpu_rate_edges.py relies on (a class must sit where its name says,
a tie must be an exact tie, the two roundings must differ on the tie set)."""
import json
import os

import numpy as np
import pytest

import rate_ref as R
from cdc_compression_amd import synth
from helpers import GOLDEN
from oracle import entropy as oe
from oracle import model as om


def _golden_prior_sd(meta):
    pman = [(k, tuple(v)) for k, v in meta["prior_manifest"]]
    psd = synth.unet_state_dict(pman, seed=11)
    return {k: ((v * 2.0).astype(np.float32) if ".weight" in k else v) for k, v in psd.items()}


@pytest.mark.parametrize("name", ["hyperdec_small_x", "hyperdec_full_x", "hyperdec_full_eps"])
def test_float32_method_reproduces_the_reference_bpp(name):
    """rate_terms_f32 is the reference's method: summed, it gives the real reference's bpp of the golden fixtures."""
    meta = json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    hr, cr = R.rate_terms_f32(_golden_prior_sd(meta), g["q_hyper_for_bpp"], g["q_latent_for_bpp"], g["mean"], g["scale"])
    H, W = (int(v) for v in g["img_hw"])
    b = (hr.sum(axis=(1, 2, 3)) + cr.sum(axis=(1, 2, 3))) / (H * W)
    assert b.shape == g["bpp"].shape
    assert np.abs(b - g["bpp"]).max() <= 1e-4 * max(1.0, float(np.abs(g["bpp"]).max())), (b, g["bpp"])


def test_float64_terms_are_those_of_compressor_bpp():
    sd = R.prior_sd()
    names, qh, ql, mu, sc = R.class_batch()
    hr, cr = R.rate_terms_f64(sd, qh, ql, mu, sc)
    assert hr.shape == qh.shape and cr.shape == ql.shape and hr.dtype == np.float64 and cr.dtype == np.float64
    want = om.compressor_bpp(sd, (64, 64), qh, ql, mu, sc)
    got = ((hr.sum(axis=(1, 2, 3)) + cr.sum(axis=(1, 2, 3))) / (64 * 64)).astype(np.float32)
    np.testing.assert_array_equal(got, want)


def test_classes_sit_where_their_names_say():
    """Share of elements the float64 reference prices at the 1e-9 floor: <= 10 % in every class but `floor` and `far`, >= 99 % there.
    A class on the floor says nothing about the chain before the clamp; the two that belong there say nothing else."""
    sd = R.prior_sd()
    for seed in (0, 1):
        for name in R.GAUSS_CLASSES:
            ql, mu, sc = R.gauss_class(name, seed)
            assert ql.shape == (R.CL, 4, 4) and ql.dtype == mu.dtype == sc.dtype == np.float32
            _, cr = R.rate_terms_f64(sd, R.hyper_class("centre", seed)[None], ql[None], mu[None], sc[None])
            share = R.floor_share(cr)
            print(f"gauss/{name} seed {seed}: {100 * share:.1f} % at the floor")
            assert share >= 0.99 if name == "floor" else share <= 0.10, (name, share)
            d = np.abs(ql.astype(np.float64) - mu.astype(np.float64))
            s = sc.astype(np.float64)
            assert sc.min() >= np.float32(0.1) and sc.max() <= 2048
            if name == "centre":
                assert np.all(d == 0) and sc.min() < 0.2 and sc.max() > 1000
            if name == "tail":
                assert np.all(d / s >= 4.0) and np.all(d / s <= 6.0)
            if name == "wide":
                assert sc.min() >= 256 and d.max() > 3000
            if name == "smin":
                assert np.all(sc == np.float32(0.1)) and set(np.unique(d)) == {0.0, 1.0}
        for name in R.HYPER_CLASSES:
            qh = R.hyper_class(name, seed)
            hr, _ = R.rate_terms_f64(sd, qh[None], *(a[None] for a in R.quiet_gauss()))
            share = R.floor_share(hr)
            print(f"hyper/{name} seed {seed}: {100 * share:.1f} % at the floor")
            assert share >= 0.99 if name == "far" else share <= 0.10, (name, share)
    # the quiet latent part really is quiet: the hyper-class images of the batch are priced by their hyper term
    _, cr = R.rate_terms_f64(sd, R.hyper_class("centre", 0)[None], *(a[None] for a in R.quiet_gauss()))
    assert cr.sum() < 0.01


def test_per_channel_priors_differ_strongly():
    """Test (b) of the GPU suite tells channels apart by what one symbol costs under their priors."""
    sd = R.prior_sd()
    x = (R.medians()[None, :, None, None] + np.float32(3.0)).astype(np.float32)
    hr = -np.log2(om.flexible_prior_likelihood(sd, x)).reshape(-1)
    assert np.ptp(hr) > 5.0 and np.abs(np.diff(hr)).mean() > 0.5, (np.ptp(hr), np.abs(np.diff(hr)).mean())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1027, 128 * 16])
def test_tie_builders_yield_exact_ties_of_both_parities_and_signs(n):
    off = R.tie_offsets(n)
    x, k = R.tie_set(off)
    d = x - off                                                  # float32, as the kernels subtract
    assert d.dtype == np.float32
    assert np.all(d - np.floor(d) == np.float32(0.5))            # 100 % exact ties
    if n >= 255:
        assert {int(v) & 1 for v in k} == {0, 1} and k.min() < 0 < k.max() and d.min() < 0 < d.max()
        differ = np.rint(d) != R.round_half_away(d)
        assert differ.mean() >= 0.25, differ.mean()                  # or no test on this set could tell the two roundings apart
        # every (offset, k) pair of the two grids occurs: 6 and 17 are coprime
        assert n < 102 or len({(float(o), int(v)) for o, v in zip(off, k)}) == R.MEAN_GRID.size * R.TIE_K.size
    # hyper ties: medians + k + 0.5
    med = R.medians(n)
    xh, kh = R.tie_set(med, start=5)
    dh = xh - med
    assert np.all(dh - np.floor(dh) == np.float32(0.5))


def test_edge_scale_sets_cover_every_edge_and_its_neighbours():
    e = oe.edges()
    assert e[0] == np.float32(0.1) and e.shape == (128,)
    sets = dict((n, (s, b)) for n, s, b in R.edge_scale_sets())
    assert set(sets) == {"edges", "above", "below", "beyond"}
    for name, (s, want) in sets.items():
        assert s.dtype == np.float32 and s.shape == (128,)
        clamped = np.maximum(s, np.float32(0.1))
        np.testing.assert_array_equal(R.spec_bins(clamped), want, err_msg=name)
    assert np.array_equal(sets["edges"][0], e)
    assert np.all(sets["above"][0] > e) and np.all(sets["below"][0] < e)
    assert np.all(sets["above"][0].view(np.int32) - e.view(np.int32) == 1) and np.all(e.view(np.int32) - sets["below"][0].view(np.int32) == 1)
    beyond = sets["beyond"][0]
    assert 4096.0 in beyond and beyond.min() < 0 and np.count_nonzero(beyond < np.float32(0.1)) >= 3
    # a strict comparison in place of "s <= e_i" moves all 128 edge scales but the last one bin up
    assert np.count_nonzero(np.minimum(np.searchsorted(e, e, side="right"), 127) != sets["edges"][1]) == 127
    for i in (0, 17, 64, 100, 127):
        assert R.spec_K(i) == oe.gauss_table(i)[0]
    assert R.spec_K(127) == R.spec_K(100) == 1023 and 2 < R.spec_K(17) < R.spec_K(64) < 1023 and R.spec_K(0) == 2     # the cap included
