"""Region-of-interest coding, the part that needs no GPU: the references of tests/price_map_ref.py against themselves (the band and the
share of undecided symbols of every op-level case tests/test_gpu_price_map.py runs, the consequences the header states for g = 1,
g = 0 and a growing mu, the cell mean), the argument rules of the Python surface, psnr_weighted's host composition, and the agreement
of include/cdc_hip.h and _lib.py on the new symbols."""
import os
import re

import numpy as np
import pytest

import cdc_compression_amd as cdc
import price_map_ref as PR
import rdo_ref as R
from cdc_compression_amd import _lib, compressor as C, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cdc_price_cells", "cdc_set_rdo_map", "cdc_op_rdo_quantize_map"]
SMALL = dict(dim=8, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3)


# ---- the reference against itself -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_,P", PR.CASES)
@pytest.mark.parametrize("n", [3, 1])
def test_band_and_undecided_share_of_the_op_cases(C_, P, n):
    """The cap is a condition the references alone must meet: at most 1 % of a case's symbols inside the band (10 x the float32
    method's own loss in eff dR - dD over the case's inputs), exact-zero prices counted as decided; and outside the band the float32
    restatement already equals the float64 decision."""
    y, m, s = PR.op_case(C_, P)
    g = PR.map_case(n, P)
    assert g.shape == (n, P) and np.all(g >= 0) and np.all(np.isfinite(g)) and g[0, -1] == (0.0 if P >= 5 else PR.FIXED[P - 1])
    eff = PR.effective(PR.MUS, g, C_)
    assert eff.shape == y.shape and eff.dtype == np.float32 and eff.max() <= 8.0 and not eff[0].any()
    band, worst = PR.method_band(y, m, s, eff)
    t = R.terms64(y, m, s)
    und = PR.undecided(t, eff, band)
    print(f"[price] (C, P) = ({C_}, {P}), n = {n}: float32 method off by {worst:.3g}, band {band:.3g}, undecided {int(und.sum())} of {und.size}")
    assert 0 < band < 0.05
    assert und.sum() <= R.UNDECIDED_CAP * und.size
    d32 = (t["k0"] != 0) & (PR.margin32(y, m, s, eff) > 0)
    assert not np.any((d32 != PR.decide64(t, eff)) & ~und)
    assert not PR.decide64(t, eff)[eff == 0].any()                     # a price of exactly 0 never moves


def test_the_consequences_the_header_states():
    y, m, s = PR.op_case(5, 259)
    t = R.terms64(y, m, s)
    # g = 1: the scalar rule (mu * 1.0f is exact)
    ones = PR.effective(R.MUS, np.ones((1, 259), np.float32), 5)
    for b, mu in enumerate(R.MUS):
        assert np.array_equal(ones[b], np.full((5, 259), mu, np.float32))
        assert np.array_equal(PR.decide64(t, ones)[b], R.decide64({k: v[b] for k, v in t.items()}, mu))
    # g = 0 never moves, whatever mu
    assert not PR.decide64(t, PR.effective([1e30] * 3, np.zeros((1, 259), np.float32), 5)).any()
    # monotone in mu for a fixed map: the float32 product of non-negatives is monotone
    g = PR.map_case(3, 259)
    prev = np.zeros(y.shape, bool)
    for mu in np.concatenate([[0.0], C.RDO_LADDER, [3e38]]).astype(np.float32):
        with np.errstate(over="ignore"):
            eff = PR.effective([mu] * 3, g, 5)
        with np.errstate(invalid="ignore"):
            mv = PR.decide64(t, eff)
        assert not np.any(prev & ~mv), mu
        prev = mv
    # the overflowed product behaves as the limit: it moves where dR > 0 and k0 != 0, and inf * 0 = NaN compares false
    assert np.isinf(eff).any()
    inf = np.isinf(eff)
    assert np.array_equal(mv[inf], ((t["k0"] != 0) & (t["dR"] > 0))[inf])


def test_the_cell_reference_on_a_window_inside_a_larger_frame():
    """100 x 150 in a 128 x 192 frame, 16-pixel cells: row 6 has 4 pixel rows inside and row 7 none, column 9 has 6 pixel columns inside
    and columns 10 and 11 none.  Dyadic values: every float64 sum is exact, so the mean is that of numpy in any order."""
    H, W, cell, gh, gw = 100, 150, 16, 8, 12
    pm = PR.dyadic_map(2, H, W, Hf=128, Wf=192)
    assert np.isnan(pm[:, H:, :]).all() and np.isnan(pm[:, :, W:]).all() and np.isin(pm[:, :H, :W], PR.DYADIC).all()
    cells = PR.cells_ref(pm, H, W, cell, gh, gw)
    assert cells.shape == (2, gh, gw) and cells.dtype == np.float32 and np.all(np.isfinite(cells))
    win = pm[:, :H, :W].astype(np.float64)
    assert cells[1, 2, 3] == np.float32(win[1, 32:48, 48:64].mean())
    assert cells[0, 6, 0] == np.float32(win[0, 96:100, 0:16].mean())                   # four rows inside
    assert cells[0, 0, 9] == np.float32(win[0, 0:16, 144:150].mean())                  # six columns inside
    assert cells[0, 6, 9] == np.float32(win[0, 96:100, 144:150].mean())
    assert np.array_equal(cells[:, 7], cells[:, 6])                                    # a row beyond the window: the nearest one inside
    assert np.array_equal(cells[:, :, 10], cells[:, :, 9]) and np.array_equal(cells[:, :, 11], cells[:, :, 9])
    one = PR.cells_ref(np.full((1, 1, 1), 0.25, np.float32), 1, 1, 16, 4, 4)           # a 1 x 1 window fills every cell
    assert np.array_equal(one, np.full((1, 4, 4), 0.25, np.float32))
    const = PR.cells_ref(np.full((1, 70, 33), 4.0, np.float32), 70, 33, 16, 5, 3)
    assert np.all(const == 4.0)


# ---- argument rules, checked before the library is touched ------------------------------------------------------------------------------

def _calls(comp, img, lat, hyp):
    return (lambda **k: comp.compress_to_bytes(img, **k), lambda **k: comp.encode(img, **k), lambda **k: comp.forward(img, **k),
            lambda **k: comp.latents_to_bytes(lat, hyp, **k))


def test_price_map_argument_rules():
    """On a model with no weights loaded: every refusal is the argument's own, raised before the library is touched."""
    comp = cdc.BigCompressor(**SMALL)
    B, H, W = 2, 100, 150
    img = np.zeros((B, 3, H, W), np.float32)
    lat, hyp = np.zeros((B, 32, 8, 12), np.float32), np.zeros((B, 32, 2, 3), np.float32)
    ok = np.ones((H, W), np.float32)
    for call in _calls(comp, img, lat, hyp)[:3]:
        for bad in (np.ones((H, W + 1), np.float32), np.ones((3, H, W), np.float32), np.ones((B, 2, H, W), np.float32), np.ones((H,), np.float32),
                    np.ones((H, W), np.float64), np.ones((H, W), np.int32)):
            with pytest.raises(ValueError, match="price_map"):
                call(rdo=1.0, price_map=bad)
        for v in (-0.5, np.nan, np.inf):
            bad = ok.copy()
            bad[40, 7] = v
            with pytest.raises(ValueError, match="finite and >= 0"):
                call(rdo=1.0, price_map=bad)
        with pytest.raises(ValueError, match="need one of rdo"):
            call(price_map=ok)
        with pytest.raises(ValueError, match="exclude each other"):
            call(rdo=1.0, price_map=ok, price_cells=np.ones((8, 12), np.float32))
    to_bytes = _calls(comp, img, lat, hyp)[3]                          # (its map is at the coded extent: 128 x 192)
    with pytest.raises(ValueError, match="price_map"):
        to_bytes(rdo=1.0, price_map=ok)
    with pytest.raises(ValueError, match="need one of rdo"):
        to_bytes(price_map=np.ones((128, 192), np.float32))
    with pytest.raises(ValueError, match="need one of rdo"):
        comp.compress_to_bytes(img, price_cells=np.ones((8, 12), np.float32))
    for bad in (np.ones((3, 8, 12), np.float32), np.ones((8,), np.float32), -np.ones((8, 12), np.float32), np.full((8, 12), np.nan, np.float32),
                np.ones((8, 12), np.float64)):
        with pytest.raises(ValueError, match="price_cells"):
            comp.compress_to_bytes(img, rdo=1.0, price_cells=bad)
    with pytest.raises(ValueError, match="price_map"):
        comp.rate_sweep(img, [0.0, 1.0], price_map=np.ones((H + 1, W), np.float32))
    with pytest.raises(ValueError, match="exclude each other"):
        comp.rdo_quantize(lat, lat, lat, 1.0, price_map=np.ones((128, 192), np.float32), price_cells=np.ones((8, 12), np.float32))
    with pytest.raises(ValueError):
        comp.rdo_quantize(lat, lat, lat, 1.0, price_cells=np.ones((1, 95), np.float32))
    # the accepted forms: [H, W], [1, H, W], [B, H, W], [B, 1, H, W]; bool is cast
    for shape in ((H, W), (1, H, W), (B, H, W), (B, 1, H, W)):
        v = C.price_map_values(np.ones(shape, bool), B, H, W)
        assert v.dtype == np.float32 and v.shape == ((B if shape[0] == B and len(shape) > 2 else 1), H, W) and np.all(v == 1)
    assert C.price_args(None, None, B, (H, W), False) is None
    assert C.price_cells_values(np.ones((8, 12), bool), B, (8, 12)).shape == (1, 8, 12)


def test_diffusion_checks_the_price_map_before_the_library_is_touched():
    kw = dict(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    diff = cdc.GaussianDiffusionEps(cdc.Unet(**kw), cdc.BigCompressor(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3),
                                    num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")
    img = np.zeros((2, 3, 32, 32), np.float32)
    ok = np.ones((32, 32), np.float32)
    for call in (lambda **k: diff.compress(img, sample_steps=2, sample_mode="ddim", **k), lambda **k: diff.compress_to_bytes(img, **k),
                 lambda **k: diff.compress_best_of(img, 2, seed=1, **k), lambda **k: diff.evaluate(img, sample_steps=2, sample_mode="ddim", **k)):
        with pytest.raises(ValueError, match="need one of rdo"):
            call(price_map=ok)
        with pytest.raises(ValueError, match="price_map"):
            call(rdo=1.0, price_map=np.ones((32, 31), np.float32))
        with pytest.raises(ValueError, match="finite and >= 0"):
            call(target_bpp=0.3, price_map=-ok)
        with pytest.raises(ValueError, match="exclude each other"):
            call(rdo=1.0, price_map=ok, price_cells=np.ones((2, 2), np.float32))


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    """What the C entry points refuse before they need a device: null handles, other handle kinds, n = 0 turning the map off."""
    L = _lib.lib()
    comp = cdc.BigCompressor(**SMALL)
    h = comp._hyper_handle()
    cells = np.ones((1, 4, 4), np.float32)
    assert L.cdc_set_rdo_map(h, None, 0, 0, 0, 0, None) == 0 and L.cdc_set_rdo_map(h, cells.ctypes.data, 0, 4, 4, 0, None) == 0
    assert L.cdc_set_rdo_map(h, None, 1, 4, 4, 0, None) == -1 and L.cdc_set_rdo_map(h, cells.ctypes.data, -1, 4, 4, 0, None) == -1
    assert L.cdc_set_rdo_map(h, cells.ctypes.data, 1, 0, 4, 0, None) == -1 and L.cdc_set_rdo_map(h, cells.ctypes.data, 1, 4, 4, 7, None) == -1
    assert L.cdc_set_rdo_map(None, cells.ctypes.data, 1, 4, 4, 0, None) == -1
    for other in (comp._handle(), comp._enc_handle()):
        assert L.cdc_set_rdo_map(other, cells.ctypes.data, 1, 4, 4, 0, None) == -2 and b"hyper decoder" in L.cdc_last_error(other)
    assert L.cdc_price_cells(None, cells.ctypes.data, 1, 1, 4, 4, 4, 4, 1, 4, 4, cells.ctypes.data, 0, None) == -1
    assert L.cdc_op_rdo_quantize_map(None, *[cells.ctypes.data] * 5, 1, cells.ctypes.data, None, 1, 1, 16, 0, None) == -1


# ---- psnr_weighted -------------------------------------------------------------------------------------------------------------------------

def test_psnr_weighted_with_equal_weights_is_the_unweighted_formula():
    rng = np.random.default_rng(4)
    B, gh, gw = 3, 8, 12
    count = np.full((B, gh, gw), 3 * 256, np.int32)
    count[:, 6] = 3 * 4 * 16
    count[:, 7] = 0
    count[:, :, 10:] = 0
    sse = rng.random((B, gh, gw)) * count * 0.01
    plain = 10.0 * np.log10(1.0 / (sse.reshape(B, -1).sum(1) / count.reshape(B, -1).sum(1)))
    for w in (np.ones((gh, gw)), np.full((1, gh, gw), 0.37), np.full((B, gh, gw), 4.0, np.float32)):
        assert np.allclose(metrics.weighted_psnr_of(sse, count, w), plain, rtol=1e-14, atol=0)
    # a region's own figure: weight 1 on the left half, 0 elsewhere
    w = np.zeros((gh, gw))
    w[:, :5] = 1
    left = 10.0 * np.log10(1.0 / (sse[:, :, :5].reshape(B, -1).sum(1) / count[:, :, :5].reshape(B, -1).sum(1)))
    assert np.allclose(metrics.weighted_psnr_of(sse, count, w), left, rtol=1e-14, atol=0)
    assert np.all(np.isposinf(metrics.weighted_psnr_of(np.zeros_like(sse), count, np.ones((gh, gw)))))
    for bad in (np.ones((gh, gw + 1)), np.ones((2, gh, gw)), -np.ones((gh, gw)), np.full((gh, gw), np.nan), np.zeros((gh, gw))):
        with pytest.raises(ValueError, match="cell_weights"):
            metrics.weighted_psnr_of(sse, count, bad)
    w = np.zeros((gh, gw))
    w[7] = 1                                                             # weight on cells beyond the window only
    with pytest.raises(ValueError, match="cell_weights"):
        metrics.weighted_psnr_of(sse, count, w)


# ---- header and binding ---------------------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "cdc_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert name in _lib.EXPORTS and hasattr(L, name)
        params = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
        assert len(params.split(",")) == len(getattr(L, name).argtypes), name
