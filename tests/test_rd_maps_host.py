"""Rate and error maps, the part that needs no GPU: the input conditions tests/test_gpu_rd_maps.py relies on (tests/rd_maps_ref.py),
the Python argument rules, which raise before the library is touched, and rate_map_cell of the three compressor classes."""
import numpy as np
import pytest

import cdc_compression_amd as cdc
import metrics_ref as M
import rate_ref as R
import rd_maps_ref as D
from cdc_compression_amd import _lib, metrics
from cdc_compression_amd.compressor import SimpleCompressor


def test_typical_case_keeps_off_the_likelihood_floor():
    """(c): fewer than 5 % of the symbols sit on the 1e-9 floor, where an error of the chain is clamped away."""
    (qh, ql, mu, sc), ref, own, (h64, c64) = D.typical_case()
    assert ql.shape == (D.TYPICAL_B, R.CL, 20, 16) and qh.shape == (D.TYPICAL_B, R.CH, 5, 4)
    share = R.floor_share(np.concatenate([h64.ravel(), c64.ravel()]))
    print(f"[rd-maps] typical case: {100 * share:.2f} % of the symbols on the floor")
    assert share < 0.05
    assert R.floor_share(h64) < 0.05 and R.floor_share(c64) < 0.05
    for b in range(1, D.TYPICAL_B):                                   # distinct images: a row mix-up shows
        assert not np.array_equal(ql[b], ql[0]) and not np.array_equal(qh[b], qh[0])


def test_moved_symbols_cost_bits_and_stay_off_the_floor():
    """(b): every moved symbol costs at least 1 bit more than on the baseline and stays below FLOOR_BITS, and nothing else moves."""
    (qh, ql, mu, sc), ref, own, (h64, c64) = D.geometry_case()
    for i, ((y, x), c) in enumerate(D.LATENT_MOVES, 1):
        moved, base = c64[i, c, y, x], c64[0, c, y, x]
        assert moved - base >= 1.0 and moved < R.FLOOR_BITS, (i, moved, base)
        d = c64[i] - c64[0]
        d[c, y, x] = 0.0
        assert not d.any() and np.array_equal(h64[i], h64[0])
    for j, ((y, x), c) in enumerate(D.HYPER_MOVES, 1 + len(D.LATENT_MOVES)):
        moved, base = h64[j, c, y, x], h64[0, c, y, x]
        assert moved - base >= 1.0 and moved < R.FLOOR_BITS, (j, moved, base)
        d = h64[j] - h64[0]
        d[c, y, x] = 0.0
        assert not d.any() and np.array_equal(c64[j], c64[0])
    # the move stands out of the entry it falls into by far more than the entry's tolerance
    tol = D.tolerance(ref["cell"], own["cell"])
    assert float(tol.max()) < 1e-2


def test_reference_sums_agree_with_each_other():
    """The five sums of rd_maps_ref.sums are sums of the same terms: cell, and both profiles, add up to the image's bits."""
    names, _, ref, own, (h64, c64) = D.class_case()
    total = h64.sum(axis=(1, 2, 3)) + c64.sum(axis=(1, 2, 3))
    np.testing.assert_allclose(ref["cell"].sum(axis=(1, 2)), total, rtol=1e-12)
    np.testing.assert_allclose(ref["latent_channels"].sum(axis=1) + ref["hyper_channels"].sum(axis=1), total, rtol=1e-12)
    assert ref["latent"].shape == (9, 4, 4) and ref["hyper"].shape == (9, 1, 1) and ref["hyper_channels"].shape == (9, R.CH)


def test_cell_sums_reference():
    v = np.ones((2, 3, 70, 100), np.int64)
    s, n = D.cell_sums(v, 16, 8, 8)
    assert n[0, 0, 0] == 3 * 256 and n[0, 4, 0] == 3 * 6 * 16 and n[0, 0, 6] == 3 * 16 * 4 and n[0, 4, 6] == 3 * 6 * 4
    assert not n[:, 5:].any() and not n[:, :, 7:].any() and np.array_equal(s, n) and n.sum() == 2 * 3 * 70 * 100


def test_as_saved_floats_of_the_byte_case_give_the_bytes_back():
    """(g): the float32 operand v / 255 * 2 - 1 is saved as the byte v, so its as_saved map has the uint8 operands' bits."""
    u = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    f = (u.astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    assert np.array_equal(M.saved_u8(f), u)


# ---- the Python argument rules raise before the library is touched ----------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_rate_map_refuses_an_unknown_name_before_the_library(no_library):
    m = cdc.ResnetCompressor(**R.MODEL_KW)
    z = np.zeros((1, R.CH, 1, 1), np.float32)
    l = np.zeros((1, R.CL, 4, 4), np.float32)
    for what in (("cell", "bits"), "total", (), ("latent", None)):
        with pytest.raises(ValueError):
            m.rate_map(z, l, l, l, what=what)


def test_sse_map_argument_rules_raise_before_the_library(no_library):
    a = np.zeros((2, 3, 70, 100), np.float32)
    u = np.zeros((2, 3, 70, 100), np.uint8)
    model = object()
    for kw in (dict(cell=0), dict(cell=-4), dict(cell=2.5), dict(cell=True),
               dict(cell=16, grid=(4, 7)), dict(cell=16, grid=(5, 6)), dict(cell=16, grid=(0, 7)),      # does not cover 70 x 100
               dict(cell=16, size=(71, 100)), dict(cell=16, size=(0, 5)), dict(cell=16, as_saved=(True,))):
        with pytest.raises(ValueError):
            metrics.sse_map(model, a, u, **kw)
    with pytest.raises(ValueError):
        metrics.sse_map(model, a.astype(np.float64), u, 16)
    with pytest.raises(ValueError):
        metrics.sse_map(model, a[:1], u, 16)
    assert metrics._check_grid(70, 100, 16, None) == (16, 5, 7) and metrics._check_grid(70, 100, 16, (8, 8)) == (16, 8, 8)
    assert metrics._check_grid(3, 5, 1, None) == (1, 3, 5) and metrics._check_grid(3, 5, 1000, None) == (1000, 1, 1)


def test_rate_map_cell_is_the_frame_multiple_over_the_upsampling():
    models = [cdc.ResnetCompressor(**R.MODEL_KW), cdc.ResnetCompressor(dim=8), cdc.BigCompressor(dim=8), cdc.BigCompressor(dim=8, vbr=True),
              SimpleCompressor(dim=16), cdc.BigCompressor(dim=8, dim_mults=(1, 2, 3), hyper_dims_mults=(3, 3))]
    for m in models:
        U = 2 ** (len(m.reversed_hyper_dims) - 2)
        assert m.hyper_upsampling == U and m.rate_map_cell * U == m.frame_multiple
    assert [m.rate_map_cell for m in models] == [16, 16, 16, 16, 16, 8]
    assert models[-1].hyper_upsampling == 2 and models[0].hyper_upsampling == 4


def test_header_and_python_mirror_agree_on_the_new_symbols():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cdc_hip.h")).read()
    for name in ("cdc_rate_map", "cdc_distortion_map"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in _lib.EXPORTS
