"""Region-of-interest coding on the GPU: cdc_op_rdo_quantize_map against the float64 decision of tests/price_map_ref.py, cdc_price_cells
against the float64 cell mean bit for bit, cdc_entropy_rate_sweep under cdc_set_rdo_map against the coder itself and against float64
sums, the streams of compress_to_bytes(price_map=), and GaussianDiffusion.compress_to_bytes / evaluate with a map.

The model, the images and their analysed latents are those of tests/test_gpu_rdo.py (the small four-level BigCompressor: frame multiple
64, 32 latent channels, 16-pixel cells; a 64 x 64 image has 4 x 4 latent positions, a 128 x 192 one 8 x 12), computed once and shared.
tests/test_price_map_host.py asserts on the CPU what the op-level cases rest on: the band and the share of undecided symbols."""
import ctypes
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
import metrics_ref as M
import price_map_ref as PR
import rate_ref as RR
import rdo_ref as R
import test_gpu_rdo as TR
from cdc_compression_amd import _lib, compressor as C, metrics, synth

pytestmark = pytest.mark.gpu

_bits32, _dev, _model, _images, _analysed = TR._bits32, TR._dev, TR._model, TR._images, TR._analysed


# ---- op level ---------------------------------------------------------------------------------------------------------------------------

def _check_op(case, q, moved, y, m, s, g):
    C_ = y.shape[1]
    eff = PR.effective(PR.MUS, g, C_)
    band, worst = PR.method_band(y, m, s, eff)
    t = R.terms64(y, m, s)
    is0, is1 = _bits32(q) == _bits32(t["x0"]), _bits32(q) == _bits32(t["x1"])
    assert np.all(is0 | is1), case                                       # every output symbol is k0 or k1
    took1 = ~is0
    assert not took1[0].any()                                            # mu = 0
    assert not np.any(took1 & (t["k0"] == 0)) and not np.any(took1 & (eff == 0))      # k0 = 0 cannot move, a price of 0 never moves
    assert np.array_equal(moved, took1.reshape(3, -1).sum(1)), (case, moved)            # the counts are exact
    want = PR.decide64(t, eff)
    und = PR.undecided(t, eff, band)
    differ = took1 != want
    off = np.abs(PR.margin64(t, eff))[differ]
    print(f"[price] (C, P) = {case}, map rows {g.shape[0]}: moved {moved.tolist()}, undecided {int(und.sum())}, differing from float64 "
          f"{int(differ.sum())} (largest float64 margin among them {off.max() if off.size else 0.0:.3g}), band {band:.3g} = 10 x {worst:.3g}")
    assert not np.any(differ & ~und), (case, np.argwhere(differ & ~und)[:5])
    assert und.sum() <= R.UNDECIDED_CAP * und.size


@pytest.mark.parametrize("C_,P", PR.CASES)
def test_op_against_the_float64_decision(C_, P):
    """cdc_op_rdo_quantize_map, B = 3 with mu = (0, 0.5, 2) and one map row per image (log-uniform in [1/8, 4] with 1, 0.25, 4, 0.125, 0
    at the last positions), from host and from device memory (the same bits); then n = 1 against n = B with the row repeated.
    The band is 10 x the float32 method's own loss in fl32(mu g) dR - dD, measured on the CPU over the case's inputs; a symbol whose
    effective price is exactly 0 is decided.  P = 1, 5, 37 and 259 are no multiples of 4 (the map is read as scalars whose position
    wraps inside a float4 of the latent), 16 and 96 are (float4 loads of the map)."""
    comp, _ = _model()
    y, m, s = PR.op_case(C_, P)
    g = PR.map_case(3, P)
    q, moved = comp.rdo_quantize(y, m, s, PR.MUS, price_cells=g)
    assert q.shape == y.shape and q.dtype == np.float32 and moved.dtype == np.int64 and moved.shape == (3,)
    _check_op((C_, P), q, moved, y, m, s, g)
    qd, moved_d = comp.rdo_quantize(_dev(y), _dev(m), _dev(s), PR.MUS, price_cells=_dev(g))
    assert np.array_equal(_bits32(qd.cpu().numpy()), _bits32(q)) and np.array_equal(moved_d, moved)
    g1 = PR.map_case(1, P)
    q1, moved_1 = comp.rdo_quantize(y, m, s, PR.MUS, price_cells=g1)
    _check_op((C_, P), q1, moved_1, y, m, s, g1)
    qB, moved_B = comp.rdo_quantize(y, m, s, PR.MUS, price_cells=np.repeat(g1, 3, axis=0))
    assert np.array_equal(_bits32(qB), _bits32(q1)) and np.array_equal(moved_B, moved_1)
    one, moved_one = comp.rdo_quantize(y[2:3], m[2:3], s[2:3], PR.MUS[2], price_cells=g[2:3])        # batch 1: image 2's row
    assert np.array_equal(_bits32(one[0]), _bits32(q[2])) and moved_one[0] == moved[2]


def _off_by_one(a):
    """A device copy of `a` whose base is 4 bytes past a 16-byte boundary."""
    import torch
    a = np.array(a, np.float32)
    pad = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
    v = pad[1:].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("C_,P", [(32, 96), (5, 259)])
def test_op_off_the_float4_alignment(C_, P):
    """Operands whose base is not 16-byte aligned take the scalar path for every element; a map whose base is not takes the scalar map
    loads under float4 loads of the latent.  Both give the symbols of the aligned call."""
    comp, _ = _model()
    y, m, s = PR.op_case(C_, P)
    g = PR.map_case(3, P)
    q, moved = comp.rdo_quantize(_dev(y), _dev(m), _dev(s), PR.MUS, price_cells=_dev(g))
    q2, moved2 = comp.rdo_quantize(_off_by_one(y), _off_by_one(m), _off_by_one(s), PR.MUS, price_cells=_dev(g))
    assert np.array_equal(_bits32(q2.cpu().numpy()), _bits32(q.cpu().numpy())) and np.array_equal(moved2, moved)
    q3, moved3 = comp.rdo_quantize(_dev(y), _dev(m), _dev(s), PR.MUS, price_cells=_off_by_one(g))
    assert np.array_equal(_bits32(q3.cpu().numpy()), _bits32(q.cpu().numpy())) and np.array_equal(moved3, moved)


@pytest.mark.parametrize("C_,P", [(5, 259), (32, 96)])
def test_op_identities(C_, P):
    """Bit for bit: an all-ones map is rdo_quantize without a map; a constant map of 0.5 with mu is the scalar 0.5 mu (exact products);
    positions with g = 0 keep k0."""
    comp, _ = _model()
    y, m, s = PR.op_case(C_, P)
    mus = np.array([0.25, 0.5, 8.0], np.float32)
    plain, moved0 = comp.rdo_quantize(y, m, s, mus)
    assert moved0[2] > 0
    for n in (1, 3):
        q, moved = comp.rdo_quantize(y, m, s, mus, price_cells=np.ones((n, P), np.float32))
        assert np.array_equal(_bits32(q), _bits32(plain)) and np.array_equal(moved, moved0)
    half, moved_h = comp.rdo_quantize(y, m, s, mus, price_cells=np.full((1, P), 0.5, np.float32))
    want, moved_w = comp.rdo_quantize(y, m, s, 0.5 * mus)
    assert np.array_equal(_bits32(half), _bits32(want)) and np.array_equal(moved_h, moved_w)
    g = np.ones((3, P), np.float32)
    g[:, ::3] = 0.0
    q, moved = comp.rdo_quantize(y, m, s, mus, price_cells=g)
    x0 = R.terms64(y, m, s)["x0"]
    assert np.array_equal(_bits32(q[:, :, ::3]), _bits32(x0[:, :, ::3]))
    keep = np.ones(P, bool)
    keep[::3] = False
    assert np.array_equal(_bits32(q[:, :, keep]), _bits32(plain[:, :, keep]))
    assert np.array_equal(moved, (_bits32(q) != _bits32(x0)).reshape(3, -1).sum(1)) and np.all(moved <= moved0) and moved[2] < moved0[2]
    # a bool mask is a map of 0 and 1
    qb, _ = comp.rdo_quantize(y, m, s, mus, price_cells=g.astype(bool))
    assert np.array_equal(_bits32(qb), _bits32(q))


def test_op_refusals_with_nothing_written():
    comp, _ = _model()
    L, h = _lib.lib(), comp._hyper_handle()
    C_, P = 7, 37
    y, m, s = (np.array(a) for a in PR.op_case(C_, P))
    g = PR.map_case(3, P)
    q = np.full(y.shape, -77.0, np.float32)
    moved = np.full(3, -5, np.int64)

    def call(ops, gm, n=3, mu=PR.MUS):
        return L.cdc_op_rdo_quantize_map(h, ops[0].ctypes.data, ops[1].ctypes.data, ops[2].ctypes.data, mu.ctypes.data, gm.ctypes.data, n,
                                         q.ctypes.data, moved.ctypes.data, 3, C_, P, 0, None)
    for bad in (np.nan, np.inf):
        for which in range(3):
            ops = [y.copy(), m.copy(), s.copy()]
            ops[which][1, 3, 20] = bad
            assert call(ops, g) == -1 and b"nothing written" in L.cdc_last_error(h), (which, bad)
            assert np.all(q == -77.0) and np.all(moved == -5)
    for bad in (-0.25, np.nan, np.inf, -np.inf):
        gm = g.copy()
        gm[2, 11] = bad
        assert call([y, m, s], gm) == -1 and b"map value (nothing written)" in L.cdc_last_error(h), bad
        assert np.all(q == -77.0) and np.all(moved == -5)
        with pytest.raises(_lib.CdcError, match="nothing written"):          # a device map reaches the library's check kernel
            comp.rdo_quantize(_dev(y), _dev(m), _dev(s), PR.MUS, price_cells=_dev(gm))
        with pytest.raises(ValueError):                                       # a host map is refused by the mirror
            comp.rdo_quantize(y, m, s, PR.MUS, price_cells=gm)
    assert call([y, m, s], g, n=2) == -1 and b"1 or 3 expected" in L.cdc_last_error(h)
    assert call([y, m, s], g, mu=np.array([0.0, -1.0, 1.0], np.float32)) == -1
    assert np.all(q == -77.0)
    assert call([y, m, s], g) == 0 and np.all(np.isfinite(q)) and np.all(moved >= 0)          # the handle still works


# ---- cdc_price_cells ----------------------------------------------------------------------------------------------------------------------

def _cells(comp, pm, n, H, W, cell, gh, gw, device=False, B=None):
    """cdc_price_cells on a map [n, Hf, Wf] of which the H x W window counts -> (rc, cells)."""
    L, h = _lib.lib(), comp._hyper_handle()
    Hf, Wf = pm.shape[1:]
    if device:
        import torch
        src, out = _dev(pm), torch.full((n, gh, gw), -3.0, dtype=torch.float32, device="cuda")
        rc = L.cdc_price_cells(h, src.data_ptr(), n, B or n, H, W, Hf, Wf, cell, gh, gw, out.data_ptr(), 1, C._current_stream(1))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()
    src, out = np.ascontiguousarray(pm, np.float32), np.full((n, gh, gw), -3.0, np.float32)
    return L.cdc_price_cells(h, src.ctypes.data, n, B or n, H, W, Hf, Wf, cell, gh, gw, out.ctypes.data, 0, None), out


@pytest.mark.parametrize("n,H,W,Hf,Wf,gh,gw", [
    (1, 64, 64, 64, 64, 4, 4),             # every cell full
    (3, 64, 64, 64, 64, 4, 4),
    (2, 100, 150, 128, 192, 8, 12),        # row 6: 4 pixel rows inside, row 7 none; column 9: 6 pixel columns inside, 10 and 11 none; Wf > W
    (1, 100, 150, 100, 150, 12, 16),       # a grid larger than the context model's own frame (a U-Net that asks for 192 x 256)
    (2, 1, 1, 5, 7, 4, 4),                 # a 1 x 1 window
    (1, 33, 17, 40, 17, 3, 2)])
def test_price_cells_against_the_float64_mean(n, H, W, Hf, Wf, gh, gw):
    """Dyadic pixel values: every float64 sum is exact in any order, so the cells are compared bit for bit.  Everything outside the window
    is NaN: one read there would poison a cell (and raise the kernel's flag)."""
    comp, _ = _model()
    pm = PR.dyadic_map(n, H, W, seed=7, Hf=Hf, Wf=Wf)
    want = PR.cells_ref(pm, H, W, 16, gh, gw)
    for device in (False, True):
        rc, got = _cells(comp, pm, n, H, W, 16, gh, gw, device, B=3 if n == 1 else n)
        assert rc == 0, _lib.lib().cdc_last_error(comp._hyper_handle())
        assert np.array_equal(_bits32(got), _bits32(want)), (device, np.argwhere(_bits32(got) != _bits32(want))[:5])
    if (Hf, Wf) == (H, W):                 # the mirror: the grid `rate_map` uses for the image (or that of padded_hw)
        padded = None if (gh, gw) == tuple(d // 16 for d in comp.padded_size(H, W)) else (gh * 16, gw * 16)
        assert np.array_equal(_bits32(comp.price_cells(pm, (H, W), padded)), _bits32(want))
        assert np.array_equal(_bits32(comp.price_cells(_dev(pm), (H, W), padded)), _bits32(want))


def test_price_cells_refusals():
    comp, _ = _model()
    L, h = _lib.lib(), comp._hyper_handle()
    H, W = 100, 150
    pm = PR.dyadic_map(2, H, W, seed=2, poison=0.0)
    for bad in (-1.0, np.nan, np.inf):
        for at in ((0, 0, 0), (1, 99, 149), (1, 97, 20)):
            p = pm.copy()
            p[at] = bad
            for device in (False, True):
                rc, got = _cells(comp, p, 2, H, W, 16, 8, 12, device)
                assert rc == -1 and b"nothing written" in L.cdc_last_error(h), (bad, at, device)
                assert np.all(got == -3.0)
    assert _cells(comp, pm, 2, H, W, 16, 8, 12)[0] == 0                                    # the handle still works
    for kw, text in ((dict(gh=6), b"does not cover"), (dict(gw=9), b"does not cover"), (dict(cell=0), b"cell"), (dict(H=0), b">= 1"),
                     (dict(B=3), b"1 or 3 expected")):
        a = dict(n=2, H=H, W=W, cell=16, gh=8, gw=12)
        a.update(kw)
        assert _cells(comp, pm, **a)[0] == -1 and text in L.cdc_last_error(h), kw
    out = np.zeros((2, 8, 12), np.float32)
    assert L.cdc_price_cells(h, pm.ctypes.data, 2, 2, H, W, H - 1, W, 16, 8, 12, out.ctypes.data, 0, None) == -1
    assert L.cdc_price_cells(h, None, 2, 2, H, W, H, W, 16, 8, 12, out.ctypes.data, 0, None) == -1
    assert L.cdc_price_cells(h, pm.ctypes.data, 2, 2, H, W, H, W, 16, 8, 12, None, 0, None) == -1
    for other in (comp._handle(), comp._enc_handle()):                                     # any handle kind
        assert L.cdc_price_cells(other, pm.ctypes.data, 2, 2, H, W, H, W, 16, 8, 12, out.ctypes.data, 0, None) == 0


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------

LADDERS = {1: np.array([2.0], np.float32),
           18: np.concatenate([np.zeros(1, np.float32), C.RDO_LADDER]),              # what compress_to_bytes(target_bpp=) sweeps
           32: np.concatenate([np.zeros(1, np.float32), np.geomspace(2.0 ** -8, 2.0 ** 8, 31).astype(np.float32)])}


def _two_valued(n, gh, gw):
    """Cells of 0.25 and 4, the border at another column in every row of the batch."""
    cells = np.full((n, gh, gw), 0.25, np.float32)
    for b in range(n):
        cells[b, :, (gw // 2 + b) % gw:] = 4.0
        cells[b, b % gh, 0] = 4.0
    return cells


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 64, 64), (1, 128, 192), (3, 128, 192)])
@pytest.mark.parametrize("L", [1, 18, 32])
def test_sweep_under_a_map_against_the_coder_and_float64(B, H, W, L):
    comp, psd = _model()
    latent, hyper, streams0, q0, qh, mean, scale = _analysed(B, H, W)
    gh, gw = latent.shape[2:]
    mus = LADDERS[L]
    # an all-ones map, broadcast or per image: the sweep without a map, bit for bit
    plain = comp._sweep(latent, hyper, mus)
    for n in sorted({1, B}):
        ones = comp._sweep(latent, hyper, mus, cells=np.ones((n, gh, gw), np.float32))
        assert all(np.array_equal(ones[k].view(np.int64), plain[k].view(np.int64)) for k in plain), n
    cells = _two_valued(B, gh, gw)
    t = comp._sweep(latent, hyper, mus, cells=cells)
    bits, sse, moved = t["bits"], t["sse"], t["moved"]
    assert bits.shape == sse.shape == moved.shape == (B, L) and moved.dtype == np.int64
    # monotone along the ladder, exactly
    assert np.all(np.diff(bits, axis=1) <= 0) and np.all(np.diff(moved, axis=1) >= 0) and np.all(np.diff(sse, axis=1) >= 0)
    # every entry against an encode at that mu under the map, decoded: the same count, and the float64 price of those symbols
    for j, mu in enumerate(mus):
        qj = comp.decompress_from_bytes(comp.latents_to_bytes(latent, hyper, rdo=float(mu), price_cells=cells))
        changed = (_bits32(qj) != _bits32(q0)).reshape(B, -1).sum(1)
        assert np.array_equal(changed, moved[:, j]), (j, mu, changed, moved[:, j])
        h64, c64 = RR.rate_terms_f64(psd, qh, qj, mean, scale)
        h32, c32 = RR.rate_terms_f32(psd, qh, qj, mean, scale)
        for b in range(B):
            ref = float(h64[b].sum() + c64[b].sum())
            own = float(np.abs(h32[b] - h64[b]).sum() + np.abs(c32[b] - c64[b]).sum())
            tol = 8.0 * own + 4.0 * float(np.spacing(np.float32(ref)))             # the bound of tests/test_gpu_rate_edges.py
            assert abs(bits[b, j] - ref) <= tol, (b, j, bits[b, j], ref, tol)
            sse_j = float(((latent[b].astype(np.float64) - qj[b].astype(np.float64)) ** 2).sum())
            assert np.isclose(sse[b, j], sse_j, rtol=1e-12, atol=0)
    assert L == 1 or moved[:, -1].all()
    print(f"[price] sweep {B} x {H} x {W}, L = {L}: bits {bits[0, 0]:.1f} -> {bits[0, -1]:.1f}, moved {moved[0, -1]} of {latent[0].size} "
          f"(without a map {plain['moved'][0, -1]})")
    # batch rows equal batch-1 rows under the image's own map row; device operands give the same bits
    if B > 1:
        for b in range(B):
            one = comp._sweep(latent[b:b + 1], hyper[b:b + 1], mus, cells=cells[b:b + 1])
            assert all(np.array_equal(one[k][0].view(np.int64), t[k][b].view(np.int64)) for k in t), b
        dev = comp._sweep(_dev(latent), _dev(hyper), mus, cells=cells)
        assert all(np.array_equal(dev[k].view(np.int64), t[k].view(np.int64)) for k in t)


# ---- streams --------------------------------------------------------------------------------------------------------------------------------

def test_a_protected_half_and_a_half_that_pays():
    """128 x 192, price 0 on the left half and 4 on the right, rdo = 2: the left half keeps its symbols and its bits, the right pays."""
    comp, _ = _model()
    H, W = 128, 192
    images = _images(1, H, W)
    latent, hyper, streams0, q0, qh, mean, scale = _analysed(1, H, W)
    pm = np.zeros((H, W), np.float32)
    pm[:, W // 2:] = 4.0
    cells = comp.price_cells(pm, (H, W))
    assert cells.shape == (1, 8, 12) and np.all(cells[:, :, :6] == 0) and np.all(cells[:, :, 6:] == 4)
    streams = comp.compress_to_bytes(images, rdo=2.0, price_map=pm)
    assert streams == comp.latents_to_bytes(latent, hyper, rdo=2.0, price_cells=cells) == comp.compress_to_bytes(images, rdo=2.0, price_cells=cells)
    q, qh2 = comp.decompress_from_bytes(streams, return_hyper=True)
    assert np.array_equal(_bits32(qh2), _bits32(qh))
    assert np.array_equal(_bits32(q[:, :, :, :6]), _bits32(q0[:, :, :, :6]))             # every left-half position: the plain symbols
    assert np.any(_bits32(q[:, :, :, 6:]) != _bits32(q0[:, :, :, 6:]))
    rm0 = comp.rate_map(qh, q0, mean, scale)["cell"]
    rm = comp.rate_map(qh, q, mean, scale)["cell"]
    assert np.array_equal(_bits32(rm[:, :, :6]), _bits32(rm0[:, :, :6]))
    right, right0 = rm[:, :, 6:].astype(np.float64).sum(), rm0[:, :, 6:].astype(np.float64).sum()
    print(f"[price] right half: {right0:.1f} -> {right:.1f} bits, {len(streams0[0])} -> {len(streams[0])} bytes")
    assert right <= right0 and len(streams[0]) <= len(streams0[0])
    # the same decision through encode / forward
    qe, _, st = comp.encode(images, rdo=2.0, price_map=pm)
    assert np.array_equal(_bits32(qe), _bits32(q)) and st["rdo_moved"][0] == (_bits32(q) != _bits32(q0)).sum()
    out = comp.forward(images, rdo=2.0, price_map=pm.astype(bool) * np.float32(4.0), return_rate_map=True)
    assert np.array_equal(_bits32(out["q_latent"]), _bits32(q)) and np.array_equal(_bits32(out["rate_map"]), _bits32(rm))


def test_stream_identities_and_per_image_maps():
    comp, _ = _model()
    H, W = 128, 192
    images = _images(3, H, W)
    latent, hyper, streams0 = _analysed(3, H, W)[:3]
    plain = list(streams0)
    mu3 = [0.5, 2.0, 8.0]
    with_rdo = comp.compress_to_bytes(images, rdo=mu3)
    assert with_rdo != plain
    assert comp.compress_to_bytes(images, rdo=mu3, price_map=np.ones((H, W), np.float32)) == with_rdo      # all-ones map = the rdo= bytes
    assert comp.compress_to_bytes(images, rdo=mu3, price_map=np.ones((3, 1, H, W), bool)) == with_rdo
    pm = PR.dyadic_map(3, H, W, seed=11)
    assert comp.compress_to_bytes(images, rdo=0.0, price_map=pm) == plain                                    # rdo = 0 = the plain bytes
    assert comp.compress_to_bytes(images) == plain                                                           # the handle keeps nothing
    # per-image maps in a batch of 3 = the three batch-1 streams
    cells = comp.price_cells(pm, (H, W))
    streams = comp.latents_to_bytes(latent, hyper, rdo=mu3, price_cells=cells)
    assert streams == comp.compress_to_bytes(images, rdo=mu3, price_map=pm) and streams != with_rdo
    comp.decompress_from_bytes(streams)
    for b in range(3):
        one = comp.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], rdo=mu3[b], price_cells=cells[b:b + 1])
        assert one[0] == streams[b], b
    dev = comp.latents_to_bytes(_dev(latent), _dev(hyper), rdo=mu3, price_cells=cells)
    assert dev == streams
    # an image of any size: the cells of the padding take the nearest cell of the image
    small = _images(1, 100, 150)
    pm2 = PR.dyadic_map(1, 100, 150, seed=5)
    s2 = comp.compress_to_bytes(small, rdo=2.0, price_map=pm2)
    assert s2 == comp.compress_to_bytes(small, rdo=2.0, price_cells=PR.cells_ref(pm2, 100, 150, 16, 8, 12))
    assert comp.decompress_from_bytes(s2, return_image_size=True)[1] == (100, 150)


def test_target_bpp_under_a_map():
    comp, _ = _model()
    H, W = 128, 192
    images = _images(3, H, W)
    plain = comp.compress_to_bytes(images)
    pm = np.full((3, H, W), 0.25, np.float32)
    pm[0, :, W // 2:] = 4.0
    pm[1, H // 2:] = 0.0
    cells = comp.price_cells(pm, (H, W))
    ladder = LADDERS[18]
    curve = comp.rate_sweep(images, ladder, price_map=pm)
    bpp = curve["bpp"]
    assert np.array_equal(bpp[:, 0], comp.rate_sweep(images, ladder[:1])["bpp"][:, 0])            # mu = 0: the map does not matter
    js = [int(np.nonzero(np.diff(bpp[b]) < 0)[0][-1]) + 1 for b in range(3)]
    target = np.array([0.5 * (bpp[b, j] + bpp[b, j - 1]) for b, j in enumerate(js)])
    streams, info = comp.compress_to_bytes(images, target_bpp=target, price_map=pm, return_info=True)
    assert info["met"].all() and np.all(info["estimated_bpp"] <= target) and info["reencodes"] == 0
    for b, j in enumerate(js):
        lo, hi = ladder[j - 1], ladder[j]
        assert lo < info["mu"][b] <= hi                                       # "mu" is the base price the map multiplies
        fine = C.rdo_refine_ladder(lo, hi)
        k = int(np.nonzero(fine == info["mu"][b])[0][0])
        below = comp.rate_sweep(images[b:b + 1], fine[k - 1:k + 1], price_cells=cells[b:b + 1])["bpp"][0]
        assert below[0] > target[b] >= below[1], (b, below, target[b])        # the refining sweep saw the image's own map row
        assert len(streams[b]) <= len(plain[b])
    assert streams == comp.latents_to_bytes(*_analysed(3, H, W)[:2], rdo=info["mu"], price_cells=cells)
    got = TR._rate_of(comp, streams, (H, W))
    assert np.all(np.abs(got.astype(np.float64) - info["estimated_bpp"]) <= 4.0 * np.spacing(got)), (got, info["estimated_bpp"])
    print(f"[price] target_bpp {target} under a map -> mu {info['mu']}, estimated {info['estimated_bpp']}, moved {info['moved']}")
    s2, i2 = comp.compress_to_bytes(images, max_bytes=[int(0.95 * len(s)) for s in plain], price_map=pm, return_info=True)
    comp.decompress_from_bytes(s2)
    assert all(len(a) <= len(b) for a, b in zip(s2, plain))


def test_a_map_without_mu_and_maps_that_do_not_fit_are_refused():
    comp, _ = _model()
    L, h = _lib.lib(), comp._hyper_handle()
    latent, hyper, streams0 = _analysed(3, 128, 192)[:3]
    cells = np.ones((1, 8, 12), np.float32)
    try:
        assert L.cdc_set_rdo_map(h, cells.ctypes.data, 1, 8, 12, 0, None) == 0
        with pytest.raises(_lib.CdcError, match="no mu"):                     # never a silent no-op
            comp.latents_to_bytes(latent, hyper)
        buf, offs = np.empty(1 << 20, np.uint8), (ctypes.c_size_t * 4)()
        med = comp._median_vector()
        assert L.cdc_entropy_encode(h, latent.ctypes.data, hyper.ctypes.data, med.ctypes.data, 3, 2, 3, buf.ctypes.data, buf.size, offs, 0, None) == -2
        assert comp.latents_to_bytes(latent, hyper, rdo=0.0) == list(streams0)              # with a mu the handle's map is used
        for bad in (-1.0, np.nan, np.inf):                                   # validated before it replaces the handle's map
            c = np.ones((3, 8, 12), np.float32)
            c[1, 2, 3] = bad
            assert L.cdc_set_rdo_map(h, c.ctypes.data, 3, 8, 12, 0, None) == -1 and b"finite and >= 0" in L.cdc_last_error(h)
            assert L.cdc_set_rdo_map(h, _dev(c).data_ptr(), 3, 8, 12, 1, None) == -1
        assert comp.latents_to_bytes(latent, hyper, rdo=0.0) == list(streams0)
        assert L.cdc_set_rdo_map(h, cells.ctypes.data, 1, 4, 24, 0, None) == 0              # the same number of positions, another grid
        with pytest.raises(_lib.CdcError, match="latent grid"):
            comp.latents_to_bytes(latent, hyper, rdo=1.0)
        with pytest.raises(_lib.CdcError, match="latent grid"):
            comp._sweep(latent, hyper, [0.0, 1.0])
        two = np.ones((2, 8, 12), np.float32)
        assert L.cdc_set_rdo_map(h, two.ctypes.data, 2, 8, 12, 0, None) == 0
        with pytest.raises(_lib.CdcError, match="1 or 3 expected"):
            comp.latents_to_bytes(latent, hyper, rdo=1.0)
    finally:
        assert L.cdc_set_rdo_map(h, None, 0, 0, 0, 0, None) == 0
    assert comp.latents_to_bytes(latent, hyper) == list(streams0)
    with pytest.raises(ValueError, match="latent grid"):                     # the mirror checks the grid before the library
        comp.latents_to_bytes(latent, hyper, rdo=1.0, price_cells=np.ones((4, 24), np.float32))


# ---- one end-to-end ---------------------------------------------------------------------------------------------------------------------

def test_diffusion_with_a_price_map():
    """GaussianDiffusion.compress_to_bytes(target_bpp=, price_map=mask) -> decompress on a 100 x 150 image (no quality claim), and
    evaluate(price_map=, maps=True): the three maps on one grid."""
    meta = json.load(open(os.path.join(TR.GOLDEN, "manifest_anysize_small.json")))["x"]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0))
    comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
    comp.load_state_dict(synth.unet_state_dict([(k, tuple(v)) for k, v in meta["comp_manifest"]], seed=meta["seed"]))
    diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    H, W = 100, 150
    images = M.as_u8(M.picture(2, H, W))
    mask = np.zeros((H, W), bool)
    mask[:, W // 2:] = True                                                  # the left half is protected
    plain = diff.compress_to_bytes(images)
    base = comp.rate_sweep(images, [0.0, 256.0], price_map=mask)["bpp"]
    assert np.all(base[:, 1] < base[:, 0])
    target = 0.5 * (base[:, 0] + base[:, 1])
    streams, info = diff.compress_to_bytes(images, target_bpp=target, price_map=mask, return_info=True)
    assert len(streams) == 2 and info["met"].all() and np.all(info["estimated_bpp"] <= target) and np.all(info["mu"] > 0)
    assert all(len(a) <= len(b) for a, b in zip(streams, plain))
    rec = diff.decompress(streams, sample_steps=2, seed=1, gamma=0.8)
    assert tuple(rec.shape) == (2, 3, H, W) and np.all(np.isfinite(np.asarray(rec)))
    cell = comp.rate_map_cell
    q, q0 = comp.decompress_from_bytes(streams), comp.decompress_from_bytes(plain)
    half = (W // 2) // cell                                                  # latent columns wholly inside the protected half
    assert np.array_equal(_bits32(q[:, :, :, :half]), _bits32(q0[:, :, :, :half])) and np.any(_bits32(q) != _bits32(q0))
    out = diff.evaluate(images, sample_steps=2, seed=1, gamma=0.8, rdo=info["mu"], price_map=mask, maps=True)
    grid = out["rate_map"].shape[1:]
    assert out["map_cell"] == cell and out["sse_map"].shape[1:] == grid and out["price_cells"].shape == (1,) + tuple(grid)
    Hp, Wp = diff.padded_size(H, W)
    assert tuple(grid) == (Hp // cell, Wp // cell)
    assert np.array_equal(_bits32(out["price_cells"]), _bits32(comp.price_cells(mask, (H, W), (Hp, Wp))))
    assert np.allclose(np.asarray(out["bpp"], np.float64), info["estimated_bpp"], rtol=1e-6)
    # the figure a region-of-interest user reports: equal weights give psnr's own MSE; the mask's weights the region's
    eq = metrics.psnr_weighted(un, out["reconstruction"], images, np.ones(grid), cell, as_saved=True)
    assert np.allclose(eq, out["psnr"], rtol=1e-12, atol=0)
    roi = metrics.psnr_weighted(un, out["reconstruction"], images, 1.0 - out["price_cells"], cell, as_saved=True)
    w = 1.0 - out["price_cells"].astype(np.float64)
    want = 10.0 * np.log10(1.0 / ((w * out["sse_map"]).reshape(2, -1).sum(1) / (w * out["sse_count"]).reshape(2, -1).sum(1)))
    assert np.allclose(roi, want, rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="need one of rdo"):
        diff.evaluate(images, sample_steps=2, price_map=mask)
