"""Tiled decode without a GPU: the tile plan and the feather weights of cdc_compression_amd/tiles.py against the float64 restatement
of tests/tiles_ref.py, the frame-indexed draws of cdc_randn_framed_host against crops of cdc_randn_host (bit for bit: both are
csrc/rng.h on the CPU), and the argument rules of decompress(tile=...)."""
import ctypes
import os
import re

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, tiles
import tiles_ref as R
from test_rng import randn_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 16
PLANS = [(2 * G, G), (4 * G, G), (4 * G, 2 * G), (8 * G, G), (8 * G, 3 * G), (6 * G, 3 * G)]


@pytest.mark.parametrize("tile,overlap", PLANS)
def test_plan_covers_the_frame_with_tiles_inside_it(tile, overlap):
    three_way = False
    for n in range(1, 41):
        L = n * G
        origins, size = tiles.axis_origins(L, tile, overlap)
        assert (origins, size) == R.axis_plan(L, tile, overlap)
        assert all(o % G == 0 for o in origins) and size % G == 0
        assert all(0 <= o and o + size <= L for o in origins)
        assert origins == sorted(set(origins))
        cov = R.cover(origins, size, L)
        assert cov.min() >= 1
        three_way |= cov.max() >= 3
        assert cov.max() <= 3
        if L <= tile:
            assert origins == [0] and size == L
        else:
            assert size == tile and origins[0] == 0 and origins[-1] == L - tile
            for a, b in zip(origins, origins[1:]):
                assert a + size - b >= overlap, (L, a, b)
            assert all(b - a == tile - overlap for a, b in zip(origins[:-2], origins[1:-1]))
    # three tiles meet where the shifted last tile starts inside the overlap of the two before it: L - tile strictly between the last
    # regular origin and that origin + overlap, which a multiple of G can be only when overlap >= 2 G
    assert three_way == (overlap >= 2 * G)


def test_plan_numbers_the_tiles_row_major_and_finds_the_ones_under_a_region():
    p = tiles.Plan(6 * G, 5 * G, (4 * G, 4 * G), (G, G))
    assert (p.ys, p.xs, p.th, p.tw, p.T) == ([0, 2 * G], [0, G], 4 * G, 4 * G, 4)
    assert p.origins() == [(0, 0), (0, G), (2 * G, 0), (2 * G, G)]
    assert p.intersecting(None) == [0, 1, 2, 3]
    assert p.intersecting((0, 0, G, G)) == [0]                             # inside tile 0 alone
    assert p.intersecting((2 * G - 1, G - 1, 2, 2)) == [0, 1, 2, 3]         # across the four-tile corner
    assert p.intersecting((5 * G, 0, G, G)) == [2]
    assert p.intersecting((5 * G, 4 * G + 3, 1, 1)) == [3]
    one = tiles.Plan(6 * G, 5 * G, (8 * G, 8 * G), (G, G))
    assert (one.T, one.th, one.tw, one.origins()) == (1, 6 * G, 5 * G, [(0, 0)])
    assert tiles.default_chunk(4) == 4 and tiles.default_chunk(32) == 32 and tiles.default_chunk(33) == 17 and tiles.default_chunk(65) == 22


@pytest.mark.parametrize("tile,overlap", PLANS)
def test_weights(tile, overlap):
    """Two tiles over exactly `overlap` sum to 1 there; the sum is positive everywhere; a tile's weight is 1 on a frame border."""
    for n in range(1, 41):
        L = n * G
        origins, size = tiles.axis_origins(L, tile, overlap)
        total = np.zeros(L)
        cov = R.cover(origins, size, L)
        for o in origins:
            p = np.arange(o, o + size)
            w = tiles.axis_weight(p, o, size, L, overlap)
            np.testing.assert_array_equal(w, R.axis_weight(p, o, size, L, overlap))
            assert w.min() > 0 and w.max() <= 1
            total[o:o + size] += w
        assert total.min() > 0
        assert total[0] == 1.0 and total[-1] == 1.0
        first, last = origins[0], origins[-1]
        assert tiles.axis_weight(0, first, size, L, overlap) == 1.0 and tiles.axis_weight(L - 1, last, size, L, overlap) == 1.0
        for a, b in zip(origins, origins[1:]):
            if a + size - b == overlap:                      # a two-tile overlap of length exactly `overlap`
                seg = slice(b, a + size)
                if cov[seg].max() == 2:
                    np.testing.assert_allclose(total[seg], 1.0, rtol=0, atol=1e-15)
        if len(origins) == 1:
            np.testing.assert_array_equal(total, 1.0)


def _crop(full, C, fh, fw, y0, x0, th, tw):
    return full.reshape(C, fh, fw)[:, y0:y0 + th, x0:x0 + tw]


FRAMED_CASES = [
    # (C, frame_h, frame_w, y0, x0, th, tw): the quad path (everything a multiple of 4), an odd x0, a frame width that is no multiple of 4
    (3, 24, 32, 4, 8, 12, 16),
    (3, 24, 32, 5, 3, 12, 16),
    (3, 20, 50, 2, 8, 9, 40),
    (3, 20, 50, 0, 0, 20, 50),
    (1, 7, 9, 6, 8, 1, 1),
]


@pytest.mark.parametrize("draw", [0, 5])
@pytest.mark.parametrize("case", FRAMED_CASES)
def test_framed_host_fill_is_the_crop_of_the_full_frame_fill(case, draw):
    C, fh, fw, y0, x0, th, tw = case
    seed = (3 << 33) + 17
    full = randn_host([seed], C * fh * fw, draw, 0.8)[0]
    got = tiles.randn_framed_host([seed], [(fh, fw, y0, x0)], C, th, tw, draw=draw, scale=0.8)
    assert got.shape == (1, C, th, tw)
    np.testing.assert_array_equal(got[0].view(np.uint32), _crop(full, C, fh, fw, y0, x0, th, tw).view(np.uint32))


def test_framed_host_fill_two_rows_with_their_own_frames_and_seeds():
    seeds = [1234, 2 ** 64 - 1]
    frames = [(24, 32, 4, 8), (20, 50, 7, 3)]
    got = tiles.randn_framed_host(seeds, frames, 3, 12, 16, draw=5)
    for b, (fh, fw, y0, x0) in enumerate(frames):
        full = randn_host([seeds[b]], 3 * fh * fw, 5)[0]
        np.testing.assert_array_equal(got[b].view(np.uint32), _crop(full, 3, fh, fw, y0, x0, 12, 16).view(np.uint32))
    assert not np.array_equal(got[0], got[1])


def test_framed_host_fill_refuses_windows_outside_their_frame():
    L = _lib.lib()
    out = np.empty((1, 3, 4, 4), np.float32)
    sd = np.asarray([1], np.uint64)
    for rows in ([8, 8, 5, 0], [8, 8, 0, 5], [8, 8, -1, 0], [0, 8, 0, 0], [8, 8, 8, 0]):
        r = np.asarray(rows, np.int32)
        assert L.cdc_randn_framed_host(sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 3, 4, 4,
                                       0, 1.0, out.ctypes.data) != 0, rows
    with pytest.raises(_lib.CdcError):
        tiles.randn_framed_host([1], [(8, 8, 5, 0)], 3, 4, 4)


def test_entry_points_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "cdc_hip.h")).read()
    L = _lib.lib()
    for name in ("cdc_set_noise_frames", "cdc_randn_framed", "cdc_randn_framed_host", "cdc_tile_gather", "cdc_tile_blend"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(L, name)


def test_set_noise_frames_argument_rules():
    """On a handle that never touches a device: kinds, n, rows; n = 0 clears with or without a pointer."""
    L = _lib.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)
    un = cdc.Unet(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    h = un._handle()
    ok = np.asarray([[64, 64, 0, 16], [64, 64, 32, 0]], np.int32)
    assert L.cdc_set_noise_frames(h, ok.ctypes.data_as(i32p), 2) == 0
    assert L.cdc_set_noise_frames(h, None, 0) == 0
    assert L.cdc_set_noise_frames(h, ok.ctypes.data_as(i32p), 0) == 0
    assert L.cdc_set_noise_frames(h, None, 2) != 0
    assert L.cdc_set_noise_frames(h, ok.ctypes.data_as(i32p), -1) != 0
    for bad in ([0, 64, 0, 0], [64, 64, 64, 0], [64, 64, 0, -4]):
        r = np.asarray([bad], np.int32)
        assert L.cdc_set_noise_frames(h, r.ctypes.data_as(i32p), 1) != 0, bad
    comp = cdc.BigCompressor(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3)
    assert L.cdc_set_noise_frames(comp._handle(), ok.ctypes.data_as(i32p), 2) != 0        # a U-Net handle's state


def test_decompress_checks_the_tile_arguments_before_the_library_is_touched():
    """No weights are loaded: the refusal is the argument's, not a missing state dict's."""
    kw = dict(dim=16, channels=3, context_channels=3, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    diff = cdc.GaussianDiffusionEps(cdc.Unet(**kw), cdc.BigCompressor(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3),
                                    num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")
    M = diff.padded_size(1, 1)[0]
    q = np.zeros((1, 48, 8 * M // 4, 8 * M // 4), np.float32)
    dec = lambda **k: diff.decompress(q, (1, 3, 8 * M, 8 * M), sample_steps=2, **k)      # noqa: E731
    with pytest.raises(ValueError, match="samples exclude"):
        dec(tile=2 * M, samples=2, seed=1, gamma=0.8)
    with pytest.raises(ValueError, match="trajectory exclude"):
        dec(tile=2 * M, trajectory=[0])
    with pytest.raises(ValueError, match="belongs to tile"):
        dec(region=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="belongs to tile"):
        dec(tile_overlap=M)
    with pytest.raises(ValueError, match="belongs to tile"):
        dec(tile_chunk=2)
    with pytest.raises(ValueError, match="multiple of the model's frame multiple"):
        dec(tile=2 * M + 1)
    with pytest.raises(ValueError, match="multiple of the model's frame multiple"):
        dec(tile=4 * M, tile_overlap=M + 1)
    with pytest.raises(ValueError, match="overlap <= tile / 2"):
        dec(tile=2 * M, tile_overlap=2 * M)
    with pytest.raises(ValueError, match="overlap <= tile / 2"):
        dec(tile=M)                                                          # the default overlap is the multiple itself
    with pytest.raises(ValueError, match="overlap <= tile / 2"):
        dec(tile=(4 * M, 2 * M), tile_overlap=(M, 2 * M))
    with pytest.raises(ValueError, match="positive"):
        dec(tile=0)
    with pytest.raises(ValueError, match="int or a pair"):
        dec(tile=2.5 * M)
    with pytest.raises(ValueError, match="tile_chunk must be an int >= 1"):
        dec(tile=2 * M, tile_chunk=0)
    with pytest.raises(ValueError, match="region must be"):
        dec(tile=2 * M, region=(0, 0, 8))
    with pytest.raises(ValueError, match="h, w >= 1"):
        dec(tile=2 * M, region=(0, 0, 0, 8))
    with pytest.raises(ValueError, match="reaches outside"):
        dec(tile=2 * M, region=(0, 8 * M - 4, 8, 8))
    with pytest.raises(ValueError, match="needs a seed"):
        dec(tile=2 * M, eta=0.5)
    with pytest.raises(ValueError, match="needs a seed"):
        dec(tile=2 * M, gamma=0.8)
    with pytest.raises(ValueError, match="needs the latent"):
        diff.decompress([q], (1, 3, 8 * M, 8 * M), sample_steps=2, tile=2 * M)
    img = np.zeros((1, 3, 8 * M, 8 * M), np.float32)
    with pytest.raises(ValueError, match="maps=True exclude"):
        diff.evaluate(img, sample_steps=2, sample_mode="ddim", tile=2 * M, maps=True)
    with pytest.raises(ValueError, match="region belongs to compress"):
        diff.evaluate(img, sample_steps=2, sample_mode="ddim", tile=2 * M, region=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="trajectory exclude"):
        diff.compress(img, sample_steps=2, sample_mode="ddim", tile=2 * M, trajectory=[0])
