"""Segmented streams (container versions 11 - 14) on the MI355X: the product's streams against the Python-built streams of oracle
segments byte for byte (tests/segments_ref.py restates the format), the full and the windowed decode against the unsegmented
stream's decode bit for bit, corruption, and the tiled decode of a region.  Weights are synthetic: nothing here is about quality."""
import json
import os
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth, tiles
from oracle import entropy as oe
from helpers import GOLDEN
import segments_ref as sr

pytestmark = pytest.mark.gpu

CELL = 16                                                          # image pixels per latent position of every model here


def _bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def small():
    """The 32-channel compressor of test_sections_that_do_not_fill_their_last_iteration."""
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3,
                                out_channels=8)
    sd = synth.unet_state_dict(comp.manifest() + comp.hyper_manifest() + comp.encoder_manifest(), seed=5)
    C = comp.reversed_hyper_dims[0]
    sd.update(sr.prior_sd(C, seed=7))
    comp.load_state_dict(sd)
    assert comp.rate_map_cell == CELL
    return comp, oe.raw_prior(sd, C), comp._median_vector()


def _symbols(comp, latent, hyper, med, b, rate=None):
    """What the coder codes of image b, from the public calls at batch 1 (the coder's plan): (sym_h, sym_l, scale, q_latent, q_hyper, mean)."""
    lat, hyp = latent[b:b + 1], hyper[b:b + 1]
    q_hyper = comp.dequantize(hyp, comp._medians_like(hyp))
    mean, scale = comp.hyper_decode(q_hyper) if rate is None else comp.hyper_decode(q_hyper, cond=np.float32([rate]))
    q_latent = comp.dequantize(lat, mean)
    sym_h = np.rint(q_hyper[0] - med[:, None, None]).astype(np.int32)
    sym_l = np.rint(q_latent[0] - mean[0]).astype(np.int32)
    return sym_h, sym_l, scale[0], q_latent, q_hyper, mean


@pytest.fixture(scope="module")
def coded(small):
    """Per (image size): the analysis of a batch of 3, the plain streams and their decode -- computed once, left unchanged."""
    comp, prior, med = small
    out = {}
    for hw in ((128, 192), (64, 64)):
        x = synth.normal("img", (3, 3) + hw, seed=13, std=0.6)
        latent, hyper = comp.analysis(x)
        plain = comp.latents_to_bytes(latent, hyper)
        q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
        for a in (latent, hyper, q, qh):
            a.setflags(write=False)
        out[hw] = (latent, hyper, tuple(plain), q, qh)
    return out


@pytest.mark.parametrize("hw,seg", [((128, 192), 8), ((128, 192), 5), ((64, 64), 1), ((64, 64), 64)])
def test_streams_equal_the_oracle_segments_byte_for_byte_and_decode_whole(small, coded, hw, seg):
    comp, prior, med = small
    latent, hyper, plain, q, qh = coded[hw]
    streams = comp.latents_to_bytes(latent, hyper, segment=seg * CELL)
    Hl, Wl = hw[0] // CELL, hw[1] // CELL
    grid = (-(-Hl // seg), -(-Wl // seg))
    assert comp.segments_of(streams) == [(seg,) + grid] * 3 and comp.segments_of(plain) == [(0, 1, 1)] * 3
    for b in range(3):
        sym_h, sym_l, scale, q_latent, q_hyper, _ = _symbols(comp, latent, hyper, med, b)
        ref = sr.oracle_stream(sym_h, sym_l, scale, prior, med, seg)          # (asserts that the segment checksums add up to `symbols`)
        assert streams[b][3] == 11 and streams[b] == ref, (b, len(streams[b]), len(ref))
        assert struct.unpack("<I", streams[b][22:26])[0] == oe.symbol_hash(sym_h, sym_l) == struct.unpack("<I", plain[b][22:26])[0]
        assert comp.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], segment=seg * CELL)[0] == streams[b]     # batch == batch 1
        one, one_h = comp.decompress_from_bytes([streams[b]], return_hyper=True)
        np.testing.assert_array_equal(_bits(one), _bits(q[b:b + 1]))
        np.testing.assert_array_equal(_bits(one_h), _bits(qh[b:b + 1]))
        np.testing.assert_array_equal(one, q_latent)
    ql, qhl, counts = comp.decompress_from_bytes(streams, return_hyper=True, return_segments=True)
    np.testing.assert_array_equal(_bits(ql), _bits(q))
    np.testing.assert_array_equal(_bits(qhl), _bits(qh))
    assert counts == (grid[0] * grid[1],) * 2
    assert comp.latents_to_bytes(latent, hyper) == list(plain)     # the handle is back on unsegmented streams
    with pytest.raises(_lib.CdcError, match="one form"):
        comp.decompress_from_bytes([streams[0], plain[1]])


def test_recorded_size_rdo_and_price_map_compose(small):
    comp, prior, med = small
    x = synth.normal("img", (2, 3, 100, 150), seed=21, std=0.6)
    plain = comp.compress_to_bytes(x)
    streams = comp.compress_to_bytes(x, segment=5 * CELL)
    assert [s[3] for s in plain] == [5, 5] and [s[3] for s in streams] == [13, 13]
    assert comp.image_size_of(streams) == [(100, 150)] * 2 and comp.segments_of(streams) == [(5, 2, 3)] * 2      # the padded frame: latent 8 x 12
    q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
    for b in range(2):
        mean, scale = comp.hyper_decode(qh[b:b + 1])
        sym_h = np.rint(qh[b] - med[:, None, None]).astype(np.int32)
        sym_l = np.rint(q[b] - mean[0]).astype(np.int32)
        assert streams[b] == sr.oracle_stream(sym_h, sym_l, scale[0], prior, med, 5, version=5, size=(100, 150))
    np.testing.assert_array_equal(_bits(comp.decompress_from_bytes(streams)), _bits(q))
    pm = np.ones((100, 150), np.float32)
    pm[:40, :60] = 0.0
    for kw in (dict(rdo=0.5), dict(rdo=np.float32([0.25, 2.0])), dict(rdo=1.0, price_map=pm)):
        a = comp.decompress_from_bytes(comp.compress_to_bytes(x, **kw))
        s = comp.compress_to_bytes(x, segment=2 * CELL, **kw)
        assert [t[3] for t in s] == [13, 13]
        np.testing.assert_array_equal(_bits(comp.decompress_from_bytes(s)), _bits(a))
        assert np.any(_bits(a) != _bits(q))                        # (the quantiser did move symbols)


def test_variable_bitrate_streams_are_versions_12_and_14():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_small.json")))
    sd = synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"])
    comp = cdc.BigCompressor(vbr=True, **meta["kwargs"])
    comp.load_state_dict(sd)
    C = comp.reversed_hyper_dims[0]
    prior, med = oe.raw_prior(sd, C), comp._median_vector()
    rates = np.float32([0.1, 0.9])
    cell = comp.rate_map_cell
    for hw, version in (((128, 192), 4), ((100, 150), 6)):
        x = synth.normal("img", (2, 3) + hw, seed=22, std=0.6)
        plain = comp.compress_to_bytes(x, bitrate_scale=rates)
        streams = comp.compress_to_bytes(x, bitrate_scale=rates, segment=3 * cell)
        assert [s[3] for s in plain] == [version] * 2 and [s[3] for s in streams] == [version + 8] * 2
        np.testing.assert_array_equal(comp.bitrate_scale_of(streams), rates)
        q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
        for b in range(2):
            mean, scale = comp.hyper_decode(qh[b:b + 1], cond=rates[b:b + 1])
            sym_h = np.rint(qh[b] - med[:, None, None]).astype(np.int32)
            sym_l = np.rint(q[b] - mean[0]).astype(np.int32)
            ref = sr.oracle_stream(sym_h, sym_l, scale[0], prior, med, 3, version=version, rate=float(rates[b]),
                                   size=hw if version == 6 else None)
            assert streams[b] == ref, (hw, b)
        np.testing.assert_array_equal(_bits(comp.decompress_from_bytes(streams)), _bits(q))


def test_full_compressor_four_segments_of_16384_symbols():
    from test_entropy import _full_compressor
    comp, sd = _full_compressor()
    C = comp.reversed_hyper_dims[0]
    prior, med = oe.raw_prior(sd, C), comp._median_vector()
    x = synth.normal("img", (1, 3, 256, 256), seed=4, std=0.4)
    latent, hyper = comp.analysis(x)
    assert latent.shape == (1, 256, 16, 16)
    streams = comp.latents_to_bytes(latent, hyper, segment=8 * comp.rate_map_cell)
    sym_h, sym_l, scale, q_latent, q_hyper, _ = _symbols(comp, latent, hyper, med, 0)
    ref = sr.oracle_stream(sym_h, sym_l, scale, prior, med, 8)
    assert comp.segments_of(streams) == [(8, 2, 2)] and streams[0] == ref
    ql, qh = comp.decompress_from_bytes(streams, return_hyper=True)
    np.testing.assert_array_equal(ql, q_latent)
    np.testing.assert_array_equal(qh, q_hyper)


WINDOWS = [((1, 1, 3, 3), [0]), ((3, 3, 4, 4), [0, 1, 3, 4]), ((0, 0, 8, 12), [0, 1, 2, 3, 4, 5]), ((7, 11, 1, 1), [5]), ((5, 0, 1, 12), [3, 4, 5])]


@pytest.mark.parametrize("window,want", WINDOWS)
def test_window_decodes_the_segments_it_touches_and_leaves_the_mean_elsewhere(small, coded, window, want):
    """Latent 8 x 12 in segments of 5: 2 x 3 segments of 5 / 3 rows and 5 / 5 / 2 columns."""
    comp, prior, med = small
    latent, hyper, plain, q, qh = coded[(128, 192)]
    streams = comp.latents_to_bytes(latent, hyper, segment=5 * CELL)
    wins, _ = sr.windows(8, 12, 5)
    y0, x0, h, w = window
    assert [i for i, (a, b, c, d) in enumerate(wins) if a < y0 + h and y0 < b and c < x0 + w and x0 < d] == want
    got, got_h, counts = comp.decompress_from_bytes(streams, return_hyper=True, window=window, return_segments=True)
    assert counts == (6, len(want))
    np.testing.assert_array_equal(_bits(got_h), _bits(qh))
    inside = np.zeros((8, 12), bool)
    for i in want:
        inside[wins[i][0]:wins[i][1], wins[i][2]:wins[i][3]] = True
    for b in range(3):
        mean, _ = comp.hyper_decode(qh[b:b + 1])
        np.testing.assert_array_equal(_bits(got[b][:, inside]), _bits(q[b][:, inside]))
        np.testing.assert_array_equal(_bits(got[b][:, ~inside]), _bits(mean[0][:, ~inside]))
        one = comp.decompress_from_bytes([streams[b]], window=window)
        np.testing.assert_array_equal(_bits(one[0]), _bits(got[b]))           # batch == batch 1
    # an unsegmented stream decodes whole, whatever the window
    whole, counts = comp.decompress_from_bytes(plain, window=window, return_segments=True)
    np.testing.assert_array_equal(_bits(whole), _bits(q))
    assert counts == (1, 1)
    for bad in ((0, 0, 9, 1), (0, 12, 1, 1), (7, 0, 2, 1)):
        with pytest.raises(_lib.CdcError, match="not inside"):
            comp.decompress_from_bytes(streams, window=bad)
        with pytest.raises(_lib.CdcError, match="not inside"):
            comp.decompress_from_bytes(plain, window=bad)


def test_corruption_is_refused_with_the_segment_named(small, coded):
    comp, prior, med = small
    latent, hyper, plain, q, qh = coded[(128, 192)]
    s = comp.latents_to_bytes(latent[:2], hyper[:2], segment=5 * CELL)
    good = s[0]
    nbh = struct.unpack("<I", good[10:14])[0]
    lat = 34 + nbh
    entries = [struct.unpack("<III", good[lat + 8 + 12 * i: lat + 20 + 12 * i]) for i in range(6)]
    starts = np.cumsum([lat + 8 + 72] + [e[0] for e in entries])
    k = 4                                                          # segment (1, 1): rows 5 - 7, columns 5 - 9
    assert entries[k][0] > 256 + 4 * entries[k][1] + 8
    touching, away = (6, 6, 1, 1), (0, 0, 4, 4)
    for at in (starts[k] + 17, starts[k] + 256 + 3, starts[k + 1] - 1):        # lane states, renormalisation bytes, the last byte
        bad = bytearray(good)
        bad[at] ^= 0x10
        bad = bytes(bad)
        for call in (lambda: comp.decompress_from_bytes([s[1], bad]), lambda: comp.decompress_from_bytes([s[1], bad], window=touching)):
            with pytest.raises(_lib.CdcError, match=r"image 1, segment 4 \(row 1, column 1\)"):
                call()
        got = comp.decompress_from_bytes([s[1], bad], window=away)              # by design not noticed
        np.testing.assert_array_equal(_bits(got[1][:, :5, :5]), _bits(q[0][:, :5, :5]))
    bad = good[:lat + 8 + 12 * k + 8] + struct.pack("<I", entries[k][2] ^ 0x100) + good[lat + 8 + 12 * k + 12:]
    with pytest.raises(_lib.CdcError, match=r"image 0, segment 4 \(row 1, column 1\): symbol checksum"):
        comp.decompress_from_bytes([bad])
    with pytest.raises(_lib.CdcError, match="symbol checksum"):
        comp.decompress_from_bytes([bad], window=touching)
    assert comp.decompress_from_bytes([bad], window=away).shape == (1, 32, 8, 12)
    # the header's `symbols` is checked by the full decode (and cannot be by a window)
    bad = good[:22] + struct.pack("<I", struct.unpack("<I", good[22:26])[0] ^ 1) + good[26:]
    with pytest.raises(_lib.CdcError, match="image 0: symbol checksum"):
        comp.decompress_from_bytes([bad])
    assert comp.decompress_from_bytes([bad], window=(0, 0, 8, 12)).shape == (1, 32, 8, 12)
    # a grid that is not the handle's: 3 x 2 segments of 5 do not tile 8 x 12 (the index itself stays sound)
    bad = good[:lat + 2] + struct.pack("<HH", 3, 2) + good[lat + 6:]
    assert comp.segments_of([bad]) == [(5, 3, 2)]
    with pytest.raises(_lib.CdcError, match="do not tile"):
        comp.decompress_from_bytes([bad])
    # max_image_hw refuses before anything is allocated, as for unsegmented streams
    with pytest.raises(_lib.CdcError, match="exceeds the decoder's limit"):
        comp.decompress_from_bytes([good], max_image_hw=(64, 64))
    np.testing.assert_array_equal(_bits(comp.decompress_from_bytes([good], max_image_hw=(128, 192))), _bits(q[:1]))


def test_max_bytes_counts_the_larger_container(small):
    comp, _, _ = small
    x = synth.normal("img", (2, 3, 128, 192), seed=23, std=0.6)
    sizes = [len(s) for s in comp.compress_to_bytes(x, segment=2 * CELL)]
    for budget in (int(0.8 * min(sizes)), 20):                     # reachable; below the container itself
        streams, info = comp.compress_to_bytes(x, max_bytes=budget, segment=2 * CELL, return_info=True)
        assert comp.segments_of(streams) == [(2, 4, 6)] * 2
        print(f"max_bytes {budget}: {[len(s) for s in streams]} bytes, met {info['met'].tolist()}, mu {info['mu'].tolist()}, reencodes {info['reencodes']}")
        for b in range(2):
            assert (len(streams[b]) <= budget) == bool(info["met"][b])
    assert info["met"].tolist() == [False, False]                  # 20 bytes hold no header


def test_tiled_region_of_segmented_streams_is_that_of_plain_streams_bit_for_bit():
    from test_gpu_anysize import _small
    diff, un, comp, _ = _small("x")
    G = diff.padded_size(1, 1)[0]
    H, W = 6 * G, 5 * G
    cell = 1 << len(comp.rev_mults)
    img = synth.normal("tiles_image", (2, 3, H, W), seed=31, std=0.5).clip(-1, 1).astype(np.float32)
    plain = diff.compress_to_bytes(img)
    seg = diff.compress_to_bytes(img, segment=G)
    n_seg = (H // G) * (W // G)
    assert comp.segments_of(seg) == [(G // cell, H // G, W // G)] * 2
    args = dict(sample_steps=2, seed=(3 << 33) + 17, gamma=0.8, eta=0.5, tile=4 * G, tile_overlap=G)
    plan = tiles.Plan(H, W, (4 * G, 4 * G), (G, G))
    for region, want_tiles, want_segs in (((G // 2, G // 2, G // 4, G // 4), [0], 16),                  # tile 0: 4 G x 4 G of segments
                                          ((2 * G - 3, G - 2, 7, 5), [0, 1, 2, 3], n_seg)):           # the four-tile corner: all
        assert plan.intersecting(region) == want_tiles
        a, info_a = diff.decompress(plain, region=region, **args)
        b, info_b = diff.decompress(seg, region=region, **args)
        np.testing.assert_array_equal(_bits(a), _bits(b))
        assert info_a == {"tiles": 4, "tiles_decoded": len(want_tiles), "region": region}
        assert info_b == {**info_a, "segments": n_seg, "segments_decoded": want_segs}
    assert 16 < n_seg
    np.testing.assert_array_equal(_bits(diff.decompress(seg, **args)), _bits(diff.decompress(plain, **args)))
    q = comp(img)["q_latent"]
    _, info = diff.decompress(q, region=(G // 2, G // 2, G // 4, G // 4), **args)
    assert info == {"tiles": 4, "tiles_decoded": 1, "region": (G // 2, G // 2, G // 4, G // 4)}
