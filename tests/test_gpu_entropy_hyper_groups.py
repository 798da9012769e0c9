"""Grouped hyper part (container versions 19 - 22) on the MI355X: the product's streams against the Python-built streams of oracle
groups and segments byte for byte (tests/hyper_groups_ref.py restates the format), the full and the windowed decode against the
ungrouped and the unsegmented stream's decode bit for bit, corruption refused with image and group named, and the default path.
Weights are synthetic: nothing here is about quality."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from oracle import entropy as oe
from helpers import GOLDEN
import hyper_groups_ref as hr
import segments_ref as sr

pytestmark = pytest.mark.gpu

CELL = 16                                                          # image pixels per latent position of every model here
HW = (128, 192)                                                    # latent 8 x 12, hyper-latent 2 x 3: per = 6 symbols a channel
GROUPS = {32: (1, 32), 7: (5, 7), 3: (11, 3), 1: (32, 1)}          # hyper_groups=G -> (cg, ng) of 32 channels


def _bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def _symbols(comp, latent, hyper, med, b, rate=None):
    """What the coder codes of image b, from the public calls at batch 1 (the coder's plan): (sym_h, sym_l, scale, q_latent, q_hyper)."""
    lat, hyp = latent[b:b + 1], hyper[b:b + 1]
    q_hyper = comp.dequantize(hyp, comp._medians_like(hyp))
    mean, scale = comp.hyper_decode(q_hyper) if rate is None else comp.hyper_decode(q_hyper, cond=np.float32([rate]))
    q_latent = comp.dequantize(lat, mean)
    sym_h = np.rint(q_hyper[0] - med[:, None, None]).astype(np.int32)
    sym_l = np.rint(q_latent[0] - mean[0]).astype(np.int32)
    return sym_h, sym_l, scale[0], q_latent, q_hyper


@pytest.fixture(scope="module")
def small():
    """The 32-channel compressor of tests/test_gpu_entropy_segments.py."""
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3,
                                out_channels=8)
    sd = synth.unet_state_dict(comp.manifest() + comp.hyper_manifest() + comp.encoder_manifest(), seed=5)
    C = comp.reversed_hyper_dims[0]
    sd.update(sr.prior_sd(C, seed=7))
    comp.load_state_dict(sd)
    assert comp.rate_map_cell == CELL and C == 32
    return comp, oe.raw_prior(sd, C), comp._median_vector()


@pytest.fixture(scope="module")
def coded(small):
    """The analysis of a batch of 3 with hyper latents far outside the tables in channels 3 and 20, what the coder codes of each image,
    the unsegmented and the segmented streams and their decode -- computed once, left unchanged."""
    comp, prior, med = small
    x = synth.normal("img", (3, 3) + HW, seed=13, std=0.6)
    latent, hyper = comp.analysis(x)
    hyper = np.array(hyper, np.float32)
    hyper[:, 3, 1, 2] += 1500.0                                    # beyond every table (K <= 1024): escapes
    hyper[1:, 20, 0, 0] -= 1200.0
    plain = comp.latents_to_bytes(latent, hyper)
    q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
    syms = [_symbols(comp, latent, hyper, med, b) for b in range(3)]
    cut = {seg: tuple(comp.latents_to_bytes(latent, hyper, segment=seg * CELL)) for seg in (8, 5)}
    for a in (latent, hyper, q, qh):
        a.setflags(write=False)
    return latent, hyper, tuple(plain), q, qh, syms, cut


@pytest.mark.parametrize("G", [32, 7, 3, 1])
@pytest.mark.parametrize("seg", [8, 5])
def test_streams_equal_the_oracle_groups_byte_for_byte_and_decode_whole(small, coded, seg, G):
    comp, prior, med = small
    latent, hyper, plain, q, qh, syms, cut = coded
    cg, ng = GROUPS[G]
    streams = comp.latents_to_bytes(latent, hyper, segment=seg * CELL, hyper_groups=G)
    grid = (-(-8 // seg), -(-12 // seg))
    assert comp.hyper_groups_of(streams) == [(cg, ng)] * 3 and comp.segments_of(streams) == [(seg,) + grid] * 3
    assert comp.hyper_groups_of(plain) == [(0, 1)] * 3 and comp.hyper_groups_of(cut[seg]) == [(0, 1)] * 3
    for b in range(3):
        sym_h, sym_l, scale, q_latent, q_hyper = syms[b]
        escapes = [e[1] for e in hr.hyper_part(sym_h, prior, med, cg)[3]]
        assert max(escapes) > 0 and (ng == 1 or min(escapes) == 0), escapes    # groups with escapes and groups without any
        assert streams[b][4] == plain[b][4]                                   # the arithmetic hyper_dec ran in
        ref = hr.oracle_stream(sym_h, sym_l, scale, prior, med, seg, cg, arith=plain[b][4])      # (asserts that the checksums add up to `symbols`)
        assert streams[b][3] == 19 and streams[b] == ref, (b, len(streams[b]), len(ref))
        assert streams[b][22:26] == plain[b][22:26] == cut[seg][b][22:26]      # `symbols`: that of the ungrouped streams
        assert comp.latents_to_bytes(latent[b:b + 1], hyper[b:b + 1], segment=seg * CELL, hyper_groups=G)[0] == streams[b]     # batch == batch 1
        one, one_h = comp.decompress_from_bytes([streams[b]], return_hyper=True)
        np.testing.assert_array_equal(_bits(one), _bits(q[b:b + 1]))
        np.testing.assert_array_equal(_bits(one_h), _bits(qh[b:b + 1]))
        np.testing.assert_array_equal(one, q_latent)
    ql, qhl, counts = comp.decompress_from_bytes(streams, return_hyper=True, return_segments=True)
    np.testing.assert_array_equal(_bits(ql), _bits(q))
    np.testing.assert_array_equal(_bits(qhl), _bits(qh))
    c11, c11h = comp.decompress_from_bytes(cut[seg], return_hyper=True)
    np.testing.assert_array_equal(_bits(ql), _bits(c11))
    np.testing.assert_array_equal(_bits(qhl), _bits(c11h))
    assert counts == (grid[0] * grid[1],) * 2
    # the handle is back on ungrouped and on unsegmented streams
    assert tuple(comp.latents_to_bytes(latent, hyper, segment=seg * CELL)) == cut[seg] and comp.latents_to_bytes(latent, hyper) == list(plain)


def test_default_path_writes_the_version_11_stream(small, coded):
    comp, prior, med = small
    latent, hyper, plain, q, qh, syms, cut = coded
    streams = comp.latents_to_bytes(latent, hyper, segment=5 * CELL, hyper_groups=None)
    for b in range(3):
        sym_h, sym_l, scale, _, _ = syms[b]
        ref = sr.oracle_stream(sym_h, sym_l, scale, prior, med, 5, arith=plain[b][4])
        assert streams[b][3] == 11 and hashlib.sha256(streams[b]).hexdigest() == hashlib.sha256(ref).hexdigest()


def test_groups_without_segments_are_refused_by_the_library(small, coded):
    comp, _, _ = small
    latent, hyper, plain = coded[:3]
    L, h = _lib.lib(), comp._hyper_handle()
    assert L.cdc_entropy_set_hyper_groups(h, 33) == -1 and L.cdc_entropy_set_hyper_groups(h, -1) == -1
    assert L.cdc_entropy_set_hyper_groups(h, 5) == 0
    try:
        with pytest.raises(_lib.CdcError, match="cdc_entropy_set_segments"):
            comp.latents_to_bytes(latent, hyper)
        assert comp.hyper_groups_of(comp.latents_to_bytes(latent, hyper, segment=5 * CELL)) == [(5, 7)] * 3
    finally:
        assert L.cdc_entropy_set_hyper_groups(h, 0) == 0
    assert comp.latents_to_bytes(latent, hyper) == list(plain)


@pytest.mark.parametrize("hw,G,want", [((256, 256), 4, (64, 4)), ((512, 384), 16, (16, 16))])
def test_full_compressor(hw, G, want):
    from test_entropy import _full_compressor
    comp, sd = _full_compressor()
    C = comp.reversed_hyper_dims[0]
    assert C == 256
    prior, med = oe.raw_prior(sd, C), comp._median_vector()
    x = synth.normal("img", (1, 3) + hw, seed=4, std=0.4)
    latent, hyper = comp.analysis(x)
    assert hyper.shape == (1, 256, hw[0] // 64, hw[1] // 64)
    streams = comp.latents_to_bytes(latent, hyper, segment=8 * comp.rate_map_cell, hyper_groups=G)
    sym_h, sym_l, scale, q_latent, q_hyper = _symbols(comp, latent, hyper, med, 0)
    ref = hr.oracle_stream(sym_h, sym_l, scale, prior, med, 8, want[0])
    assert comp.hyper_groups_of(streams) == [want] and streams[0] == ref
    ql, qh = comp.decompress_from_bytes(streams, return_hyper=True)
    np.testing.assert_array_equal(ql, q_latent)
    np.testing.assert_array_equal(qh, q_hyper)


def test_recorded_size_rdo_price_map_and_max_bytes_compose(small):
    comp, prior, med = small
    x = synth.normal("img", (2, 3, 100, 150), seed=21, std=0.6)
    plain = comp.compress_to_bytes(x)
    streams = comp.compress_to_bytes(x, segment=5 * CELL, hyper_groups=7)
    assert [s[3] for s in plain] == [5, 5] and [s[3] for s in streams] == [21, 21]
    assert comp.image_size_of(streams) == [(100, 150)] * 2 and comp.segments_of(streams) == [(5, 2, 3)] * 2 and comp.hyper_groups_of(streams) == [(5, 7)] * 2
    q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
    for b in range(2):
        mean, scale = comp.hyper_decode(qh[b:b + 1])
        sym_h = np.rint(qh[b] - med[:, None, None]).astype(np.int32)
        sym_l = np.rint(q[b] - mean[0]).astype(np.int32)
        assert streams[b] == hr.oracle_stream(sym_h, sym_l, scale[0], prior, med, 5, 5, version=5, size=(100, 150))
    np.testing.assert_array_equal(_bits(comp.decompress_from_bytes(streams)), _bits(q))
    pm = np.ones((100, 150), np.float32)
    pm[:40, :60] = 0.0
    for kw in (dict(rdo=0.5), dict(rdo=np.float32([0.25, 2.0])), dict(rdo=1.0, price_map=pm)):
        a, ah = comp.decompress_from_bytes(comp.compress_to_bytes(x, **kw), return_hyper=True)
        s = comp.compress_to_bytes(x, segment=2 * CELL, hyper_groups=3, **kw)
        assert [t[3] for t in s] == [21, 21]
        g, gh = comp.decompress_from_bytes(s, return_hyper=True)
        np.testing.assert_array_equal(_bits(g), _bits(a))
        np.testing.assert_array_equal(_bits(gh), _bits(ah))
        assert np.any(_bits(a) != _bits(q))                        # (the quantiser did move symbols)
    x = synth.normal("img", (2, 3) + HW, seed=23, std=0.6)
    sizes = [len(s) for s in comp.compress_to_bytes(x, segment=2 * CELL, hyper_groups=32)]
    assert comp._stream_header_bytes(x, HW, 2 * CELL, 32) == 34 + 8 + 12 * 24 + 8 + 12 * 32
    for budget in (int(0.8 * min(sizes)), 20):                     # reachable; below the container itself
        streams, info = comp.compress_to_bytes(x, max_bytes=budget, segment=2 * CELL, hyper_groups=32, return_info=True)
        assert comp.hyper_groups_of(streams) == [(1, 32)] * 2
        print(f"max_bytes {budget}: {[len(s) for s in streams]} bytes, met {info['met'].tolist()}, mu {info['mu'].tolist()}, reencodes {info['reencodes']}")
        for b in range(2):
            assert (len(streams[b]) <= budget) == bool(info["met"][b])
    assert info["met"].tolist() == [False, False]                  # 20 bytes hold no header


def test_variable_bitrate_streams_are_versions_20_and_22():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_small.json")))
    sd = synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"])
    comp = cdc.BigCompressor(vbr=True, **meta["kwargs"])
    comp.load_state_dict(sd)
    C = comp.reversed_hyper_dims[0]
    prior, med = oe.raw_prior(sd, C), comp._median_vector()
    rates = np.float32([0.1, 0.9])
    cell = comp.rate_map_cell
    G = min(C, 3)
    cg = -(-C // G)
    for hw, version in ((HW, 4), ((100, 150), 6)):
        x = synth.normal("img", (2, 3) + hw, seed=22, std=0.6)
        plain = comp.compress_to_bytes(x, bitrate_scale=rates)
        streams = comp.compress_to_bytes(x, bitrate_scale=rates, segment=3 * cell, hyper_groups=G)
        assert [s[3] for s in plain] == [version] * 2 and [s[3] for s in streams] == [version + 16] * 2
        assert comp.hyper_groups_of(streams) == [(cg, -(-C // cg))] * 2
        np.testing.assert_array_equal(comp.bitrate_scale_of(streams), rates)
        q, qh = comp.decompress_from_bytes(plain, return_hyper=True)
        for b in range(2):
            mean, scale = comp.hyper_decode(qh[b:b + 1], cond=rates[b:b + 1])
            sym_h = np.rint(qh[b] - med[:, None, None]).astype(np.int32)
            sym_l = np.rint(q[b] - mean[0]).astype(np.int32)
            ref = hr.oracle_stream(sym_h, sym_l, scale[0], prior, med, 3, cg, version=version, rate=float(rates[b]),
                                   size=hw if version == 6 else None)
            assert streams[b] == ref, (hw, b)
        g, gh = comp.decompress_from_bytes(streams, return_hyper=True)
        np.testing.assert_array_equal(_bits(g), _bits(q))
        np.testing.assert_array_equal(_bits(gh), _bits(qh))


@pytest.mark.parametrize("window,n_dec", [((1, 1, 3, 3), 1), ((3, 3, 4, 4), 4), ((0, 0, 8, 12), 6), ((7, 11, 1, 1), 1)])
def test_window_decode_is_that_of_the_ungrouped_segmented_stream(small, coded, window, n_dec):
    comp, prior, med = small
    latent, hyper, plain, q, qh, syms, cut = coded
    streams = comp.latents_to_bytes(latent, hyper, segment=5 * CELL, hyper_groups=7)
    want, want_h, want_counts = comp.decompress_from_bytes(cut[5], return_hyper=True, window=window, return_segments=True)
    got, got_h, counts = comp.decompress_from_bytes(streams, return_hyper=True, window=window, return_segments=True)
    assert counts == want_counts == (6, n_dec)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    np.testing.assert_array_equal(_bits(got_h), _bits(want_h))
    np.testing.assert_array_equal(_bits(got_h), _bits(qh))         # every group is decoded, whatever the window
    one = comp.decompress_from_bytes([streams[1]], window=window)
    np.testing.assert_array_equal(_bits(one[0]), _bits(got[1]))    # batch == batch 1


def test_corruption_is_refused_with_image_and_group_named(small, coded):
    comp, prior, med = small
    latent, hyper, plain, q, qh, syms, cut = coded
    s = comp.latents_to_bytes(latent[:2], hyper[:2], segment=5 * CELL, hyper_groups=3)
    good = s[0]
    cg, ng = 11, 3
    entries = [struct.unpack("<III", good[34 + 8 + 12 * i: 34 + 20 + 12 * i]) for i in range(ng)]
    starts = np.cumsum([34 + 8 + 12 * ng] + [e[0] for e in entries])
    assert starts[-1] == 34 + struct.unpack("<I", good[10:14])[0]
    k = 1                                                          # channels 11 - 21
    assert entries[k][0] > 256 + 4 * entries[k][1] + 8
    away = (0, 0, 4, 4)
    for at in (starts[k] + 17, starts[k] + 256 + 3, starts[k + 1] - 1):        # lane states, renormalisation bytes, the last byte
        bad = bytearray(good)
        bad[at] ^= 0x10
        bad = bytes(bad)
        assert comp.hyper_groups_of([bad]) == [(cg, ng)]           # the index is sound: only the decoder can tell
        for call in (lambda: comp.decompress_from_bytes([s[1], bad]), lambda: comp.decompress_from_bytes([s[1], bad], window=away)):
            with pytest.raises(_lib.CdcError, match=r"image 1, hyper group 1 \(channels 11 - 21\)"):
                call()
    bad = good[:34 + 8 + 12 * 2 + 8] + struct.pack("<I", entries[2][2] ^ 0x100) + good[34 + 8 + 12 * 2 + 12:]
    for kw in ({}, {"window": away}):
        with pytest.raises(_lib.CdcError, match=r"image 0, hyper group 2 \(channels 22 - 31\): symbol checksum"):
            comp.decompress_from_bytes([bad], **kw)
    # the header's `symbols` is checked by the full decode (and cannot be by a window)
    bad = good[:22] + struct.pack("<I", struct.unpack("<I", good[22:26])[0] ^ 1) + good[26:]
    with pytest.raises(_lib.CdcError, match="image 0: symbol checksum"):
        comp.decompress_from_bytes([bad])
    assert comp.decompress_from_bytes([bad], window=(0, 0, 8, 12)).shape == (1, 32, 8, 12)
    # groups that are not the handle's: 3 groups of 20 or of 40 channels do not cover 32 (the index itself stays sound)
    for wrong in (20, 40):
        bad = good[:34] + struct.pack("<H", wrong) + good[36:]
        assert comp.hyper_groups_of([bad]) == [(wrong, ng)]
        with pytest.raises(_lib.CdcError, match="image 0: 3 hyper groups of %d channels do not cover" % wrong):
            comp.decompress_from_bytes([bad])
    # one call decodes one form and one group size
    other = comp.latents_to_bytes(latent[:1], hyper[:1], segment=5 * CELL, hyper_groups=7)[0]
    for pair in ([good, cut[5][1]], [cut[5][0], s[1]], [good, other]):
        with pytest.raises(_lib.CdcError, match="image 1: .* one form"):
            comp.decompress_from_bytes(pair)
    np.testing.assert_array_equal(_bits(comp.decompress_from_bytes(s)), _bits(q[:2]))


def test_tiled_region_of_grouped_streams_is_that_of_segmented_streams_bit_for_bit():
    from test_gpu_anysize import _small
    diff, un, comp, _ = _small("x")
    G = diff.padded_size(1, 1)[0]
    H, W = 3 * G, 2 * G
    Ch = comp.reversed_hyper_dims[0]
    img = synth.normal("tiles_image", (2, 3, H, W), seed=31, std=0.5).clip(-1, 1).astype(np.float32)
    seg = diff.compress_to_bytes(img, segment=G)
    grp = diff.compress_to_bytes(img, segment=G, hyper_groups=2)
    cg = -(-Ch // 2)
    assert comp.hyper_groups_of(grp) == [(cg, -(-Ch // cg))] * 2 and comp.segments_of(grp) == comp.segments_of(seg)
    args = dict(sample_steps=2, seed=(3 << 33) + 17, gamma=0.8, eta=0.5, tile=2 * G, tile_overlap=G)
    region = (G // 2, G // 2, G // 4, G // 4)
    a, info_a = diff.decompress(seg, region=region, **args)
    b, info_b = diff.decompress(grp, region=region, **args)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert "hyper_groups" not in info_a and info_b == {**info_a, "hyper_groups": -(-Ch // cg)}
    assert info_a["segments_decoded"] < info_a["segments"]
    np.testing.assert_array_equal(_bits(diff.decompress(grp, **args)), _bits(diff.decompress(seg, **args)))
