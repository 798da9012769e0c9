"""Partial streams on the MI355X: cdc_entropy_decode_partial against the full decode and hyper_decode's mean, bits compared, at every
prefix that matters and under damage (tests/partial_ref.py says which segment is which by arithmetic on the index); cdc_segment_mask
against its restatement; decompress(partial=True) against the plain decode of the concealed latent.  Weights are synthetic: nothing
here is about quality."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from helpers import GOLDEN
import partial_ref as pr
import segments_ref as sr

pytestmark = pytest.mark.gpu

CELL = 16
OK, ABSENT, DAMAGED = pr.OK, pr.ABSENT, pr.DAMAGED


def _bits(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a))
    return a if a.dtype == np.uint8 else a.astype(np.float32, copy=False).view(np.uint32)


@pytest.fixture(scope="module")
def small():
    """The 32-channel compressor of tests/test_gpu_entropy_segments.py."""
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3,
                                out_channels=8)
    sd = synth.unet_state_dict(comp.manifest() + comp.hyper_manifest() + comp.encoder_manifest(), seed=5)
    sd.update(sr.prior_sd(comp.reversed_hyper_dims[0], seed=7))
    comp.load_state_dict(sd)
    assert comp.rate_map_cell == CELL
    return comp


@pytest.fixture(scope="module")
def coded(small):
    """Per image size: the analysis of a batch of 3, the full decode of the plain streams and hyper_decode's mean per image at batch 1
    (the coder's plan) -- computed once, left unchanged."""
    out = {}
    for hw in ((128, 192), (64, 64)):
        x = synth.normal("img", (3, 3) + hw, seed=13, std=0.6)
        latent, hyper = small.analysis(x)
        q, qh = small.decompress_from_bytes(small.latents_to_bytes(latent, hyper), return_hyper=True)
        mean = np.concatenate([small.hyper_decode(qh[b:b + 1])[0] for b in range(3)])
        for a in (latent, hyper, q, qh, mean):
            a.setflags(write=False)
        out[hw] = (latent, hyper, q, qh, mean)
    return out


def _partial(comp, streams, **kw):
    return comp.decompress_from_bytes(streams, partial=True, return_status=True, return_hyper=True, **kw)


def _flip(s, at, bit=0x10):
    b = bytearray(s)
    b[at] ^= bit
    return bytes(b)


@pytest.mark.parametrize("groups", [None, 3])
@pytest.mark.parametrize("hw,seg", [((128, 192), 8), ((128, 192), 5), ((64, 64), 1), ((64, 64), 64)])
def test_full_length_equals_the_plain_decode(small, coded, hw, seg, groups):
    latent, hyper, q, qh, _ = coded[hw]
    streams = small.latents_to_bytes(latent, hyper, segment=seg * CELL, hyper_groups=groups)
    assert streams[0][3] == (11 if groups is None else 19)
    got, got_h, counts, status = _partial(small, streams, return_segments=True)
    np.testing.assert_array_equal(_bits(got), _bits(q))
    np.testing.assert_array_equal(_bits(got_h), _bits(qh))
    ny, nx = -(-hw[0] // CELL // seg), -(-hw[1] // CELL // seg)
    assert status.shape == (3, ny, nx) and status.dtype == np.uint8 and not status.any()
    assert counts == (ny * nx, ny * nx)
    plain, plain_h = small.decompress_from_bytes(streams, return_hyper=True)
    np.testing.assert_array_equal(_bits(got), _bits(plain))
    np.testing.assert_array_equal(_bits(got_h), _bits(plain_h))


def test_full_length_of_sized_and_variable_bitrate_streams():
    """Versions 13 / 21 (a recorded size) of the small model, 12 / 14 / 20 / 22 of the variable-bitrate model."""
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=8)
    sd = synth.unet_state_dict(comp.manifest() + comp.hyper_manifest() + comp.encoder_manifest(), seed=5)
    sd.update(sr.prior_sd(comp.reversed_hyper_dims[0], seed=7))
    comp.load_state_dict(sd)
    x = synth.normal("img", (2, 3, 125, 185), seed=21, std=0.6)
    for groups, version in ((None, 13), (7, 21)):
        streams = comp.compress_to_bytes(x, segment=5 * CELL, hyper_groups=groups)
        assert [s[3] for s in streams] == [version] * 2
        q = comp.decompress_from_bytes(streams)
        got, size, status = comp.decompress_from_bytes(streams, partial=True, return_status=True, return_image_size=True)
        np.testing.assert_array_equal(_bits(got), _bits(q))
        assert size == (125, 185) and status.shape == (2, 2, 3) and not status.any()
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_small.json")))
    vbr = cdc.BigCompressor(vbr=True, **meta["kwargs"])
    vbr.load_state_dict(synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"]))
    rates = np.float32([0.1, 0.9])
    cell = vbr.rate_map_cell
    for hw, base in (((128, 192), 4), ((100, 150), 6)):
        x = synth.normal("img", (2, 3) + hw, seed=22, std=0.6)
        for groups, version in ((None, base + 8), (2, base + 16)):
            streams = vbr.compress_to_bytes(x, bitrate_scale=rates, segment=3 * cell, hyper_groups=groups)
            assert [s[3] for s in streams] == [version] * 2
            q = vbr.decompress_from_bytes(streams)
            got, r, size, status = vbr.decompress_from_bytes(streams, partial=True, return_status=True, return_bitrate_scale=True, return_image_size=True)
            np.testing.assert_array_equal(_bits(got), _bits(q))
            np.testing.assert_array_equal(r, rates)
            assert size == hw and not status.any()
            # a prefix of image 1 alone: image 0 stays whole, the rates are still read
            ends = vbr.segment_ends(streams[1])
            got, r, status = vbr.decompress_from_bytes([streams[0], streams[1][: ends[1]]], partial=True, return_status=True, return_bitrate_scale=True)
            np.testing.assert_array_equal(r, rates)
            assert not status[0].any() and status[1].reshape(-1)[:2].tolist() == [OK, OK] and (status[1].reshape(-1)[2:] == ABSENT).all()
            np.testing.assert_array_equal(_bits(got[0]), _bits(q[0]))
    # a fixed-rate stream on the variable-bitrate handle stays refused by the same message
    fixed = comp.compress_to_bytes(synth.normal("img", (1, 3, 128, 192), seed=21, std=0.6), segment=3 * CELL)
    for kw in ({}, {"partial": True}):
        with pytest.raises(_lib.CdcError, match="a fixed-rate stream"):
            vbr.decompress_from_bytes(fixed, **kw)


@pytest.mark.parametrize("groups", [None, 7])
@pytest.mark.parametrize("hw,seg", [((128, 192), 8), ((128, 192), 5), ((64, 64), 1), ((64, 64), 64)])
def test_every_prefix_that_matters(small, coded, hw, seg, groups):
    """Each segment boundary e of segment_ends: the lengths e - 1, e, e + 1; floor; floor - 1 is refused.  seg 1: segments of fewer
    symbols than lanes; seg 5: the ragged right and bottom segments."""
    latent, hyper, q, qh, mean = coded[hw]
    Hl, Wl = hw[0] // CELL, hw[1] // CELL
    s = small.latents_to_bytes(latent[:1], hyper[:1], segment=seg * CELL, hyper_groups=groups)[0]
    info = small.stream_info(s)
    ends = small.segment_ends(s)
    assert ends == pr.layout(s)["ends"] and ends[-1] == len(s) == info["declared"]
    lengths = sorted({info["floor"]} | {n for e in ends for n in (e - 1, e, e + 1) if info["floor"] <= n <= len(s)})
    kinds = set()
    for n in lengths:
        got, got_h, status = _partial(small, [s[:n]])
        want = pr.status(s, n, Hl, Wl)
        np.testing.assert_array_equal(status[0], want, err_msg=f"length {n}")
        np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q[:1], mean[:1], status, seg)), err_msg=f"length {n}")
        np.testing.assert_array_equal(_bits(got_h), _bits(qh[:1]))
        assert small.stream_info(s[:n])["complete"] == int((want == OK).sum())
        kinds.add(int((want == OK).sum()))
    assert kinds == set(range(len(ends) + 1))
    with pytest.raises(_lib.CdcError, match="segment index"):
        _partial(small, [s[: info["floor"] - 1]])
    with pytest.raises(_lib.CdcError, match="segment index"):
        _partial(small, [s + b"\0"])


def _damage_case(small, coded, n_images=1):
    latent, hyper, q, qh, mean = coded[(128, 192)]
    s = small.latents_to_bytes(latent[:n_images], hyper[:n_images], segment=5 * CELL)
    lay = pr.layout(s[0])
    return s, lay, q, mean


def test_damage_costs_one_segment(small, coded):
    s, lay, q, mean = _damage_case(small, coded, 2)
    good, starts, entries, lat = s[0], lay["starts"] + [lay["declared"]], lay["entries"], lay["lat"]
    k = 4                                                          # segment (1, 1): rows 5 - 7, columns 5 - 9
    assert entries[k][0] > 256 + 4 * entries[k][1] + 8
    want = np.zeros((1, 2, 3), np.uint8)
    want[0, 1, 1] = DAMAGED
    touching, away = (6, 6, 1, 1), (0, 0, 4, 4)
    cases = [(_flip(good, at), r"image 1, segment 4 \(row 1, column 1\)") for at in (starts[k] + 17, starts[k] + 256 + 3, starts[k + 1] - 1)]
    flipped = good[:lat + 8 + 12 * k + 8] + struct.pack("<I", entries[k][2] ^ 0x100) + good[lat + 8 + 12 * k + 12:]
    cases.append((flipped, r"image 1, segment 4 \(row 1, column 1\): symbol checksum"))
    for bad, message in cases:
        got, _, status = _partial(small, [bad])
        np.testing.assert_array_equal(status, want)
        np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q[:1], mean[:1], want, 5)))
        np.testing.assert_array_equal(_bits(got[0][:, 5:8, 5:10]), _bits(mean[0][:, 5:8, 5:10]))      # the segment's window is the mean
        with pytest.raises(_lib.CdcError, match=message):                                          # the plain decode still refuses it
            small.decompress_from_bytes([s[1], bad])
        # under a window: touching -> DAMAGED, away -> ABSENT (and by design not noticed)
        got, _, status = _partial(small, [bad], window=touching)
        w = np.full((1, 2, 3), ABSENT, np.uint8)
        w[0, 1, 1] = DAMAGED
        np.testing.assert_array_equal(status, w)
        np.testing.assert_array_equal(_bits(got), _bits(mean[:1]))
        got, _, status = _partial(small, [bad], window=away)
        w = np.full((1, 2, 3), ABSENT, np.uint8)
        w[0, 0, 0] = OK
        np.testing.assert_array_equal(status, w)
        np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q[:1], mean[:1], w, 5)))
    # two damaged segments in one image; damage plus truncation in one image
    two = _flip(_flip(good, starts[1] + 17), starts[k] + 17)
    got, _, status = _partial(small, [two])
    want2 = np.uint8([[[OK, DAMAGED, OK], [OK, DAMAGED, OK]]])
    np.testing.assert_array_equal(status, want2)
    np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q[:1], mean[:1], want2, 5)))
    cut = _flip(good, starts[1] + 17)[: starts[k] + 5]
    got, _, status = _partial(small, [cut])
    want3 = np.uint8([[[OK, DAMAGED, OK], [OK, ABSENT, ABSENT]]])
    np.testing.assert_array_equal(status, want3)
    np.testing.assert_array_equal(status, pr.status(good, len(cut), 8, 12, damaged=(1,))[None])
    np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q[:1], mean[:1], want3, 5)))
    # the header's `symbols` is checked exactly when every segment is OK and no window was given
    bad = good[:22] + struct.pack("<I", struct.unpack("<I", good[22:26])[0] ^ 1) + good[26:]
    with pytest.raises(_lib.CdcError, match="image 0: symbol checksum"):
        _partial(small, [bad])
    assert not _partial(small, [bad], window=(0, 0, 8, 12))[2].any()
    assert _partial(small, [bad[: starts[5] + 1]])[2].reshape(-1).tolist() == [OK] * 5 + [ABSENT]


def test_batch_equals_batch_one(small, coded):
    latent, hyper, q, qh, mean = coded[(128, 192)]
    s = small.latents_to_bytes(latent, hyper, segment=5 * CELL)
    lays = [pr.layout(t) for t in s]
    call = [s[0][: lays[0]["ends"][2] + 7], _flip(s[1], lays[1]["starts"][3] + 17), s[2][: lays[2]["floor"]]]
    got, got_h, status = _partial(small, call)
    assert status[0].reshape(-1).tolist() == [OK, OK, OK, ABSENT, ABSENT, ABSENT]
    assert status[1].reshape(-1).tolist() == [OK, OK, OK, DAMAGED, OK, OK]
    assert (status[2] == ABSENT).all()
    np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q, mean, status, 5)))
    np.testing.assert_array_equal(_bits(got[2]), _bits(mean[2]))
    np.testing.assert_array_equal(_bits(got_h), _bits(qh))
    for b in range(3):
        one, one_h, st = _partial(small, [call[b]])
        np.testing.assert_array_equal(_bits(one[0]), _bits(got[b]))
        np.testing.assert_array_equal(_bits(one_h[0]), _bits(got_h[b]))
        np.testing.assert_array_equal(st[0], status[b])


def test_what_stays_refused(small, coded):
    latent, hyper, q, qh, mean = coded[(128, 192)]
    s = small.latents_to_bytes(latent[:1], hyper[:1], segment=5 * CELL)[0]
    g = small.latents_to_bytes(latent[:1], hyper[:1], segment=5 * CELL, hyper_groups=3)[0]
    plain = small.latents_to_bytes(latent[:1], hyper[:1])[0]
    lay, lg = pr.layout(s), pr.layout(g)
    cut = lay["ends"][2]
    for kw in ({}, {"partial": True}):
        with pytest.raises(_lib.CdcError, match="image 0: corrupt hyper stream"):
            small.decompress_from_bytes([_flip(s, lay["hdr"] + 17)], **kw)
        with pytest.raises(_lib.CdcError, match=r"image 0, hyper group 1 \(channels 11 - 21\)"):
            small.decompress_from_bytes([_flip(g, lg["hdr"] + 8 + 36 + struct.unpack("<I", g[lg["hdr"] + 8: lg["hdr"] + 12])[0] + 17)], **kw)
        wrong = s[: lay["lat"] + 2] + struct.pack("<HH", 3, 2) + s[lay["lat"] + 6:]
        with pytest.raises(_lib.CdcError, match="do not tile"):
            small.decompress_from_bytes([wrong], **kw)
        with pytest.raises(_lib.CdcError, match="exceeds the decoder's limit"):
            small.decompress_from_bytes([s], max_image_hw=(64, 64), **kw)
        with pytest.raises(_lib.CdcError, match="other probability tables"):
            small.decompress_from_bytes([s[:18] + struct.pack("<I", struct.unpack("<I", s[18:22])[0] ^ 1) + s[22:]], **kw)
    # ... and of prefixes: the hyper part is always whole, so it is always checked
    with pytest.raises(_lib.CdcError, match="image 0: corrupt hyper stream"):
        small.decompress_from_bytes([_flip(s, lay["hdr"] + 17)[:cut]], partial=True)
    with pytest.raises(_lib.CdcError, match="do not tile"):
        small.decompress_from_bytes([wrong[:cut]], partial=True)
    with pytest.raises(_lib.CdcError, match="segment="):
        small.decompress_from_bytes([plain], partial=True)
    with pytest.raises(_lib.CdcError, match="not inside"):
        small.decompress_from_bytes([s[:cut]], partial=True, window=(0, 0, 9, 1))
    # the C-ABI itself names segment= for an unsegmented stream
    h = small._hyper_handle()
    offs = (ctypes.c_size_t * 2)(0, len(plain))
    out, st, med = np.empty((32, 8, 12), np.float32), np.zeros(6, np.uint8), small._median_vector()
    with pytest.raises(_lib.CdcError, match="segment= at the encoder"):
        _lib.check(h, _lib.lib().cdc_entropy_decode_partial(h, plain, offs, med.ctypes.data, 1, None, out.ctypes.data, None, st.ctypes.data, 0, None))
    np.testing.assert_array_equal(_bits(small.decompress_from_bytes([s])), _bits(q[:1]))     # the handle is as it was


def test_wave_scale_conceal_over_16384_positions():
    """The full compressor of test_full_compressor_four_segments_of_16384_symbols: cut after segment 1, segment 0 damaged, so that
    seg_conceal_kernel runs over 16 384 positions and 64 blocks of one pair."""
    from test_entropy import _full_compressor
    comp, _ = _full_compressor()
    x = synth.normal("img", (1, 3, 256, 256), seed=4, std=0.4)
    latent, hyper = comp.analysis(x)
    assert latent.shape == (1, 256, 16, 16)
    s = comp.latents_to_bytes(latent, hyper, segment=8 * comp.rate_map_cell)[0]
    q, qh = comp.decompress_from_bytes([s], return_hyper=True)
    mean = comp.hyper_decode(qh)[0]
    lay = pr.layout(s)
    assert (lay["ny"], lay["nx"]) == (2, 2) and 256 * 8 * 8 == 16384
    bad = _flip(s, lay["starts"][0] + 256 + 40)[: lay["ends"][1]]
    got, status = comp.decompress_from_bytes([bad], partial=True, return_status=True)
    want = np.uint8([[[DAMAGED, OK], [ABSENT, ABSENT]]])
    np.testing.assert_array_equal(status, want)
    np.testing.assert_array_equal(_bits(got), _bits(pr.conceal(q, mean, want, 8)))
    np.testing.assert_array_equal(_bits(got[0][:, :8, 8:]), _bits(q[0][:, :8, 8:]))
    np.testing.assert_array_equal(_bits(got[0][:, :8, :8]), _bits(mean[0][:, :8, :8]))


@pytest.mark.parametrize("as_uint8", [False, True])
@pytest.mark.parametrize("hw", [(128, 192), (125, 185), (125, 188), (1, 1)])
def test_segment_mask(small, hw, as_uint8):
    """An image that is its own frame, one that is not (W % 4 != 0: element stores; W % 4 == 0 with a cropped height), and one pixel;
    statuses of all three kinds; host memory and device memory."""
    import torch
    status = np.uint8([[[OK, ABSENT, DAMAGED], [DAMAGED, OK, OK]], [[ABSENT, OK, ABSENT], [OK, DAMAGED, OK]]])
    want = pr.mask(status, 5, CELL, hw[0], hw[1], as_uint8)
    assert want.any() and not want.all() or hw == (1, 1)
    got = small.segment_mask(status, 5, hw, as_uint8=as_uint8)
    assert got.shape == (2, 1) + hw and got.dtype == (np.uint8 if as_uint8 else np.float32)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    dev = small.segment_mask(status, 5, hw, as_uint8=as_uint8, like=torch.empty(0, device="cuda"))
    assert dev.is_cuda and dev.dtype == (torch.uint8 if as_uint8 else torch.float32)
    np.testing.assert_array_equal(_bits(dev), _bits(want))
    # segments of one position, one segment for everything
    one = small.segment_mask(np.uint8([[[OK]]]), 64, hw, as_uint8=as_uint8)
    assert (one == (255 if as_uint8 else 1)).all()
    with pytest.raises(_lib.CdcError, match="larger than"):
        small.segment_mask(status, 5, (161, 16))


def test_decompress_partial_is_the_plain_decode_of_the_concealed_latent():
    from test_gpu_anysize import _small
    diff, un, comp, _ = _small("x")
    G = diff.padded_size(1, 1)[0]
    H, W = 4 * G, 3 * G
    cell = comp.rate_map_cell
    img = synth.normal("partial_image", (1, 3, H, W), seed=33, std=0.5).clip(-1, 1).astype(np.float32)
    streams = diff.compress_to_bytes(img, segment=G)
    info = comp.stream_info(streams[0])
    assert (info["seg"], info["ny"], info["nx"]) == (G // cell, 4, 3)
    ends = comp.segment_ends(streams[0])
    half = [streams[0][: ends[5] + 3]]                              # the first two rows of segments, and a little of the next
    args = dict(sample_steps=5, seed=(3 << 33) + 17, gamma=0.8, eta=0.5)
    # the whole frame from the concealed latent: the plain path on that q_latent
    rec, got = diff.decompress(half, partial=True, **args)
    q_c, status = comp.decompress_from_bytes(half, partial=True, return_status=True)
    assert status.reshape(-1).tolist() == [OK] * 6 + [ABSENT] * 6
    np.testing.assert_array_equal(_bits(rec), _bits(diff.decompress(q_c, (1, 3, H, W), **args)))
    np.testing.assert_array_equal(got["segment_status"], status)
    assert got["present_region"] == (0, 0, 2 * G, W) and set(got) == {"segment_status", "present_mask", "present_region"}
    np.testing.assert_array_equal(_bits(got["present_mask"]), _bits(pr.mask(status, G // cell, cell, H, W)))
    # tiles: region="present" is the region tuple it names, and costs fewer tiles
    tile = dict(tile=2 * G, tile_overlap=G)
    a, ia = diff.decompress(half, partial=True, region="present", as_uint8=True, **tile, **args)
    b, ib = diff.decompress(half, partial=True, region=ia["present_region"], as_uint8=True, **tile, **args)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert a.shape == (1, 3, 2 * G, W) and a.dtype == np.uint8 and ia["present_mask"].dtype == np.uint8
    assert ia["tiles"] == 6 and ia["tiles_decoded"] == 4 and ia["region"] == ia["present_region"] == (0, 0, 2 * G, W)
    assert ia["segments"] == 12 and ia["segments_decoded"] == 6
    for k in ("tiles", "tiles_decoded", "region", "present_region", "segments", "segments_decoded"):
        assert ia[k] == ib[k]
    np.testing.assert_array_equal(ia["segment_status"], ib["segment_status"])
    with pytest.raises(_lib.CdcError, match="no segment of these streams is complete"):
        diff.decompress([streams[0][: info["floor"] + 10]], partial=True, region="present", **tile, **args)
    # the full stream: partial=True is the plain decode
    rec, got = diff.decompress(streams, partial=True, **args)
    np.testing.assert_array_equal(_bits(rec), _bits(diff.decompress(streams, **args)))
    assert not got["segment_status"].any() and got["present_region"] == (0, 0, H, W) and (got["present_mask"] == 1).all()
