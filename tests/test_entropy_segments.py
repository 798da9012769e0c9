"""Segmented streams (container versions 11 - 14), the parts that need no GPU: the handle-free peeks against streams built in
Python from oracle sections (tests/segments_ref.py is the restatement of the format), the container's overhead derived from the
section bound, and the argument rules of segment=."""
import ctypes
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, compressor, synth
from oracle import entropy as oe
import segments_ref as sr

L = _lib.lib()
C = 32                                                             # channels of the small compressor's latent and hyper-latent


def _peeks(s):
    """(rc of cdc_entropy_peek, of _peek_bitrate_scale, of _peek_image_size, of _peek_segments, (seg, ny, nx))"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    f = ctypes.c_float()
    seg, ny, nx = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rcs = (L.cdc_entropy_peek(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
           L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(a), ctypes.byref(f)),
           L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
           L.cdc_entropy_peek_segments(s, len(s), ctypes.byref(seg), ctypes.byref(ny), ctypes.byref(nx)))
    return rcs, (seg.value, ny.value, nx.value)


def _refused(s):
    rcs, _ = _peeks(bytes(s))
    return all(rc == -1 for rc in rcs)


def _symbols(Hl, Wl, seed=0):
    """Synthetic hyper symbols [C, Hl / 4, Wl / 4], latent symbols and scales [C, Hl, Wl] (a few escapes among them)."""
    rng = np.random.default_rng(seed)
    sym_h = np.rint(rng.standard_normal((C, Hl // 4, Wl // 4)) * 4).astype(np.int32)
    scale = np.exp(rng.uniform(np.log(0.1), np.log(30.0), (C, Hl, Wl))).astype(np.float32)
    sym_l = np.rint(rng.standard_normal((C, Hl, Wl)) * scale).astype(np.int32)
    sym_l.reshape(-1)[::211] = rng.integers(-100000, 100000, sym_l.reshape(-1)[::211].shape)
    return sym_h, sym_l, scale


@pytest.fixture(scope="module")
def model():
    prior = oe.raw_prior(sr.prior_sd(C, seed=7), C)
    med = synth.normal("med", (C,), 3, 0.3).astype(np.float32)
    return prior, med


@pytest.mark.parametrize("Hl,Wl,seg,grid", [(8, 12, 8, (1, 2)), (8, 12, 5, (2, 3)), (4, 4, 1, (4, 4)), (8, 12, 64, (1, 1))])
def test_peek_reads_good_streams(model, Hl, Wl, seg, grid):
    prior, med = model
    sym_h, sym_l, scale = _symbols(Hl, Wl)
    for version, kw in ((3, {}), (4, {"rate": 0.5}), (5, {"size": (Hl * 16 - 3, Wl * 16 - 7)}), (6, {"rate": 0.25, "size": (Hl * 16 - 1, Wl * 16)})):
        s = sr.oracle_stream(sym_h, sym_l, scale, prior, med, seg, version=version, **kw)
        assert s[3] == version + 8
        rcs, got = _peeks(s)
        assert rcs == (0, 0, 0, 0) and got == (seg,) + grid, (version, rcs, got)
        assert cdc.ResnetCompressor.segments_of([s]) == [(seg,) + grid]
        plain = sr.oracle_stream(sym_h, sym_l, scale, prior, med, 0, version=version, **kw)
        assert plain[3] == version and _peeks(plain) == ((0, 0, 0, 0), (0, 1, 1))
        # the fields of the base version read as they always did
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        f = ctypes.c_float()
        assert L.cdc_entropy_peek(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and (a.value, b.value, c.value) == (Hl // 4, Wl // 4, 1)
        assert L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(a), ctypes.byref(f)) == 0 and a.value == (version in (4, 6))
        assert not a.value or f.value == kw["rate"]
        assert L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and a.value == (version in (5, 6))
        assert not a.value or (b.value, c.value) == kw["size"]
    # the ragged edges are where the specification puts them
    wins, _ = sr.windows(Hl, Wl, seg)
    if (Hl, Wl, seg) == (8, 12, 5):
        assert [y1 - y0 for y0, y1, _, _ in wins[::3]] == [5, 3] and [x1 - x0 for _, _, x0, x1 in wins[:3]] == [5, 5, 2]
    if seg == 1:
        assert len(wins) == 16 and all((y1 - y0) * (x1 - x0) * C == 32 for y0, y1, x0, x1 in wins)    # fewer symbols than lanes


@pytest.mark.parametrize("version", [3, 4, 5, 6])
def test_peek_refusals(model, version):
    prior, med = model
    Hl, Wl, seg = 8, 12, 5
    sym_h, sym_l, scale = _symbols(Hl, Wl, seed=1)
    kw = {3: {}, 4: {"rate": 0.5}, 5: {"size": (120, 190)}, 6: {"rate": 0.5, "size": (120, 190)}}[version]
    s = sr.oracle_stream(sym_h, sym_l, scale, prior, med, seg, version=version, **kw)
    assert _peeks(s)[0] == (0, 0, 0, 0)
    hdr = 34 + (4 if version in (4, 6) else 0) + (8 if version in (5, 6) else 0)
    nbh, nbl, el = struct.unpack("<I", s[10:14])[0], struct.unpack("<I", s[14:18])[0], struct.unpack("<I", s[30:34])[0]
    lat = hdr + nbh                                                # where the latent part starts
    n_seg = 6
    entries = [struct.unpack("<III", s[lat + 8 + 12 * i: lat + 20 + 12 * i]) for i in range(n_seg)]
    assert hdr + nbh + nbl == len(s) and sum(e[1] for e in entries) == el
    # truncation at every field boundary: of the header, the 8 bytes, every index entry, every segment
    cuts = [3, 4, 5, 6, 8, 10, 14, 18, 22, 26, 30, 34, hdr, lat, lat + 2, lat + 4, lat + 6, lat + 8]
    cuts += [lat + 8 + 12 * i + d for i in range(n_seg) for d in (4, 8, 12)]
    at = lat + 8 + 12 * n_seg
    for e in entries:
        at += e[0]
        cuts += [at - 1] if at == len(s) else [at]
    for cut in sorted(set(cuts)):
        assert cut < len(s) and _refused(s[:cut]), cut
    assert _refused(s + b"\0")                                     # ... and a byte too many

    def patched(at, fmt, *v):
        b = bytearray(s)
        b[at: at + struct.calcsize(fmt)] = struct.pack(fmt, *v)
        return b

    assert _refused(patched(lat, "<H", 0))                         # seg = 0
    assert _refused(patched(lat + 2, "<H", 0)) and _refused(patched(lat + 4, "<H", 0))        # ny nx = 0
    assert _refused(patched(lat + 2, "<HH", 256, 256))             # ny nx = 65536 > 65535
    assert _refused(patched(lat + 6, "<H", 1))                     # reserved != 0
    for i in (0, n_seg - 1):
        assert _refused(patched(lat + 8 + 12 * i, "<I", entries[i][0] + 1)) and _refused(patched(lat + 8 + 12 * i, "<I", entries[i][0] - 1))
    i = next(i for i, e in enumerate(entries) if e[1] > 0)         # a segment with escapes
    assert _refused(patched(lat + 8 + 12 * i + 4, "<I", entries[i][1] - 1))                   # sum esc != esc_latent
    assert _refused(patched(30, "<I", el + 1))
    # bytes < 256 + 4 esc, the sums kept right: entry 0 shrinks to 255 + 4 esc, entry 1 takes its bytes
    b0 = 255 + 4 * entries[0][1]
    bad = patched(lat + 8, "<I", b0)
    bad[lat + 20: lat + 24] = struct.pack("<I", entries[1][0] + entries[0][0] - b0)
    assert _refused(bad)
    # the version bytes between and around the two families stay no stream
    for v in (7, 8, 9, 10, 15):
        assert _refused(s[:3] + bytes([v]) + s[4:])
    assert _peeks(bytes(patched(lat + 8 + 8, "<I", entries[0][2] ^ 1)))[0] == (0, 0, 0, 0)          # a checksum needs the symbols: the decoder's


def test_a_65535_segment_index_is_accepted_and_one_more_is_not():
    """ny nx <= 65535 is the limit itself: an index of 255 x 257 empty sections (256 bytes of lane states each) reads, 256 x 256 does not."""
    def empty(ny, nx):
        n = ny * nx
        part = struct.pack("<HHHH", 1, ny, nx, 0) + struct.pack("<III", 256, 0, 0) * n + bytes(256 * n)
        return sr.stream(3, 1, 1, 1, (bytes(256), 0), part, 0, 0, 0)
    assert _peeks(empty(255, 257)) == ((0, 0, 0, 0), (1, 255, 257))
    assert _refused(empty(256, 256))


def test_overhead_is_the_index_and_one_section_slack_per_segment():
    """The section bound 0 <= 8 len - ideal_bits <= 64 * 32 + 64 (64 lane states of 32 bits and a bit of slack each) holds for the
    oracle on every segment; ideal bits add up over segments, so a latent part of n segments is between 8 + 12 n - 264 and
    8 + n (12 + 264) bytes larger than the one section of the same symbols."""
    rng = np.random.default_rng(2)                                 # the inputs of test_code_length_tracks_the_gaussian_rate_estimate
    n = 60000
    scale = np.exp(rng.uniform(np.log(0.3), np.log(20.0), n)).astype(np.float32)
    sym = np.rint(rng.standard_normal(n) * scale).astype(np.int32)
    sym, scale = sym.reshape(32, 25, 75), scale.reshape(32, 25, 75)
    slack = 64 * 32 + 64
    whole = len(oe.encode_latent(sym, scale)[0])
    assert 0 <= 8 * whole - oe.ideal_bits_latent(sym, scale) <= slack
    for seg in (25, 16, 8, 5):
        wins, (ny, nx) = sr.windows(25, 75, seg)
        part, _, _, entries = sr.latent_part(sym, scale, seg)
        for (y0, y1, x0, x1), e in zip(wins, entries):
            ideal = oe.ideal_bits_latent(sym[:, y0:y1, x0:x1], scale[:, y0:y1, x0:x1])
            assert 0 <= 8 * e[0] - ideal <= slack, (seg, (y0, x0), 8 * e[0] - ideal)
        k = ny * nx
        assert 8 + 12 * k - 264 <= len(part) - whole <= 8 + k * (12 + 264), (seg, len(part) - whole)


def _small():
    return cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=8)


@pytest.mark.parametrize("segment", [24, 8, -16, 0, 16.0, True])
def test_segment_argument_rules(segment, monkeypatch):
    """segment= is image pixels, a positive int multiple of the 16 pixels of a latent position: refused before the library is touched."""
    comp = _small()
    assert comp.rate_map_cell == 16
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    x = np.zeros((1, 3, 64, 64), np.float32)
    for call in (lambda: comp.compress_to_bytes(x, segment=segment), lambda: comp.encode(x, segment=segment),
                 lambda: comp.latents_to_bytes(np.zeros((1, 32, 4, 4), np.float32), np.zeros((1, 32, 1, 1), np.float32), segment=segment)):
        with pytest.raises(ValueError, match="segment"):
            call()
    assert compressor.segment_positions(None, 16) == 0 and compressor.segment_positions(128, 16) == 8


def test_segment_needs_a_stream_not_a_context_pyramid(monkeypatch):
    """A context_fn that only returns a context pyramid writes no stream: segment= on the diffusion model's entry points is refused
    before anything runs; with this package's compressor the same argument rule applies as on the compressor."""
    from cdc_compression_amd import diffusion
    x = np.zeros((1, 3, 64, 64), np.float32)
    for ctx, segment in ((lambda images: {"output": [images], "bpp": 0.0}, 64), (_small(), 24), (_small(), -64)):
        model = object.__new__(diffusion.GaussianDiffusionX)
        model.context_fn = ctx
        monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
        for call in (lambda: model.compress(x, segment=segment), lambda: model.compress_to_bytes(x, segment=segment),
                     lambda: model.compress_best_of(x, 2, seed=1, gamma=0.8, segment=segment)):
            with pytest.raises(ValueError, match="segment"):
                call()


def test_header_bytes_count_the_index():
    comp = _small()
    x = np.zeros((1, 3, 128, 192), np.float32)
    assert comp._stream_header_bytes(x, (128, 192)) == 34
    assert comp._stream_header_bytes(x, (128, 192), 128) == 34 + 8 + 12 * 2
    assert comp._stream_header_bytes(x, (120, 190), 80) == 34 + 8 + 8 + 12 * 6
    assert comp._stream_header_bytes(x, (128, 192), 16) == 34 + 8 + 12 * 96
