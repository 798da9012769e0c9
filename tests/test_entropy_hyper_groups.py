"""Grouped hyper part (container versions 19 - 22), the parts that need no GPU: the handle-free peeks against streams built in Python
from oracle sections (tests/hyper_groups_ref.py is the restatement of the format), the container's overhead derived from the section
bound, and the argument rules of hyper_groups=."""
import ctypes
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, compressor, synth
from oracle import entropy as oe
import hyper_groups_ref as hr
import segments_ref as sr

L = _lib.lib()
C = 32                                                             # channels of the small compressor's latent and hyper-latent
HH, WH = 2, 3                                                      # the hyper grid: per = 6 symbols a channel
SEG = 5                                                            # the latent 8 x 12 in 2 x 3 segments
VERSIONS = ((3, {}), (4, {"rate": 0.5}), (5, {"size": (120, 190)}), (6, {"rate": 0.25, "size": (127, 192)}))


def _peeks(s):
    """(rcs of the five peeks, (seg, ny, nx), (cg, ng))"""
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    f = ctypes.c_float()
    seg, ny, nx = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    cg, ng = ctypes.c_int(-1), ctypes.c_int(-1)
    rcs = (L.cdc_entropy_peek(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
           L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(a), ctypes.byref(f)),
           L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
           L.cdc_entropy_peek_segments(s, len(s), ctypes.byref(seg), ctypes.byref(ny), ctypes.byref(nx)),
           L.cdc_entropy_peek_hyper_groups(s, len(s), ctypes.byref(cg), ctypes.byref(ng)))
    return rcs, (seg.value, ny.value, nx.value), (cg.value, ng.value)


OK = (0, 0, 0, 0, 0)


def _refused(s):
    return all(rc == -1 for rc in _peeks(bytes(s))[0])


def _symbols(seed=0):
    """Synthetic hyper symbols [C, 2, 3] (escapes in channels 3 and 20 only), latent symbols and scales [C, 8, 12]."""
    rng = np.random.default_rng(seed)
    sym_h = np.rint(rng.standard_normal((C, HH, WH)) * 3).astype(np.int32)
    sym_h[3, 1, 2], sym_h[20, 0, 0] = 70000, -5000
    scale = np.exp(rng.uniform(np.log(0.1), np.log(30.0), (C, 4 * HH, 4 * WH))).astype(np.float32)
    sym_l = np.rint(rng.standard_normal(scale.shape) * scale).astype(np.int32)
    sym_l.reshape(-1)[::211] = rng.integers(-100000, 100000, sym_l.reshape(-1)[::211].shape)
    return sym_h, sym_l, scale


@pytest.fixture(scope="module")
def model():
    prior = oe.raw_prior(sr.prior_sd(C, seed=7), C)
    med = synth.normal("med", (C,), 3, 0.3).astype(np.float32)
    return prior, med


@pytest.mark.parametrize("cg,ng,sizes", [(1, 32, [6] * 32), (5, 7, [30] * 6 + [12]), (11, 3, [66, 66, 60]), (32, 1, [192])])
def test_peek_reads_good_streams(model, cg, ng, sizes):
    prior, med = model
    sym_h, sym_l, scale = _symbols()
    assert [(c1 - c0) * HH * WH for c0, c1 in hr.groups(C, cg)] == sizes      # fewer than a wave; ragged; an iteration and two lanes; one group
    for version, kw in VERSIONS:
        s = hr.oracle_stream(sym_h, sym_l, scale, prior, med, SEG, cg, version=version, **kw)
        assert s[3] == version + 16
        assert _peeks(s) == (OK, (SEG, 2, 3), (cg, ng)), (version, _peeks(s))
        assert cdc.ResnetCompressor.hyper_groups_of([s]) == [(cg, ng)] and cdc.ResnetCompressor.segments_of([s]) == [(SEG, 2, 3)]
        # the fields of the base version read as they always did
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        f = ctypes.c_float()
        assert L.cdc_entropy_peek(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and (a.value, b.value, c.value) == (HH, WH, 1)
        assert L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(a), ctypes.byref(f)) == 0 and a.value == (version in (4, 6))
        assert not a.value or f.value == kw["rate"]
        assert L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and a.value == (version in (5, 6))
        assert not a.value or (b.value, c.value) == kw["size"]
        # the latent part is that of the version-11 .. -14 stream, byte for byte; so is the fixed header but for the version byte
        base = sr.oracle_stream(sym_h, sym_l, scale, prior, med, SEG, version=version, **kw)
        nbl = struct.unpack("<I", s[14:18])[0]
        hdr = 34 + (4 if version in (4, 6) else 0) + (8 if version in (5, 6) else 0)
        assert s[-nbl:] == base[-nbl:] and s[4:10] == base[4:10] and s[14:26] == base[14:26] and s[30:hdr] == base[30:hdr]
        assert s[26:30] == base[26:30]                                            # esc_hyper: the sum over the groups


@pytest.mark.parametrize("version", [3, 4, 5, 6])
def test_unchanged_streams_peek_as_one_section(model, version):
    prior, med = model
    sym_h, sym_l, scale = _symbols()
    kw = dict(VERSIONS)[version]
    plain = sr.oracle_stream(sym_h, sym_l, scale, prior, med, 0, version=version, **kw)
    cut = sr.oracle_stream(sym_h, sym_l, scale, prior, med, SEG, version=version, **kw)
    assert plain[3] == version and _peeks(plain) == (OK, (0, 1, 1), (0, 1))
    assert cut[3] == version + 8 and _peeks(cut) == (OK, (SEG, 2, 3), (0, 1))
    assert cdc.ResnetCompressor.hyper_groups_of([plain, cut]) == [(0, 1)] * 2


@pytest.mark.parametrize("version", [3, 4, 5, 6])
def test_peek_refusals(model, version):
    prior, med = model
    cg, ng = 5, 7
    sym_h, sym_l, scale = _symbols(seed=1)
    kw = dict(VERSIONS)[version]
    s = hr.oracle_stream(sym_h, sym_l, scale, prior, med, SEG, cg, version=version, **kw)
    assert _peeks(s)[0] == OK
    hdr = 34 + (4 if version in (4, 6) else 0) + (8 if version in (5, 6) else 0)
    nbh, nbl, eh = struct.unpack("<I", s[10:14])[0], struct.unpack("<I", s[14:18])[0], struct.unpack("<I", s[26:30])[0]
    entries = [struct.unpack("<III", s[hdr + 8 + 12 * i: hdr + 20 + 12 * i]) for i in range(ng)]
    assert hdr + nbh + nbl == len(s) and sum(e[1] for e in entries) == eh and 8 + 12 * ng + sum(e[0] for e in entries) == nbh
    assert entries[0][1] >= 1 and entries[4][1] >= 1 and any(e[1] == 0 for e in entries)       # groups with and without escapes
    # truncation at every field boundary of the hyper part: the 8 bytes, every index entry, every group
    cuts = [hdr, hdr + 2, hdr + 4, hdr + 8]
    cuts += [hdr + 8 + 12 * i + d for i in range(ng) for d in (4, 8, 12)]
    at = hdr + 8 + 12 * ng
    for e in entries:
        at += e[0]
        cuts.append(at)
    assert at == hdr + nbh
    for cut in sorted(set(cuts)):
        assert cut < len(s) and _refused(s[:cut]), cut
    assert _refused(s + b"\0")                                     # ... and a byte too many

    def patched(at, fmt, *v):
        b = bytearray(s)
        b[at: at + struct.calcsize(fmt)] = struct.pack(fmt, *v)
        return b

    assert _refused(patched(hdr, "<H", 0))                         # cg = 0
    assert _refused(patched(hdr + 2, "<H", 0))                     # ng = 0
    assert _refused(patched(hdr + 4, "<I", 1)) and _refused(patched(hdr + 4, "<I", 1 << 31))     # reserved != 0
    assert _refused(patched(hdr + 2, "<H", ng + 1)) and _refused(patched(hdr + 2, "<H", ng - 1))   # the sums no longer hold
    for i in (0, ng - 1):                                          # a size off by one
        assert _refused(patched(hdr + 8 + 12 * i, "<I", entries[i][0] + 1)) and _refused(patched(hdr + 8 + 12 * i, "<I", entries[i][0] - 1))
    assert _refused(patched(10, "<I", nbh + 1)) and _refused(patched(10, "<I", nbh - 1))
    assert _refused(patched(hdr + 8 + 4, "<I", entries[0][1] - 1))                   # sum esc != esc_hyper
    assert _refused(patched(hdr + 8 + 12 + 4, "<I", 1))
    assert _refused(patched(26, "<I", eh + 1))
    # bytes < 256 + 4 esc, the sums kept right: entry 0 shrinks to 255 + 4 esc, entry 1 takes its bytes
    b0 = 255 + 4 * entries[0][1]
    bad = patched(hdr + 8, "<I", b0)
    bad[hdr + 20: hdr + 24] = struct.pack("<I", entries[1][0] + entries[0][0] - b0)
    assert _refused(bad)
    # the version bytes between and around the families stay no stream
    for v in (15, 16, 17, 18, 23, 24, 27):
        assert _refused(s[:3] + bytes([v]) + s[4:])
    # cg and ng against the channel count need the handle, a checksum the symbols: both are the decoder's
    assert _peeks(bytes(patched(hdr, "<H", 6)))[2] == (6, ng)
    assert _peeks(bytes(patched(hdr + 8 + 8, "<I", entries[0][2] ^ 1)))[0] == OK
    # the latent index is still validated by every peek
    lat = hdr + nbh
    assert _refused(patched(lat + 6, "<H", 1)) and _refused(patched(lat, "<H", 0))


def test_overhead_is_the_index_and_one_section_slack_per_group(model):
    """Every section ends within 64 * 32 + 64 bits = 264 bytes above its symbols' ideal code length and never below it (the section
    bound; tests/test_entropy_segments.py asserts it against the oracle's ideal bits).  Ideal bits add up over groups, so with
    whole = ideal / 8 + a, 0 <= a <= 264, and group g = ideal_g / 8 + a_g, 0 <= a_g <= 264, a hyper part of ng groups is
    8 + 12 ng + sum a_g - a bytes larger than the one section: between 8 + 12 ng - 264 and 8 + 276 ng.  One group is the one section
    behind 20 bytes."""
    prior, med = model
    rng = np.random.default_rng(3)
    sym = np.rint(rng.standard_normal((C, 16, 16)) * 4).astype(np.int32)                 # 256 symbols a channel, as a 256 x 256 image's
    sym.reshape(-1)[::501] = rng.integers(-100000, 100000, sym.reshape(-1)[::501].shape)
    whole, esc = oe.encode_hyper(sym, prior, med)
    for cg in (32, 16, 11, 5, 2, 1):
        part, ne, _, entries = hr.hyper_part(sym, prior, med, cg)
        ng = len(entries)
        assert ng == -(-C // cg) and ne == esc
        over = len(part) - len(whole)
        print(f"cg {cg}: {ng} groups, {len(part)} bytes against {len(whole)}: +{over} ({over / ng:.0f} a group)")
        assert 8 + 12 * ng - 264 <= over <= 8 + 276 * ng, (cg, over)
        if ng == 1:
            assert over == 20 and part[20:] == whole
        at = 8 + 12 * ng
        for (c0, c1), e in zip(hr.groups(C, cg), entries):           # each group decodes as the oracle's section of its channels
            got = oe.decode_hyper(part[at: at + e[0]], e[1], c1 - c0, 256, prior[c0:c1], med[c0:c1])
            assert got.tolist() == sym[c0:c1].reshape(-1).tolist()
            at += e[0]
        assert at == len(part)


def _small():
    return cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=8)


@pytest.mark.parametrize("groups,segment", [(4, None), (0, 64), (33, 64), (-1, 64), (True, 64), (4.0, 64), ("4", 64)])
def test_hyper_groups_argument_rules(groups, segment, monkeypatch):
    """hyper_groups= is the number of groups, an int in 1 .. Ch, and needs segment=: refused before the library is touched."""
    comp = _small()
    assert comp.reversed_hyper_dims[0] == C
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    x = np.zeros((1, 3, 64, 64), np.float32)
    for call in (lambda: comp.compress_to_bytes(x, segment=segment, hyper_groups=groups), lambda: comp.encode(x, segment=segment, hyper_groups=groups),
                 lambda: comp.latents_to_bytes(np.zeros((1, 32, 4, 4), np.float32), np.zeros((1, 32, 1, 1), np.float32), segment=segment,
                                               hyper_groups=groups)):
        with pytest.raises(ValueError, match="hyper_groups"):
            call()
    from cdc_compression_amd import diffusion
    model = object.__new__(diffusion.GaussianDiffusionX)
    model.context_fn = comp
    for call in (lambda: model.compress(x, segment=segment, hyper_groups=groups), lambda: model.compress_to_bytes(x, segment=segment, hyper_groups=groups),
                 lambda: model.compress_best_of(x, 2, seed=1, gamma=0.8, segment=segment, hyper_groups=groups)):
        with pytest.raises(ValueError, match="hyper_groups"):
            call()
    model.context_fn = lambda images: {"output": [images], "bpp": 0.0}           # no stream to cut
    with pytest.raises(ValueError, match="hyper_groups"):
        model.compress_to_bytes(x, segment=None, hyper_groups=4)


def test_groups_asked_for_and_groups_written():
    """cg = ceil(Ch / G); the stream then holds ceil(Ch / cg) groups, which can be fewer than G."""
    got = {G: compressor.hyper_group_channels(G, C, 64) for G in (1, 2, 3, 7, 12, 16, 20, 32)}
    assert got == {1: 32, 2: 16, 3: 11, 7: 5, 12: 3, 16: 2, 20: 2, 32: 1}
    assert [-(-C // got[G]) for G in (3, 7, 12, 20)] == [3, 7, 11, 16]
    assert compressor.hyper_group_channels(None, C, None) == 0 and compressor.hyper_group_channels(None, C, 64) == 0


def test_header_bytes_count_the_hyper_index():
    comp = _small()
    x = np.zeros((1, 3, 128, 192), np.float32)
    assert comp._stream_header_bytes(x, (128, 192), 128) == 34 + 8 + 12 * 2
    assert comp._stream_header_bytes(x, (128, 192), 128, 32) == 34 + 8 + 12 * 2 + 8 + 12 * 32
    assert comp._stream_header_bytes(x, (120, 190), 80, 7) == 34 + 8 + 8 + 12 * 6 + 8 + 12 * 7
    assert comp._stream_header_bytes(x, (128, 192), 16, 1) == 34 + 8 + 12 * 96 + 8 + 12
