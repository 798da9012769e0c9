"""Partial streams, the parts that need no GPU: cdc_entropy_peek_partial at EVERY byte length of Python-built streams (oracle sections;
tests/segments_ref.py and tests/hyper_groups_ref.py build them) against the arithmetic of tests/partial_ref.py, its agreement with the
other peeks at full length, every refusal, segment_ends, and the argument rules of the Python layer and of the C-ABI."""
import ctypes
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from oracle import entropy as oe
import hyper_groups_ref as hg
import partial_ref as pr
import segments_ref as sr

L = _lib.lib()
C = 32
SHAPES = [(8, 12, 8), (8, 12, 5), (8, 12, 64), (4, 4, 1)]              # latent Hl x Wl and seg: those of test_entropy_segments.py
KW = {3: {}, 4: {"rate": 0.5}, 5: {"size": None}, 6: {"rate": 0.25, "size": None}}


def _symbols(Hl, Wl, seed=0):
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


def _kw(base, Hl, Wl):
    kw = dict(KW[base])
    if "size" in kw:
        kw["size"] = (Hl * 16 - 3, Wl * 16 - 7)
    return kw


def _stream(model, Hl, Wl, seg, version, seed=0):
    """The stream of container version `version` (11 - 14: segmented; 19 - 22: also grouped, 12 hyper channels per group)."""
    prior, med = model
    sym_h, sym_l, scale = _symbols(Hl, Wl, seed)
    if version >= 19:
        return hg.oracle_stream(sym_h, sym_l, scale, prior, med, seg, 12, version=version - 16, **_kw(version - 16, Hl, Wl))
    return sr.oracle_stream(sym_h, sym_l, scale, prior, med, seg, version=version - 8, **_kw(version - 8, Hl, Wl))


def _peek(s, n=None):
    """(rc, StreamInfo) of the first n bytes"""
    info = _lib.StreamInfo()
    s = bytes(s)
    return L.cdc_entropy_peek_partial(s, len(s) if n is None else n, ctypes.byref(info)), info


def _refused(s, n=None):
    return _peek(s, n)[0] == -1


@pytest.mark.parametrize("version", [11, 12, 13, 14, 19, 20, 21, 22])
@pytest.mark.parametrize("Hl,Wl,seg", SHAPES)
def test_peek_partial_at_every_byte_length(model, Hl, Wl, seg, version):
    s = _stream(model, Hl, Wl, seg, version)
    lay = pr.layout(s)
    assert lay["declared"] == len(s) and s[3] == version
    padded = s + b"\0" * 4                                          # (the call reads n bytes: a length beyond the stream needs bytes to read)
    seen = set()
    for n in range(0, lay["declared"] + 2):
        rc, info = _peek(padded, n)
        want = pr.peek(s, n)
        if want is None:
            assert rc == -1, n
            continue
        assert rc == 0, n
        assert (info.floor, info.declared, info.complete) == want, n
        assert (info.seg, info.ny, info.nx, info.cg, info.ng) == (lay["seg"], lay["ny"], lay["nx"], lay["cg"], lay["ng"]), n
        assert (info.hh, info.wh, info.arith) == (Hl // 4, Wl // 4, 1)
        seen.add(info.complete)
    assert seen == set(range(lay["ny"] * lay["nx"] + 1))              # every count from nothing to everything was met
    assert pr.peek(s, lay["floor"] - 1) is None and pr.peek(s, lay["floor"])[2] == 0


@pytest.mark.parametrize("version", [11, 12, 13, 14, 19, 20, 21, 22])
def test_full_length_agrees_with_the_other_peeks_and_the_python_layer(model, version):
    Hl, Wl, seg = 8, 12, 5
    s = _stream(model, Hl, Wl, seg, version)
    rc, info = _peek(s)
    assert rc == 0
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    f = ctypes.c_float()
    assert L.cdc_entropy_peek(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert (info.hh, info.wh, info.arith) == (a.value, b.value, c.value)
    assert L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(a), ctypes.byref(f)) == 0
    assert info.has_rate == a.value and (not a.value or info.rate == f.value)
    assert L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert info.has_size == a.value and (not a.value or (info.img_h, info.img_w) == (b.value, c.value))
    assert L.cdc_entropy_peek_segments(s, len(s), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert (info.seg, info.ny, info.nx) == (a.value, b.value, c.value) == (5, 2, 3)
    assert L.cdc_entropy_peek_hyper_groups(s, len(s), ctypes.byref(a), ctypes.byref(b)) == 0
    assert (info.cg, info.ng) == (a.value, b.value) == ((12, 3) if version >= 19 else (0, 1))
    assert info.declared == len(s) and info.complete == 6
    # the Python layer: the dict, the ends, and the helpers that keep refusing prefixes
    comp = cdc.ResnetCompressor
    d = comp.stream_info(s)
    lay = pr.layout(s)
    assert d["floor"] == lay["floor"] and d["declared"] == len(s) and d["complete"] == 6 and d["has_rate"] == (version % 8 in (4, 6))
    assert comp.segment_ends(s) == lay["ends"] and comp.segment_ends(s[: lay["floor"]]) == lay["ends"]
    cut = lay["ends"][2] + 1
    assert comp.stream_info(s[:cut])["complete"] == 3
    for helper in (comp.segments_of, comp.hyper_groups_of, comp.image_size_of):
        with pytest.raises(_lib.CdcError, match="not a CDC bitstream"):
            helper([s[:cut]])
    with pytest.raises(_lib.CdcError, match="segment index"):
        comp.stream_info(s[: lay["floor"] - 1])
    with pytest.raises(_lib.CdcError, match="segment index"):
        comp.segment_ends(s[: lay["floor"] - 1])


@pytest.mark.parametrize("base", [3, 4, 5, 6])
def test_refusals(model, base):
    prior, med = model
    Hl, Wl, seg = 8, 12, 5
    s = _stream(model, Hl, Wl, seg, base + 8, seed=1)
    g = _stream(model, Hl, Wl, seg, base + 16, seed=1)
    for t in (s, g):
        lay = pr.layout(t)
        assert not _refused(t) and not _refused(t, lay["floor"])
        assert _refused(t, lay["floor"] - 1) and _refused(t + b"\0") and _refused(t, 0) and _refused(t, 33)
        # the version bytes that are no partial-decodable stream: unsegmented, between the families, beyond
        for v in (base, 7, 8, 9, 10, 15, 16, 17, 18, 23, 24, 27):
            assert _refused(t[:3] + bytes([v]) + t[4:]), v
    sym_h, sym_l, scale = _symbols(Hl, Wl, seed=1)
    plain = sr.oracle_stream(sym_h, sym_l, scale, prior, med, 0, version=base, **_kw(base, Hl, Wl))
    assert plain[3] == base and _refused(plain)
    with pytest.raises(_lib.CdcError, match="segment="):
        cdc.ResnetCompressor.stream_info(plain)
    assert L.cdc_entropy_peek_partial(None, 100, ctypes.byref(_lib.StreamInfo())) == -1 and L.cdc_entropy_peek_partial(s, len(s), None) == -1

    # every index corruption test_entropy_segments.py / test_entropy_hyper_groups.py refuse, on the whole stream and on a prefix
    lay = pr.layout(s)
    lat, entries, el, n_seg = lay["lat"], lay["entries"], struct.unpack("<I", s[30:34])[0], 6

    def patched(src, at, fmt, *v):
        b = bytearray(src)
        b[at: at + struct.calcsize(fmt)] = struct.pack(fmt, *v)
        return bytes(b)

    def refused_everywhere(bad, floor):
        return _refused(bad) and _refused(bad, floor) and _refused(bad, floor + 300)

    F = lay["floor"]
    assert refused_everywhere(patched(s, lat, "<H", 0), F)                                            # seg = 0
    assert refused_everywhere(patched(s, lat + 2, "<H", 0), F) and refused_everywhere(patched(s, lat + 4, "<H", 0), F)
    assert refused_everywhere(patched(s, lat + 2, "<HH", 256, 256), F)                                # ny nx = 65536
    assert refused_everywhere(patched(s, lat + 6, "<H", 1), F)                                        # reserved != 0
    for i in (0, n_seg - 1):
        for d in (1, -1):
            assert refused_everywhere(patched(s, lat + 8 + 12 * i, "<I", entries[i][0] + d), F)       # the sums no longer hold
    i = next(i for i, e in enumerate(entries) if e[1] > 0)
    assert refused_everywhere(patched(s, lat + 8 + 12 * i + 4, "<I", entries[i][1] - 1), F)           # sum esc != esc_latent
    assert refused_everywhere(patched(s, 30, "<I", el + 1), F)
    b0 = 255 + 4 * entries[0][1]                                     # bytes < 256 + 4 esc with the sums kept right
    bad = patched(patched(s, lat + 8, "<I", b0), lat + 20, "<I", entries[1][0] + entries[0][0] - b0)
    assert refused_everywhere(bad, F)
    assert not _refused(patched(s, lat + 8 + 8, "<I", entries[0][2] ^ 1))                             # a checksum needs the symbols: the decoder's
    if base in (5, 6):                                               # a recorded size of 0 or beyond 2^31 - 1 is no stream
        assert refused_everywhere(patched(s, lay["hdr"] - 8, "<I", 0), F) and refused_everywhere(patched(s, lay["hdr"] - 4, "<I", 1 << 31), F)
    # ... and of the hyper index
    lg = pr.layout(g)
    hdr, G = lg["hdr"], lg["floor"]
    ge = [struct.unpack("<III", g[hdr + 8 + 12 * k: hdr + 20 + 12 * k]) for k in range(lg["ng"])]
    assert refused_everywhere(patched(g, hdr, "<H", 0), G) and refused_everywhere(patched(g, hdr + 2, "<H", 0), G)
    assert refused_everywhere(patched(g, hdr + 4, "<I", 1), G)
    assert refused_everywhere(patched(g, hdr + 2, "<H", lg["ng"] + 1), G) and refused_everywhere(patched(g, hdr + 2, "<H", lg["ng"] - 1), G)
    for k in (0, lg["ng"] - 1):
        for d in (1, -1):
            assert refused_everywhere(patched(g, hdr + 8 + 12 * k, "<I", ge[k][0] + d), G)
    assert refused_everywhere(patched(g, 26, "<I", struct.unpack("<I", g[26:30])[0] + 1), G)
    b0 = 255 + 4 * ge[0][1]
    bad = patched(patched(g, hdr + 8, "<I", b0), hdr + 20, "<I", ge[1][0] + ge[0][0] - b0)
    assert refused_everywhere(bad, G)


def test_a_65535_segment_index_is_the_limit():
    def empty(ny, nx):
        n = ny * nx
        part = struct.pack("<HHHH", 1, ny, nx, 0) + struct.pack("<III", 256, 0, 0) * n + bytes(256 * n)
        s = sr.stream(3, 1, 1, 1, (bytes(256), 0), part, 0, 0, 0)
        return s, 34 + 256 + 8 + 12 * n
    s, floor = empty(255, 257)
    rc, info = _peek(s, floor + 256 * 1000 + 255)
    assert rc == 0 and (info.ny, info.nx, info.complete, info.floor) == (255, 257, 1000, floor)
    s, floor = empty(256, 256)
    assert _refused(s) and _refused(s, floor)


def _small():
    return cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=8)


def test_argument_rules_of_the_python_layer(model, monkeypatch):
    """Refused before the library is touched."""
    from cdc_compression_amd import diffusion
    comp = _small()
    s = _stream(model, 8, 12, 5, 11)
    m = object.__new__(diffusion.GaussianDiffusionX)
    m.context_fn = comp
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    with pytest.raises(ValueError, match="no price"):
        comp.decompress_from_bytes([s], partial=True, return_rate_map=True)
    with pytest.raises(ValueError, match="return_status belongs to partial"):
        comp.decompress_from_bytes([s], return_status=True)
    with pytest.raises(ValueError, match="status must be"):
        comp.segment_mask(np.zeros((2, 3), np.uint8), 5, (128, 192))
    for kw in (dict(samples=2, seed=1, gamma=0.8), dict(trajectory=[0]), dict(reduce="mean")):
        with pytest.raises(ValueError, match="excludes samples= and trajectory="):
            m.decompress([s], partial=True, **kw)
    with pytest.raises(ValueError, match="decodes streams"):
        m.decompress(np.zeros((1, 32, 8, 12), np.float32), partial=True)
    with pytest.raises(ValueError, match="their own bitrate_scale"):
        m.decompress([s], partial=True, bitrate_scale=0.5)
    with pytest.raises(ValueError, match="region"):
        m.decompress([s], partial=True, region="absent", tile=64)
    with pytest.raises(ValueError, match="region belongs to tile="):
        m.decompress([s], partial=True, region="present")
    with pytest.raises(ValueError, match="belongs to partial=True"):
        m.decompress([s], region="present", tile=64)


def test_c_abi_refusals_without_a_device():
    out = np.zeros(16, np.uint8)
    st = np.zeros(4, np.uint8)
    offs = (ctypes.c_size_t * 2)(0, 10)
    assert L.cdc_entropy_decode_partial(None, b"x" * 10, offs, out.ctypes.data, 1, None, out.ctypes.data, None, st.ctypes.data, 0, None) == -1
    assert L.cdc_segment_mask(None, st.ctypes.data, 1, 2, 2, 1, 1, 2, 2, out.ctypes.data, 1, 0, None) == -1
    comp = _small()
    h = comp._hyper_handle()
    for args, msg in (((None, 1, 2, 2, 1, 1, 2, 2, out.ctypes.data, 1, 0), "null/invalid"),
                      ((st.ctypes.data, 0, 2, 2, 1, 1, 2, 2, out.ctypes.data, 1, 0), "null/invalid"),
                      ((st.ctypes.data, 1, 256, 256, 1, 1, 2, 2, out.ctypes.data, 1, 0), "null/invalid"),
                      ((st.ctypes.data, 1, 2, 2, 0, 1, 2, 2, out.ctypes.data, 1, 0), "null/invalid"),
                      ((st.ctypes.data, 1, 2, 2, 1, 1, 3, 2, out.ctypes.data, 1, 0), "larger than"),
                      ((st.ctypes.data, 1, 2, 2, 1, 1, 2, 3, out.ctypes.data, 1, 0), "larger than"),
                      ((st.ctypes.data, 1, 2, 2, 1, 1, 2, 2, out.ctypes.data, 2, 0), "element kind"),
                      ((st.ctypes.data, 1, 2, 2, 1, 1, 2, 2, out.ctypes.data, 1, 7), "mem_kind")):
        with pytest.raises(_lib.CdcError, match=msg):
            _lib.check(h, L.cdc_segment_mask(h, *args, None))
    bad = np.uint8([0, 1, 2, 3])
    with pytest.raises(_lib.CdcError, match=r"status\[3\] = 3"):
        _lib.check(h, L.cdc_segment_mask(h, bad.ctypes.data, 1, 2, 2, 1, 1, 2, 2, out.ctypes.data, 1, 0, None))
    with pytest.raises(_lib.CdcError):                               # a null status table is no partial decode
        _lib.check(h, L.cdc_entropy_decode_partial(h, b"x" * 10, offs, out.ctypes.data, 1, None, out.ctypes.data, None, None, 0, None))


def test_partial_ref_is_consistent_with_itself():
    """The restatement's own pieces: the status of a prefix, the concealed latent, the mask."""
    st = np.uint8([[[0, 1, 2], [0, 0, 1]]])
    ok = pr.ok_positions(st[0], 5, 8, 12)
    assert ok.shape == (8, 12) and ok[:5, :5].all() and not ok[:5, 5:].any() and ok[5:, :10].all() and not ok[5:, 10:].any()
    full, mean = np.ones((1, 2, 8, 12), np.float32), np.zeros((1, 2, 8, 12), np.float32)
    got = pr.conceal(full, mean, st, 5)
    assert got.sum() == 2 * ok.sum()
    m = pr.mask(st, 5, 16, 125, 185)
    assert m.shape == (1, 1, 125, 185) and m[0, 0, 79, 79] == 1 and m[0, 0, 79, 80] == 0 and m[0, 0, 80, 159] == 1 and m[0, 0, 124, 160] == 0
    assert pr.mask(st, 5, 16, 125, 185, as_uint8=True).max() == 255
