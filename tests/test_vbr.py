"""Variable-bitrate context model (BigCompressor(vbr=True)): the host side -- manifests against the reference's state_dict
(tests/golden/make_golden_vbr.py), the order and argument rules of cdc_enable_vbr / cdc_set_bitrate_scale, the version-4 stream
header, and the Python front end's refusals.  No GPU needed."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from helpers import GOLDEN

L = _lib.lib()


def _meta(name):
    return json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))


def _man(m):
    return [(k, tuple(v)) for k, v in m]


@pytest.mark.parametrize("name", ["vbr_small", "vbr_full"])
def test_vbr_manifests_equal_the_reference_state_dict(name):
    meta = _meta(name)
    ref = _man(meta["manifest"])
    m = cdc.BigCompressor(vbr=True, **meta["kwargs"])
    assert _man(m.manifest()) == [e for e in ref if e[0].startswith("dec.")]
    assert _man(m.hyper_manifest()) == [e for e in ref if e[0].startswith("hyper_dec.")]
    assert _man(m.encoder_manifest()) == [e for e in ref if e[0].startswith(("enc.", "hyper_enc."))]
    # every VBRCondition site of the reference is somewhere
    sites = {k.rsplit(".", 2)[0] for k, _ in ref if synth.is_vbr_key(k)}
    n = len(meta["kwargs"]["dim_mults"]) * 2 + 2 * (len(meta["kwargs"]["hyper_dims_mults"]) - 1)
    assert len(sites) == n


def test_vbr_manifest_of_the_end_to_end_model():
    meta = _meta("vbr_e2e")
    ref = _man(meta["comp_manifest"])
    m = cdc.BigCompressor(vbr=True, **meta["comp_kwargs"])
    got = _man(m.manifest()) + _man(m.hyper_manifest()) + _man(m.encoder_manifest())
    assert sorted(got) == sorted(e for e in ref if not e[0].startswith("prior."))


@pytest.mark.parametrize("name", ["encoder_full_eps"])
def test_fixed_rate_manifests_unchanged(name):
    meta = _meta(name)
    ref = _man(meta["manifest"])
    m = cdc.BigCompressor(**meta["kwargs"])
    assert _man(m.manifest()) == [e for e in ref if e[0].startswith("dec.")]
    assert _man(m.hyper_manifest()) == [e for e in ref if e[0].startswith("hyper_dec.")]
    assert _man(m.encoder_manifest()) == [e for e in ref if e[0].startswith(("enc.", "hyper_enc."))]
    assert not any(synth.is_vbr_key(k) for k, _ in m.manifest() + m.hyper_manifest() + m.encoder_manifest())


def _ctxdec_handle(up_index=2):
    cfg = _lib.CtxdecConfig()
    cfg.dim, cfg.out_channels, cfg.up_index, cfg.n_rev_mults = 8, 3, up_index, 2
    cfg.rev_mults[0], cfg.rev_mults[1] = 2, 1
    h = ctypes.c_void_p()
    assert L.cdc_ctxdec_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    return h


def _names(h):
    out = []
    for i in range(L.cdc_num_tensors(h)):
        nm, shape, nd = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
        assert L.cdc_tensor_info(h, i, ctypes.byref(nm), shape, ctypes.byref(nd)) == 0
        out.append(nm.value.decode())
    return out


def test_enable_vbr_order_and_handle_kinds():
    h = _ctxdec_handle()
    try:
        n0 = L.cdc_num_tensors(h)
        assert L.cdc_enable_vbr(h) == 0
        assert L.cdc_enable_vbr(h) == 0                     # idempotent
        names = _names(h)
        assert len(names) == n0 + 2 * 4                       # two levels, four tensors each
        assert [n for n in names if synth.is_vbr_key(n)][:4] == ["dec.0.1.scale.weight", "dec.0.1.scale.bias",
                                                                 "dec.0.1.shift.weight", "dec.0.1.shift.bias"]
        # finalize requires the new tensors (CDC_ERR_STATE names the first missing one)
        assert L.cdc_finalize_weights(h) == -2
    finally:
        L.cdc_destroy(h)
    # refused once a tensor is loaded
    h = _ctxdec_handle()
    try:
        name = _names(h)[-1].encode()                        # dec.1.2.conv.bias [3]
        a = np.zeros(3, np.float32)
        shape = (ctypes.c_int64 * 1)(3)
        assert L.cdc_load_tensor(h, name, a.ctypes.data, shape, 1) == 0
        assert L.cdc_enable_vbr(h) == -2
        assert b"before any cdc_load_tensor" in L.cdc_last_error(h)
    finally:
        L.cdc_destroy(h)
    # the VBRCondition sits at index 1: a resampling layer there (xparam ResnetCompressor layout) cannot take it
    h = _ctxdec_handle(up_index=1)
    try:
        assert L.cdc_enable_vbr(h) == -1
    finally:
        L.cdc_destroy(h)
    assert L.cdc_enable_vbr(None) == -1


def test_set_bitrate_scale_rules():
    h = _ctxdec_handle()
    try:
        one = np.array([0.5], np.float32)
        assert L.cdc_set_bitrate_scale(h, one.ctypes.data, 1) == -2          # not a VBR handle
        assert L.cdc_enable_vbr(h) == 0
        assert L.cdc_set_bitrate_scale(h, one.ctypes.data, 1) == 0
        for bad in (np.nan, np.inf, -np.inf):
            a = np.array([0.1, bad, 0.3], np.float32)
            assert L.cdc_set_bitrate_scale(h, a.ctypes.data, 3) == -1
            assert b"not finite" in L.cdc_last_error(h)
        assert L.cdc_set_bitrate_scale(h, one.ctypes.data, 0) == -1
        assert L.cdc_set_bitrate_scale(h, None, 1) == -1
        # extrapolated and negative rates are finite: taken
        a = np.array([-3.0, 0.0, 9.25], np.float32)
        assert L.cdc_set_bitrate_scale(h, a.ctypes.data, 3) == 0
    finally:
        L.cdc_destroy(h)


def _header(version, rate=None, hh=3, wh=5, arith=1):
    body = struct.pack("<3sBBBHHIIIIII", b"CDC", version, arith, 0, hh, wh, 256, 256, 0x1234, 0, 0, 0)
    assert len(body) == 34
    if rate is not None:
        body += struct.pack("<f", rate)
    return body + bytes(512)


def _peek_rate(s):
    has, r = ctypes.c_int(-1), ctypes.c_float(-1)
    rc = L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(has), ctypes.byref(r))
    return rc, has.value, r.value


def test_peek_bitrate_scale_of_hand_built_headers():
    for rate in (0.0, 0.37, 1.0, -2.5, 9.25):
        s = _header(4, rate)
        rc, has, r = _peek_rate(s)
        assert rc == 0 and has == 1
        assert np.float32(r).view(np.uint32) == np.float32(rate).view(np.uint32)
        hh, wh, ar = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert L.cdc_entropy_peek(s, len(s), ctypes.byref(hh), ctypes.byref(wh), ctypes.byref(ar)) == 0
        assert (hh.value, wh.value, ar.value) == (3, 5, 1)
    rc, has, _ = _peek_rate(_header(3))
    assert rc == 0 and has == 0
    assert _peek_rate(_header(5))[0] == -1                     # unknown container version
    assert _peek_rate(_header(4, 0.5)[:36])[0] == -1           # the rate itself truncated
    assert _peek_rate(b"XDC" + _header(4, 0.5)[3:])[0] == -1
    assert cdc.BigCompressor.bitrate_scale_of([_header(4, 0.25), _header(4, 1.0)]).tolist() == [0.25, 1.0]
    with pytest.raises(_lib.CdcError, match="fixed-rate"):
        cdc.BigCompressor.bitrate_scale_of([_header(3)])


def test_python_front_end_refusals():
    meta = _meta("vbr_small")
    q = np.zeros((2, 32, 2, 2), np.float32)
    fixed = cdc.BigCompressor(**meta["kwargs"])
    with pytest.raises(NotImplementedError):
        fixed.decode(q, np.array([0.5], np.float32))
    with pytest.raises(NotImplementedError):
        fixed.encode(np.zeros((2, 3, 64, 64), np.float32), np.array([0.5], np.float32))
    vbr = cdc.BigCompressor(vbr=True, **meta["kwargs"])
    assert vbr.vbr and not fixed.vbr
    with pytest.raises(ValueError, match="needs a bitrate_scale"):
        vbr.decode(q)
    with pytest.raises(ValueError, match="1 or 2 expected"):
        vbr.decode(q, np.array([0.1, 0.2, 0.3], np.float32))
    with pytest.raises(ValueError, match="needs a bitrate_scale"):
        vbr.encode(np.zeros((2, 3, 64, 64), np.float32))
    with pytest.raises(ValueError, match="needs a bitrate_scale"):
        vbr.compress_to_bytes(np.zeros((2, 3, 64, 64), np.float32))
