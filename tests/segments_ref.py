"""Segmented streams (container versions 11 - 14) restated in Python from the specification in include/cdc_hip.h alone: the index,
the segment order, the checksum.  The sections themselves come from the CPU oracle (oracle.entropy.encode_hyper / encode_latent): a
segment is a section of the unsegmented format over a subset of the symbols.  Shared by tests/test_entropy_segments.py (no GPU) and
tests/test_gpu_entropy_segments.py."""
import struct

import numpy as np

from cdc_compression_amd import synth
from oracle import entropy as oe


def prior_sd(C, seed=5):
    """Synthetic FlexiblePrior parameters of C channels (the shapes of the reference's state_dict)."""
    pd = (1, 3, 3, 3, 1)
    sd = {}
    for i in range(4):
        sd[f"prior.affine.{i}.weight"] = synth.normal(f"pw{i}", (C, 1, 1, pd[i], pd[i + 1]), seed, 1.0)
        sd[f"prior.affine.{i}.bias"] = synth.normal(f"pb{i}", (C, 1, 1, 1, pd[i + 1]), seed, 0.1)
        if i < 3:
            sd[f"prior.a.{i}"] = synth.normal(f"pa{i}", (C, 1, 1, 1, pd[i + 1]), seed, 0.5)
    return sd


def sym_mix(sect, i, k):
    """mix(section, index, symbol) of the header comment, elementwise over arrays, in uint32 arithmetic."""
    M = np.uint64(0xFFFFFFFF)
    i = np.asarray(i, np.uint64)
    k = np.asarray(k, np.int64).astype(np.uint64) & M
    v = ((i + np.uint64(1)) * np.uint64(0x9E3779B1) + np.uint64(sect) * np.uint64(0x7F4A7C15)) & M
    v ^= (k * np.uint64(0x85EBCA77)) & M
    v ^= v >> np.uint64(15); v = (v * np.uint64(0x2C1B3C6D)) & M
    v ^= v >> np.uint64(12); v = (v * np.uint64(0x297A2D39)) & M
    v ^= v >> np.uint64(15)
    return v


def windows(Hl, Wl, seg):
    """[(y0, y1, x0, x1)] of the segments in raster order; (ny, nx)."""
    ny, nx = -(-Hl // seg), -(-Wl // seg)
    return [(sy * seg, min(Hl, (sy + 1) * seg), sx * seg, min(Wl, (sx + 1) * seg)) for sy in range(ny) for sx in range(nx)], (ny, nx)


def latent_part(sym, scale, seg):
    """sym int32 / scale float32 [C, Hl, Wl] -> (bytes of the latent part, escapes, checksum, [(section bytes, escapes, checksum)])."""
    sym, scale = np.asarray(sym, np.int32), np.asarray(scale, np.float32)
    C, Hl, Wl = sym.shape
    index_in_section = np.arange(C * Hl * Wl, dtype=np.uint64).reshape(C, Hl, Wl)
    wins, (ny, nx) = windows(Hl, Wl, seg)
    entries, sections = [], []
    for y0, y1, x0, x1 in wins:
        k = sym[:, y0:y1, x0:x1].reshape(-1)                     # (c, y, x), c slowest
        data, ne = oe.encode_latent(k, scale[:, y0:y1, x0:x1].reshape(-1))
        check = int(sym_mix(1, index_in_section[:, y0:y1, x0:x1].reshape(-1), k).sum() & np.uint64(0xFFFFFFFF))
        entries.append((len(data), ne, check))
        sections.append(data)
    part = struct.pack("<HHHH", seg, ny, nx, 0) + b"".join(struct.pack("<III", *e) for e in entries) + b"".join(sections)
    return part, sum(e[1] for e in entries), sum(e[2] for e in entries) & 0xFFFFFFFF, entries


def stream(version, arith, hh, wh, hyper, part, esc_latent, model, symbols, rate=None, size=None):
    """A whole stream: the header of base version `version` (3 .. 6) with version byte version + 8, the hyper section (bytes, escapes)
    of the oracle, the latent part of `latent_part`."""
    hb, he = hyper
    extra = b""
    if version in (4, 6):
        extra += struct.pack("<f", rate)
    if version in (5, 6):
        extra += struct.pack("<II", *size)
    return b"CDC" + bytes([version + 8]) + struct.pack("<BBHHIIIIII", arith, 0, hh, wh, len(hb), len(part), model, symbols, he, esc_latent) + \
        extra + hb + part


def oracle_stream(sym_h, sym_l, scale, prior, med, seg, arith=1, version=3, rate=None, size=None):
    """The segmented stream of hyper symbols [Ch, hh, wh] and latent symbols / scales [C, Hl, Wl], all from the oracle; seg = 0: the
    unsegmented stream of base version `version`."""
    hyper = oe.encode_hyper(sym_h, prior, med)
    model, symbols = oe.model_hash(prior, med), oe.symbol_hash(sym_h, sym_l)
    hh, wh = sym_h.shape[1:]
    if seg == 0:
        lb, le = oe.encode_latent(sym_l, scale)
        s = stream(version, arith, hh, wh, hyper, lb, le, model, symbols, rate, size)
        return s[:3] + bytes([version]) + s[4:]
    part, le, check, _ = latent_part(sym_l, scale, seg)
    assert (check + int(sym_mix(0, np.arange(sym_h.size), sym_h.reshape(-1)).sum())) & 0xFFFFFFFF == symbols
    return stream(version, arith, hh, wh, hyper, part, le, model, symbols, rate, size)
