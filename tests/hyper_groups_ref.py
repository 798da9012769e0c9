"""Grouped hyper part (container versions 19 - 22) restated in Python from the specification in include/cdc_hip.h alone: the 8 bytes,
the index, the channel order of groups, the checksum over the index in the full hyper section.  The sections themselves come from the
CPU oracle (oracle.entropy.encode_hyper over a slice of channels): a group is a section of the ungrouped format over a contiguous
range of the symbols.  The latent part, sym_mix and the header are those of tests/segments_ref.py.  Shared by
tests/test_entropy_hyper_groups.py (no GPU) and tests/test_gpu_entropy_hyper_groups.py."""
import struct

import numpy as np

from oracle import entropy as oe
import segments_ref as sr


def groups(Ch, cg):
    """[(c0, c1)] of the groups in channel order: ceil(Ch / cg) of them, the last may be smaller."""
    return [(c0, min(Ch, c0 + cg)) for c0 in range(0, Ch, cg)]


def hyper_part(sym_h, prior, med, cg):
    """sym_h int32 [Ch, hh, wh] -> (bytes of the hyper part, escapes, checksum, [(section bytes, escapes, checksum)])."""
    sym_h = np.asarray(sym_h, np.int32)
    Ch = sym_h.shape[0]
    index_in_section = np.arange(sym_h.size, dtype=np.uint64).reshape(sym_h.shape)
    entries, sections = [], []
    for c0, c1 in groups(Ch, cg):
        data, ne = oe.encode_hyper(sym_h[c0:c1], prior[c0:c1], med[c0:c1])
        check = int(sr.sym_mix(0, index_in_section[c0:c1].reshape(-1), sym_h[c0:c1].reshape(-1)).sum() & np.uint64(0xFFFFFFFF))
        entries.append((len(data), ne, check))
        sections.append(data)
    part = struct.pack("<HHI", cg, len(entries), 0) + b"".join(struct.pack("<III", *e) for e in entries) + b"".join(sections)
    return part, sum(e[1] for e in entries), sum(e[2] for e in entries) & 0xFFFFFFFF, entries


def oracle_stream(sym_h, sym_l, scale, prior, med, seg, cg, arith=1, version=3, rate=None, size=None):
    """The grouped stream (version byte `version` + 16) of hyper symbols [Ch, hh, wh] in groups of cg channels and latent symbols /
    scales [C, Hl, Wl] in segments of seg positions, all from the oracle."""
    part_h, eh, check_h, _ = hyper_part(sym_h, prior, med, cg)
    part_l, el, check_l, _ = sr.latent_part(sym_l, scale, seg)
    model, symbols = oe.model_hash(prior, med), oe.symbol_hash(sym_h, sym_l)
    assert (check_h + check_l) & 0xFFFFFFFF == symbols                # the group and segment checksums add up to `symbols`
    hh, wh = sym_h.shape[1:]
    s = sr.stream(version, arith, hh, wh, (part_h, eh), part_l, el, model, symbols, rate, size)
    return s[:3] + bytes([version + 16]) + s[4:]
