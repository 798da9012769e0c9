"""Partial streams restated in Python from the specification in include/cdc_hip.h alone: what a prefix of a segmented stream holds
(floor, declared, complete, the status of every segment), the concealed q_latent and the per-pixel mask.  Arithmetic on the index
and np.where on the latent grid: nothing here shares code with the library.  Shared by tests/test_entropy_partial.py (no GPU) and
tests/test_gpu_entropy_partial.py."""
import struct

import numpy as np

OK, ABSENT, DAMAGED = 0, 1, 2


def layout(stream):
    """The fields of a WHOLE segmented stream (versions 11 - 14, 19 - 22), read with struct alone -> dict: version, hdr, n_hyper,
    n_latent, declared, seg, ny, nx, cg, ng, floor, entries [(bytes, esc, checksum)], starts (where each segment begins), ends."""
    v = stream[3]
    base = v - 16 if v >= 19 else v - 8
    assert stream[:3] == b"CDC" and base in (3, 4, 5, 6), v
    hdr = 34 + (4 if base in (4, 6) else 0) + (8 if base in (5, 6) else 0)
    nbh, nbl = struct.unpack("<II", stream[10:18])
    cg, ng = (0, 1) if v < 19 else struct.unpack("<HH", stream[hdr: hdr + 4])
    lat = hdr + nbh
    seg, ny, nx, _ = struct.unpack("<HHHH", stream[lat: lat + 8])
    n = ny * nx
    entries = [struct.unpack("<III", stream[lat + 8 + 12 * i: lat + 20 + 12 * i]) for i in range(n)]
    floor = lat + 8 + 12 * n
    starts = [floor + sum(e[0] for e in entries[:i]) for i in range(n)]
    ends = [s + e[0] for s, e in zip(starts, entries)]
    return dict(version=v, hdr=hdr, n_hyper=nbh, n_latent=nbl, declared=hdr + nbh + nbl, seg=seg, ny=ny, nx=nx, cg=cg, ng=ng, floor=floor,
                entries=entries, starts=starts, ends=ends, lat=lat)


def peek(stream, n):
    """What cdc_entropy_peek_partial says of the first n bytes of the sound stream `stream`: None (refused) or (floor, declared, complete)."""
    lay = layout(stream)
    if n < lay["floor"] or n > lay["declared"]:
        return None
    complete = 0
    for e in lay["ends"]:
        if e > n:
            break
        complete += 1
    return lay["floor"], lay["declared"], complete


def windows(Hl, Wl, seg):
    ny, nx = -(-Hl // seg), -(-Wl // seg)
    return [(sy * seg, min(Hl, (sy + 1) * seg), sx * seg, min(Wl, (sx + 1) * seg)) for sy in range(ny) for sx in range(nx)], (ny, nx)


def status(stream, n, Hl, Wl, window=None, damaged=()):
    """uint8 [ny, nx] of the first n bytes (n >= floor): ABSENT where a segment is not wholly inside [0, n) or does not touch `window`
    (y0, x0, h, w in latent positions), DAMAGED where its index is in `damaged` (and it is there and selected), else OK."""
    lay = layout(stream)
    wins, (ny, nx) = windows(Hl, Wl, lay["seg"])
    assert (ny, nx) == (lay["ny"], lay["nx"]) and lay["floor"] <= n <= lay["declared"]
    out = np.full(ny * nx, ABSENT, np.uint8)
    for i, (y0, y1, x0, x1) in enumerate(wins):
        there = lay["ends"][i] <= n
        sel = window is None or (y0 < window[0] + window[2] and window[0] < y1 and x0 < window[1] + window[3] and window[1] < x1)
        if there and sel:
            out[i] = DAMAGED if i in damaged else OK
    return out.reshape(ny, nx)


def ok_positions(status_b, seg, Hl, Wl):
    """bool [Hl, Wl]: the latent positions of OK segments of one image's status [ny, nx]."""
    ok = np.repeat(np.repeat(np.asarray(status_b) == OK, seg, axis=0), seg, axis=1)
    return ok[:Hl, :Wl]


def conceal(full_q, mean, status, seg):
    """The expected q_latent [B, C, Hl, Wl]: the full decode at the positions of OK segments, hyper_decode's mean elsewhere."""
    full_q, mean = np.asarray(full_q), np.asarray(mean)
    B, _, Hl, Wl = full_q.shape
    out = np.empty_like(full_q)
    for b in range(B):
        out[b] = np.where(ok_positions(status[b], seg, Hl, Wl)[None], full_q[b], mean[b])
    return out


def mask(status, seg, cell, H, W, as_uint8=False):
    """The expected pixel mask [B, 1, H, W]: 1.0 (255) where the pixel's latent position (y // cell, x // cell) lies in an OK segment."""
    status = np.asarray(status)
    B = status.shape[0]
    ys, xs = np.arange(H) // cell // seg, np.arange(W) // cell // seg
    on = status[:, ys][:, :, xs] == OK
    return (on.astype(np.uint8) * 255 if as_uint8 else on.astype(np.float32)).reshape(B, 1, H, W)
