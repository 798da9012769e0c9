"""Float64 reference of the tiled decode's host side and blend (cdc_compression_amd/tiles.py states the definitions; include/cdc_hip.h
the C-ABI): the tile plan, the feather weights and the blend, written from the definitions and independent of the package's code.
Used by tests/test_tiles_host.py (no GPU) and tests/test_gpu_tiles.py."""
import numpy as np


def axis_plan(L, tile, overlap):
    """(origins, size) of the tiles along an axis of length L."""
    if L <= tile:
        return [0], L
    stride = tile - overlap
    origins = []
    k = 0
    while k * stride + tile < L:
        origins.append(k * stride)
        k += 1
    origins.append(L - tile)
    return origins, tile


def axis_weight(p, o, size, L, overlap):
    """float64 weight of the tile [o, o + size) at integer coordinates p of an axis of length L."""
    p = np.asarray(p, dtype=np.float64)
    lo = np.ones_like(p) if o == 0 else np.minimum(1.0, (p - o + 0.5) / overlap)
    hi = np.ones_like(p) if o + size == L else np.minimum(1.0, (o + size - p - 0.5) / overlap)
    return np.minimum(lo, hi)


def cover(origins, size, L):
    """Number of tiles that cover each coordinate of the axis."""
    n = np.zeros(L, np.int64)
    for o in origins:
        n[o:o + size] += 1
    return n


def blend(tiles, ys, xs, Hf, Wf, overlap, present=None):
    """tiles [T][C][Th][Tw] of one image (T = len(ys) * len(xs), row-major; present: the t that are there, `tiles` then holds only
    those, ascending) -> (frame [C][Hf][Wf] float64, sum of weights [Hf][Wf], number of covering present tiles [Hf][Wf]).  Pixels no
    present tile covers are NaN."""
    tiles = np.asarray(tiles, dtype=np.float64)
    _, C, Th, Tw = tiles.shape
    num = np.zeros((C, Hf, Wf))
    den = np.zeros((Hf, Wf))
    cnt = np.zeros((Hf, Wf), np.int64)
    slot = 0
    for ty, oy in enumerate(ys):
        wy = axis_weight(np.arange(oy, oy + Th), oy, Th, Hf, overlap[0])
        for tx, ox in enumerate(xs):
            t = ty * len(xs) + tx
            if present is not None and t not in present:
                continue
            w = wy[:, None] * axis_weight(np.arange(ox, ox + Tw), ox, Tw, Wf, overlap[1])[None, :]
            num[:, oy:oy + Th, ox:ox + Tw] += w[None] * tiles[slot]
            den[oy:oy + Th, ox:ox + Tw] += w
            cnt[oy:oy + Th, ox:ox + Tw] += 1
            slot += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        out = num / den[None]
    return out, den, cnt


def blend_bound(n_terms, vmax):
    """The float32 kernel against this reference, first order in u = 2^-24, for a pixel with n covering tiles (cdc_hip.h states the
    operation order).  A weight carries 3 roundings (two divisions, one product), its product with the value one more: every term of
    the numerator is off by at most 4 u |w v|; n - 1 additions add (n - 1) u of the partial sums, so the numerator is off by at most
    (n + 3) u max|v| sum(w).  The denominator's terms carry 3 u and its additions (n - 1) u: (n + 2) u sum(w).  The division adds u.
    Relative to max|v|: (2 n + 6) u -- 14 u for four terms, 24 u for nine."""
    return (2 * n_terms + 6) * 2.0 ** -24 * vmax
