"""Tiled decode: any image as overlapping tiles, one region on request (include/cdc_hip.h: cdc_tile_gather, cdc_tile_blend,
cdc_set_noise_frames, cdc_randn_framed; kernels in csrc/tile_kernels.hip and csrc/sampler_kernels.hip).

The stream is untouched: one full-frame entropy decode and hyper decode.  What follows the dequantised latent runs on tiles: the
latent is cut into overlapping windows, each window goes through `context_fn.decode` and the sampler as a batch row, and the decoded
tiles are feather-blended into the frame.  All tiles of an image share its seed and draw the noise of the frame positions they cover
(frame-indexed draws), so overlaps see identical noise and one tile that covers the frame is the plain decode.

THE PLAN.  G is the frame multiple of the model (`diffusion.padded_size(1, 1)[0]`); `tile` and `tile_overlap` are multiples of G with
0 < overlap <= tile / 2 (a pair (h, w) gives each axis its own).  Per axis of the padded frame, of length L: L <= tile is one tile of
size L at 0; else the stride is tile - overlap, the origins are 0, stride, 2 stride, ... while origin + tile < L, and one last origin
L - tile follows (the last overlap may be larger than `overlap`, and a point may lie in three tiles).  Tiles are numbered row-major,
t = ty * nx + tx; batch rows are b * T + t.

THE WEIGHTS of the blend, per axis, for a tile [o, o + size) at coordinate p: lo = 1 if o == 0 else min(1, (p - o + 0.5) / overlap),
hi = 1 if o + size == L else min(1, (o + size - p - 0.5) / overlap), w = min(lo, hi); a tile's weight is w_y * w_x and the result
sum(w v) / sum(w) over the covering tiles in ascending t, in float32.

What tiling does to decoded images of trained weights is not measured: this module defines the operation."""
import contextlib
import ctypes

import numpy as np

from . import _lib, frame
from .unet import _Arg, _current_stream, _result_like

MAX_ROWS = 32          # rows of one sampler call under the default chunk rule (as samples.MAX_ROWS)
_I32P = ctypes.POINTER(ctypes.c_int32)


def _pair(v, name):
    """An int or a pair (h, w) of ints -> (h, w)."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be an int or a pair (h, w), not {v!r}")
        h, w = v
    else:
        h = w = v
    for x in (h, w):
        if isinstance(x, bool) or not hasattr(x, "__index__"):
            raise ValueError(f"{name} must be an int or a pair (h, w) of ints, not {v!r}")
    return int(h), int(w)


def check_args(tile, tile_overlap=None, tile_chunk=None, region=None, samples=None, trajectory=None, maps=False):
    """The argument rules of `tile=` that need no model, checked before anything runs -> ((th, tw), (oh, ow) or None)."""
    if tile is None:
        for name, v in (("tile_overlap", tile_overlap), ("tile_chunk", tile_chunk), ("region", region)):
            if v is not None:
                raise ValueError(f"{name} belongs to tile=")
        return None, None
    if samples is not None:
        raise ValueError("tile and samples exclude each other: K samples per image run on the whole frame")
    if trajectory is not None:
        raise ValueError("tile and trajectory exclude each other: a trajectory is recorded on the whole frame")
    if maps:
        raise ValueError("tile and maps=True exclude each other")
    t = _pair(tile, "tile")
    o = None if tile_overlap is None else _pair(tile_overlap, "tile_overlap")
    if min(t) < 1:
        raise ValueError(f"tile must be positive, not {tile!r}")
    if o is not None and any(not 0 < ov <= tl // 2 for ov, tl in zip(o, t)):
        raise ValueError(f"tile_overlap {tile_overlap!r}: 0 < overlap <= tile / 2 on each axis (tile {tile!r})")
    if tile_chunk is not None and (isinstance(tile_chunk, bool) or not hasattr(tile_chunk, "__index__") or int(tile_chunk) < 1):
        raise ValueError(f"tile_chunk must be an int >= 1, not {tile_chunk!r}")
    if region is not None:
        if not isinstance(region, (tuple, list)) or len(region) != 4 or any(isinstance(v, bool) or not hasattr(v, "__index__") for v in region):
            raise ValueError(f"region must be (y0, x0, h, w) in image pixels, not {region!r}")
        if region[0] < 0 or region[1] < 0 or region[2] < 1 or region[3] < 1:
            raise ValueError(f"region {tuple(region)!r}: y0, x0 >= 0 and h, w >= 1")
    return t, o


def check_multiples(tile, overlap, G):
    """`tile` / `overlap` pairs against the frame multiple G -> (tile, overlap), the overlap defaulting to G."""
    if overlap is None:
        overlap = (G, G)
    for name, v in (("tile", tile), ("tile_overlap", overlap)):
        if any(x % G for x in v):
            raise ValueError(f"{name} {v} must be a multiple of the model's frame multiple {G}")
    if any(not 0 < ov <= tl // 2 for ov, tl in zip(overlap, tile)):
        raise ValueError(f"tile_overlap {overlap}: 0 < overlap <= tile / 2 on each axis (tile {tile}, frame multiple {G})")
    return tile, overlap


def check_region(region, H, W):
    """(y0, x0, h, w) inside the H x W image -> the tuple of ints."""
    y0, x0, h, w = (int(v) for v in region)
    if y0 + h > H or x0 + w > W:
        raise ValueError(f"region {(y0, x0, h, w)} reaches outside the {H} x {W} image")
    return y0, x0, h, w


def axis_origins(L, tile, overlap):
    """The origins of the tiles along one axis of length L (module docstring) -> (origins, size)."""
    if L <= tile:
        return [0], L
    stride, out, o = tile - overlap, [], 0
    while o + tile < L:
        out.append(o)
        o += stride
    out.append(L - tile)
    return out, tile


def axis_weight(p, o, size, L, overlap):
    """The weight of the tile [o, o + size) of an axis of length L at coordinate(s) p, float64 (module docstring)."""
    p = np.asarray(p, np.float64)
    lo = np.ones_like(p) if o == 0 else np.minimum(1.0, (p - o + 0.5) / overlap)
    hi = np.ones_like(p) if o + size == L else np.minimum(1.0, (o + size - p - 0.5) / overlap)
    return np.minimum(lo, hi)


class Plan:
    """The tiles of an Hp x Wp frame: `ys` / `xs` the origins per axis, `th` / `tw` the tile size, `T = ny * nx` tiles, tile t at
    `origin(t)`; `overlap` the (oh, ow) the blend ramps over."""

    def __init__(self, Hp, Wp, tile, overlap):
        self.Hp, self.Wp, self.tile, self.overlap = int(Hp), int(Wp), tuple(tile), tuple(overlap)
        self.ys, self.th = axis_origins(self.Hp, tile[0], overlap[0])
        self.xs, self.tw = axis_origins(self.Wp, tile[1], overlap[1])
        self.ny, self.nx = len(self.ys), len(self.xs)
        self.T = self.ny * self.nx

    def origin(self, t):
        return self.ys[t // self.nx], self.xs[t % self.nx]

    def origins(self, tiles=None):
        return [self.origin(t) for t in (range(self.T) if tiles is None else tiles)]

    def intersecting(self, region=None):
        """The tiles (ascending t) that intersect the window (y0, x0, h, w) of the frame; None: all."""
        if region is None:
            return list(range(self.T))
        y0, x0, h, w = region
        rows = [k for k, o in enumerate(self.ys) if o < y0 + h and o + self.th > y0]
        cols = [k for k, o in enumerate(self.xs) if o < x0 + w and o + self.tw > x0]
        return [ty * self.nx + tx for ty in rows for tx in cols]


def default_chunk(rows):
    """Rows per sampler call: the fewest calls of at most 32 rows, as equal as they come."""
    calls = -(-rows // MAX_ROWS)
    return -(-rows // calls)


# ---- the library calls ------------------------------------------------------------------------------------------------------------
def _i32(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data_as(_I32P)


def gather(handle, src, origins, th, tw, device_index):
    """src [B, C, Hs, Ws] float32 -> [B * T, C, th, tw] in the same container family, row b * T + t the window at origins[t] = (y, x)
    (cdc_tile_gather)."""
    a = _Arg(src, device_index)
    B, C, Hs, Ws = (int(d) for d in a.shape)
    keep, po = _i32(origins)
    T = len(origins)
    out, optr, _ = _result_like(src, (B * T, C, int(th), int(tw)), device_index)
    _lib.check(handle, _lib.lib().cdc_tile_gather(handle, a.ptr, optr, po, B, C, Hs, Ws, T, int(th), int(tw), a.mem, _current_stream(a.mem)))
    return out


def blend(handle, tiles, plan, B, device_index, window=None, present=None, as_uint8=False):
    """tiles [B * Tp, C, th, tw] (the present tiles of each image in ascending t; present: the list of their t, None: all) -> the window
    (y0, x0, h, w) of the blended frame (None: the frame), [B, C, h, w] float32 or uint8 (cdc_tile_blend)."""
    a = _Arg(tiles, device_index)
    C = int(a.shape[1])
    y0, x0, h, w = (0, 0, plan.Hp, plan.Wp) if window is None else window
    ky, pys = _i32(plan.ys)
    kx, pxs = _i32(plan.xs)
    mask = None
    if present is not None:
        mask = np.zeros(plan.T, np.uint8)
        mask[list(present)] = 1
    Tp = plan.T if present is None else len(present)
    if tuple(a.shape) != (B * Tp, C, plan.th, plan.tw):
        raise _lib.CdcError(f"tiles have shape {tuple(a.shape)}: expected {(B * Tp, C, plan.th, plan.tw)}")
    out, po = frame._empty_like(tiles, (B, C, int(h), int(w)), as_uint8)
    _lib.check(handle, _lib.lib().cdc_tile_blend(handle, a.ptr, po, pys, plan.ny, pxs, plan.nx, None if mask is None else mask.ctypes.data, B, C,
                                                 plan.th, plan.tw, plan.Hp, plan.Wp, plan.overlap[0], plan.overlap[1], int(y0), int(x0), int(h), int(w),
                                                 _lib.CDC_ELEM_U8 if as_uint8 else _lib.CDC_ELEM_F32, a.mem, _current_stream(a.mem)))
    return out


def frame_rows(frames):
    """[(frame_h, frame_w, y0, x0)] -> the int32 [n, 4] array the library takes."""
    a = np.ascontiguousarray(frames, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("noise frames are rows of (frame_h, frame_w, y0, x0)")
    return a


@contextlib.contextmanager
def noise_frames(handle, frames):
    """The frame-indexed draws of the seeded calls inside the block (cdc_set_noise_frames), cleared again on the way out, on error too.
    frames None: nothing is set."""
    if frames is None:
        yield
        return
    L = _lib.lib()
    rows = frame_rows(frames)
    _lib.check(handle, L.cdc_set_noise_frames(handle, rows.ctypes.data_as(_I32P), int(rows.shape[0])))
    try:
        yield
    finally:
        L.cdc_set_noise_frames(handle, None, 0)


def randn_framed(handle, seeds, frames, C, th, tw, device_index, draw=0, scale=1.0, like=None):
    """scale * z of the windows [C, th, tw] at (y0, x0) of the rows' frames, made on the device (cdc_randn_framed) -> [n, C, th, tw]."""
    rows = frame_rows(frames)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    n = int(rows.shape[0])
    out, optr, omem = _result_like(like if like is not None else np.empty(0, np.float32), (n, int(C), int(th), int(tw)), device_index)
    _lib.check(handle, _lib.lib().cdc_randn_framed(handle, sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rows.ctypes.data_as(_I32P), n, int(C),
                                                   int(th), int(tw), int(draw), float(scale), optr, omem, _current_stream(omem)))
    return out


def randn_framed_host(seeds, frames, C, th, tw, draw=0, scale=1.0):
    """The same on the host (cdc_randn_framed_host: csrc/rng.h evaluated by the CPU); no handle, no GPU."""
    rows = frame_rows(frames)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    n = int(rows.shape[0])
    out = np.empty((n, int(C), int(th), int(tw)), np.float32)
    rc = _lib.lib().cdc_randn_framed_host(sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rows.ctypes.data_as(_I32P), n, int(C), int(th), int(tw),
                                          int(draw), float(scale), out.ctypes.data)
    if rc != 0:
        raise _lib.CdcError(f"cdc_randn_framed_host: invalid argument ({rc})")
    return out
