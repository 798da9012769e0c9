"""Distortion of decoded images, computed on the device (include/cdc_hip.h: cdc_distortion; kernels in csrc/metric_kernels.hip).

`psnr` and `ms_ssim` compare two image batches `[B, 3, Hf, Wf]` over their top-left `H x W` window (`size=(H, W)`; default: the
operands' common shape), so a padded decoder frame is measured beside the image without a crop or a copy off the device.  Operands
are numpy, torch-cpu or torch-cuda tensors, float32 (in [-1, 1], mapped as `clamp(-1, 1) / 2 + 0.5`) or uint8 (`v / 255`);
`as_saved=True` measures a float32 operand through the uint8 image the reference's script would save.  The header states the
definition (PSNR: the reference's per-image `batch_psnr`; MS-SSIM: the conventions of pytorch-msssim 0.2.1, `data_range=1`).
`sse_map` is the squared error per cell of a grid over the window (cdc_distortion_map), the picture beside a compressor's `rate_map`.
`psnr_weighted` composes it on the host into a PSNR with a weight per cell: the figure of region-of-interest coding (`price_map=`).
`lpips` is the third axis: LPIPS-VGG of lpips 0.1.4 on the same operands (cdc_lpips; the model is an `lpips.LpipsVGG`, which holds
the network's weights).  Results are float64 NumPy arrays of `B` values."""
import ctypes
import math

import numpy as np

from . import _lib, frame
from .unet import _Arg, _current_stream, _is_torch

MS_SSIM_MIN_SIDE = 161      # min(H, W) > 160: five scales of an 11-tap window
LPIPS_MIN_SIDE = 16         # four floor-mode poolings leave at least one pixel


def _is_f32(t):
    if _is_torch(t):
        import torch
        return t.dtype == torch.float32
    return isinstance(t, np.ndarray) and t.dtype == np.float32


def _check_args(a, b, size, as_saved):
    """The argument rules, checked before the library is touched -> (B, H, W, (saved_a, saved_b))."""
    shapes = []
    for name, t in (("a", a), ("b", b)):
        if not (frame.is_uint8(t) or _is_f32(t)):
            raise ValueError(f"operand {name} must be a float32 or uint8 numpy array or torch tensor, got {getattr(t, 'dtype', type(t))}")
        shape = tuple(int(d) for d in t.shape)
        if len(shape) != 4 or shape[1] != 3 or min(shape) < 1:
            raise ValueError(f"operand {name} must be [B, 3, H, W] with H, W >= 1, got {shape}")
        shapes.append(shape)
    if shapes[0][0] != shapes[1][0]:
        raise ValueError(f"the operands hold {shapes[0][0]} and {shapes[1][0]} images")
    if size is None:
        if shapes[0][2:] != shapes[1][2:]:
            raise ValueError(f"operands of {shapes[0][2:]} and {shapes[1][2:]}: size=(H, W) names the window of differing frames")
        H, W = shapes[0][2:]
    else:
        H, W = (int(d) for d in size)
        if H < 1 or W < 1:
            raise ValueError(f"size {tuple(size)} must be positive")
    for name, s in zip("ab", shapes):
        if s[2] < H or s[3] < W:
            raise ValueError(f"the {H} x {W} window is larger than operand {name} ({s[2]} x {s[3]})")
    saved = (as_saved, as_saved) if isinstance(as_saved, bool) else tuple(bool(s) for s in as_saved)
    if len(saved) != 2:
        raise ValueError("as_saved is a bool or one bool per operand")
    # as_saved says "as the script saves it": a uint8 operand already is
    saved = tuple(s and not frame.is_uint8(t) for s, t in zip(saved, (a, b)))
    return shapes[0][0], H, W, saved


def _views(a, b, saved, dev):
    """The two operands as (pointer holders, cdc_image_view structures) in one memory space."""
    args = [frame._ArgU8(t, dev) if frame.is_uint8(t) else _Arg(t, dev) for t in (a, b)]
    if args[0].mem != args[1].mem:       # one mem_kind per call: a host operand joins the other on the device
        import torch
        args = [x if x.mem == _lib.CDC_MEM_DEVICE else
                (frame._ArgU8 if x.keep.dtype == np.uint8 else _Arg)(torch.from_numpy(x.keep).to(f"cuda:{dev}"), dev) for x in args]
    views = [_lib.ImageView(x.ptr, _lib.CDC_ELEM_U8 if frame.is_uint8(t) else _lib.CDC_ELEM_F32, x.shape[2], x.shape[3], int(s))
             for x, t, s in zip(args, (a, b), saved)]
    return args, views


def _distortion(model, a, b, size, as_saved, what, components=False):
    B, H, W, saved = _check_args(a, b, size, as_saved)
    if what & _lib.CDC_METRIC_MSSSIM and min(H, W) < MS_SSIM_MIN_SIDE:
        raise ValueError(f"MS-SSIM needs min(H, W) > 160, got {H} x {W}")
    h, dev = model._handle(), model.device_index
    args, views = _views(a, b, saved, dev)
    ps, ms, comp = np.empty(B, np.float64), np.empty(B, np.float64), np.empty((B, 5, 3), np.float64)
    p = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))     # noqa: E731
    mem = args[0].mem
    _lib.check(h, _lib.lib().cdc_distortion(h, ctypes.byref(views[0]), ctypes.byref(views[1]), B, H, W, what, p(ps), p(ms),
                                            p(comp) if components else None, mem, _current_stream(mem)))
    return ps, ms, comp


def psnr(model, a, b, size=None, as_saved=False):
    """10 log10(1 / mean((a - b)^2)) per image over the window, float64 [B]; +inf for identical operands.  `model`: anything with
    `_handle()` and `device_index` (a Unet, a compressor).  Two byte operands (uint8, or float32 with as_saved) give the exact MSE."""
    return _distortion(model, a, b, size, as_saved, _lib.CDC_METRIC_PSNR)[0]


def ms_ssim(model, a, b, size=None, as_saved=False, return_components=False):
    """MS-SSIM per image over the window, float64 [B] (min(H, W) > 160).  return_components: also [B, 5, 3], per channel the
    relu'd mean cs of scales 0-3 and the relu'd mean ssim of scale 4."""
    _, ms, comp = _distortion(model, a, b, size, as_saved, _lib.CDC_METRIC_MSSSIM, return_components)
    return (ms, comp) if return_components else ms


def distortion(model, a, b, size=None, as_saved=False):
    """(psnr [B], ms_ssim [B]) in one call; ms_ssim is None when the window is too small for five scales."""
    _, H, W, _ = _check_args(a, b, size, as_saved)
    if min(H, W) < MS_SSIM_MIN_SIDE:
        return psnr(model, a, b, size, as_saved), None
    ps, ms, _ = _distortion(model, a, b, size, as_saved, _lib.CDC_METRIC_PSNR | _lib.CDC_METRIC_MSSSIM)
    return ps, ms


def _check_grid(H, W, cell, grid):
    """The argument rules of sse_map's cell and grid, checked before the library is touched -> (cell, gh, gw)."""
    if isinstance(cell, bool) or int(cell) != cell or int(cell) < 1:
        raise ValueError(f"cell must be an integer >= 1, got {cell!r}")
    cell = int(cell)
    if grid is None:
        return cell, -(-H // cell), -(-W // cell)
    gh, gw = (int(g) for g in grid)
    if gh < 1 or gw < 1 or gh * cell < H or gw * cell < W:
        raise ValueError(f"a {gh} x {gw} grid of {cell}-pixel cells does not cover the {H} x {W} window")
    return cell, gh, gw


def sse_map(model, a, b, cell, size=None, as_saved=False, grid=None):
    """Where the error remains (cdc_distortion_map): (sse float64 [B, gh, gw], count int32 [B, gh, gw]) over cells of cell x cell
    pixels anchored at the window's top-left pixel.  sse: the sum of (a - b)^2 over the three channels and the cell's pixels inside
    the window, operands and window as for `psnr`; count: 3 x those pixels, 0 for a cell beyond the window.  grid=(gh, gw): default
    ceil(H / cell) x ceil(W / cell); a larger one (the rate map's, of the padded frame) gets zero cells.  sse.sum() / count.sum()
    over an image is the MSE of `psnr`; two byte operands give exact sums."""
    B, H, W, saved = _check_args(a, b, size, as_saved)
    cell, gh, gw = _check_grid(H, W, cell, grid)
    h, dev = model._handle(), model.device_index
    args, views = _views(a, b, saved, dev)
    sse, count = np.empty((B, gh, gw), np.float64), np.empty((B, gh, gw), np.int32)
    mem = args[0].mem
    if mem == _lib.CDC_MEM_HOST:
        ps, pc, keep = sse.ctypes.data, count.ctypes.data, None
    else:
        import torch
        keep = (torch.empty((B, gh, gw), dtype=torch.float64, device=f"cuda:{dev}"), torch.empty((B, gh, gw), dtype=torch.int32, device=f"cuda:{dev}"))
        ps, pc = keep[0].data_ptr(), keep[1].data_ptr()
    _lib.check(h, _lib.lib().cdc_distortion_map(h, ctypes.byref(views[0]), ctypes.byref(views[1]), B, H, W, cell, gh, gw, ps, pc, mem,
                                                _current_stream(mem)))
    if keep is not None:
        sse, count = keep[0].cpu().numpy(), keep[1].cpu().numpy()
    return sse, count


def weighted_psnr_of(sse, count, cell_weights):
    """The host composition of `psnr_weighted`: sse float64 / count int32 [B, gh, gw] of `sse_map` and weights [gh, gw], [1, gh, gw] or
    [B, gh, gw] (finite, >= 0, a positive total over the cells inside the window) -> 10 log10(1 / (sum w sse / sum w count)) per image,
    float64 [B]; +inf where the weighted error is 0."""
    sse, count = np.asarray(sse, np.float64), np.asarray(count, np.float64)
    w = np.asarray(cell_weights.detach().cpu().numpy() if _is_torch(cell_weights) else cell_weights, np.float64)
    if w.ndim == 2:
        w = w[None]
    if sse.ndim != 3 or count.shape != sse.shape or w.ndim != 3 or w.shape[1:] != sse.shape[1:] or w.shape[0] not in (1, sse.shape[0]):
        raise ValueError(f"cell_weights of shape {w.shape} for maps of shape {sse.shape}: [gh, gw], [1, gh, gw] or [B, gh, gw] expected")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("cell_weights: every weight must be finite and >= 0")
    num, den = (w * sse).reshape(sse.shape[0], -1).sum(1), (w * count).reshape(sse.shape[0], -1).sum(1)
    if np.any(den <= 0):
        raise ValueError("cell_weights: no weight on any pixel of the window")
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(1.0 / (num / den))


def psnr_weighted(model, a, b, cell_weights, cell, size=None, as_saved=False):
    """PSNR with a weight per cell of `sse_map`'s grid -- the figure a region-of-interest user reports: 10 log10(1 / (sum w sse /
    sum w count)) per image, float64 [B], composed on the host in float64 from `sse_map(model, a, b, cell, size, as_saved, grid)`.
    cell_weights: [gh, gw], [1, gh, gw] or [B, gh, gw], finite and >= 0; its grid may be the default one of the window or a larger one
    (the rate map's, of the padded frame: cells beyond the window have count 0 and do not weigh).  All weights equal gives `psnr`'s MSE
    to float64 rounding."""
    w = cell_weights.detach().cpu().numpy() if _is_torch(cell_weights) else np.asarray(cell_weights)
    if w.ndim not in (2, 3):
        raise ValueError(f"cell_weights of shape {w.shape}: [gh, gw], [1, gh, gw] or [B, gh, gw] expected")
    sse, count = sse_map(model, a, b, cell, size=size, as_saved=as_saved, grid=tuple(w.shape[-2:]))
    return weighted_psnr_of(sse, count, w)


def lpips(model, a, b, size=None, as_saved=False, return_layers=False):
    """LPIPS-VGG per image over the window, float64 [B] (H, W >= 16).  `model`: an `LpipsVGG` with loaded weights.
    return_layers: also [B, 5], the values of the taps relu1_2 ... relu5_3 whose sum the distance is."""
    B, H, W, saved = _check_args(a, b, size, as_saved)
    if min(H, W) < LPIPS_MIN_SIDE:
        raise ValueError(f"LPIPS-VGG needs H, W >= 16 (four poolings), got {H} x {W}")
    h, dev = model._ready(), model.device_index
    args, views = _views(a, b, saved, dev)
    out, layers = np.empty(B, np.float64), np.empty((B, 5), np.float64)
    p = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))     # noqa: E731
    mem = args[0].mem
    _lib.check(h, _lib.lib().cdc_lpips(h, ctypes.byref(views[0]), ctypes.byref(views[1]), B, H, W, p(out), p(layers), mem, _current_stream(mem)))
    return (out, layers) if return_layers else out


def ms_ssim_db(m):
    """-10 log10(1 - m): the decibel scale MS-SSIM is plotted on (+inf at m = 1)."""
    if np.ndim(m) == 0:
        m = float(m)
        return math.inf if m >= 1.0 else -10.0 * math.log10(1.0 - m)
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(1.0 - np.asarray(m, np.float64))
