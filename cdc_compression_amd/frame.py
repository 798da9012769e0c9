"""Images of any size: the padded frame a model runs on, and the window that comes back (include/cdc_hip.h: cdc_padded_size,
cdc_frame_pad, cdc_frame_crop; kernels in csrc/frame_kernels.hip).

The rule (fixed, so that encoder and decoder agree): M is the least common multiple of what the model's parts need, the frame is
`ceil(H / M) M x ceil(W / M) M`, padding goes to the bottom and the right by edge replication
(`torch.nn.functional.pad(mode="replicate")`), the result is the frame's top-left `H x W` window, start noise given at `H x W` is
extended with zeros, and bpp counts bits over `H * W`.  uint8 images (`torchvision.io.read_image` layout) are converted on the
device as the reference's scripts do (`v / 255 * 2 - 1`; back: `clamp(-1, 1) / 2 + 0.5`, then `save_image`'s rounding)."""
import ctypes

import numpy as np

from . import _lib
from .unet import _Arg, _current_stream, _is_torch


def is_uint8(t):
    if _is_torch(t):
        import torch
        return t.dtype == torch.uint8
    return isinstance(t, np.ndarray) and t.dtype == np.uint8


class _ArgU8:
    """(pointer, mem kind) of a numpy / torch-cpu / torch-cuda uint8 tensor, as unet._Arg is for float32."""

    def __init__(self, t, device_index):
        if _is_torch(t) and t.is_cuda:
            if t.device.index != device_index:
                raise _lib.CdcError(f"tensor on cuda:{t.device.index}, model on cuda:{device_index}")
            t = t.detach().contiguous()
            self.keep, self.ptr, self.mem, self.shape = t, t.data_ptr(), _lib.CDC_MEM_DEVICE, tuple(t.shape)
        else:
            a = np.ascontiguousarray(t.detach().numpy() if _is_torch(t) else t)
            self.keep, self.ptr, self.mem, self.shape = a, a.ctypes.data, _lib.CDC_MEM_HOST, tuple(a.shape)


def _empty_like(proto, shape, u8):
    """Uninitialised float32 / uint8 result in `proto`'s container family -> (tensor, pointer)."""
    if _is_torch(proto):
        import torch
        t = torch.empty(shape, dtype=torch.uint8 if u8 else torch.float32, device=proto.device)
        return t, t.data_ptr()
    a = np.empty(shape, np.uint8 if u8 else np.float32)
    return a, a.ctypes.data


def image_shape(t):
    shape = tuple(t.shape)
    if len(shape) != 4 or shape[1] != 3 or min(shape) < 1:
        raise _lib.CdcError(f"images must be [B, 3, H, W] with H, W >= 1, got {shape}")
    return shape


def padded_size(handles, H, W):
    """(Hp, Wp) of an H x W image for a model made of `handles` (each rounds up to its own power of two: the largest decides)."""
    L = _lib.lib()
    Hp, Wp = int(H), int(W)
    a, b = ctypes.c_int(), ctypes.c_int()
    for h in handles:
        _lib.check(h, L.cdc_padded_size(h, int(H), int(W), ctypes.byref(a), ctypes.byref(b)))
        Hp, Wp = max(Hp, a.value), max(Wp, b.value)
    return Hp, Wp


def pad(handle, images, Hp, Wp, device_index, zero=False):
    """[B, 3, H, W] float32 or uint8 -> float32 [B, 3, Hp, Wp] in the same container family (one kernel, on the device)."""
    u8 = is_uint8(images)
    a = _ArgU8(images, device_index) if u8 else _Arg(images, device_index)
    B, _, H, W = image_shape(a)
    out, po = _empty_like(images, (B, 3, Hp, Wp), False)
    _lib.check(handle, _lib.lib().cdc_frame_pad(handle, a.ptr, po, B, H, W, int(Hp), int(Wp), _lib.CDC_ELEM_U8 if u8 else _lib.CDC_ELEM_F32,
                                                _lib.CDC_FILL_ZERO if zero else _lib.CDC_FILL_EDGE, a.mem, _current_stream(a.mem)))
    return out


def crop(handle, frame, H, W, device_index, as_uint8=False):
    """float32 [B, 3, Hp, Wp] -> its top-left [B, 3, H, W] window, float32 (bit for bit) or the uint8 the reference's script saves."""
    a = _Arg(frame, device_index)
    B, _, Hp, Wp = image_shape(a)
    out, po = _empty_like(frame, (B, 3, int(H), int(W)), as_uint8)
    _lib.check(handle, _lib.lib().cdc_frame_crop(handle, a.ptr, po, B, int(H), int(W), Hp, Wp, _lib.CDC_ELEM_U8 if as_uint8 else _lib.CDC_ELEM_F32,
                                                 a.mem, _current_stream(a.mem)))
    return out


def extend_init(handle, init, B, H, W, Hp, Wp, device_index):
    """Start noise: [B, 3, H, W] is extended to the frame with zeros (what the reference starts from when init=None), one already
    of the frame's shape is used as it is, None stays None."""
    if init is None:
        return None
    shape = tuple(init.shape)
    if shape == (B, 3, Hp, Wp):
        return init
    if shape != (B, 3, H, W):
        raise _lib.CdcError(f"init has shape {shape}: expected the image's {(B, 3, H, W)} or the padded frame's {(B, 3, Hp, Wp)}")
    return pad(handle, init, Hp, Wp, device_index, zero=True)
