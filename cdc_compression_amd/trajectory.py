"""Decode trajectory: the prediction x0 and the state x_t of chosen steps, recorded inside the device loop (include/cdc_hip.h:
cdc_set_trace, cdc_trace_info, cdc_trace_read; the tap kernel lives beside the sampler kernels in csrc/sampler_kernels.hip).

For sample index i (a decode runs i = steps-1 .. 0): `x0[i]` is the prediction the update of step i used -- after the clip that
applies to the image -- and `x_t[i]` the state that update produced; `x_t` of index 0 is the decode's result.  In the x-parameterisation
`x0` of the first executed step is the network's direct estimate of the image from the latent; the later steps trade it for detail, so
one decode holds a walk along the distortion-perception trade-off.  (What that walk looks like on trained weights has not been
measured with this package: the tests run synthetic weights.)

The keywords of `p_sample_loop`, `decompress`, `compress` and `evaluate`:
    trajectory        None | an int n >= 1: every n-th executed step from the first, plus index 0 | a sequence of sample indices
    trajectory_of     "x0" | "x_t" | "both"
    trajectory_dtype  "float32" | "uint8" (the as-saved bytes, cropped inside the tap kernel: 1 byte per element of the window)
With a trajectory the calls return their usual result plus a `Trajectory`.  This module holds the argument rules -- all raised as
ValueError before anything runs -- and the result type; diffusion.py sets the trace around the library call and clears it again."""
import ctypes

import numpy as np

from . import _lib

KINDS = {"x0": _lib.CDC_TRACE_X0, "x_t": _lib.CDC_TRACE_XT, "both": _lib.CDC_TRACE_X0 | _lib.CDC_TRACE_XT}
DTYPES = ("float32", "uint8")


def expand(trajectory, steps):
    """The sample indices of `trajectory` at `steps` sample steps, in execution order (descending).
    An int n: steps-1, steps-1-n, ... and index 0.  A sequence: its indices, each inside [0, steps) and none twice."""
    steps = int(steps)
    if isinstance(trajectory, (bool, np.bool_)):
        raise ValueError("trajectory is None, an int n >= 1 or a sequence of sample indices, not a bool")
    if isinstance(trajectory, (int, np.integer)):
        n = int(trajectory)
        if n < 1:
            raise ValueError(f"trajectory={n}: every n-th step needs n >= 1")
        idx = list(range(steps - 1, -1, -n))
        if idx[-1] != 0:
            idx.append(0)
        return idx
    try:
        raw = list(trajectory)
    except TypeError:
        raise ValueError(f"trajectory {trajectory!r}: None, an int n >= 1 or a sequence of sample indices") from None
    idx = []
    for v in raw:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"trajectory index {v!r} is not an int")
        v = int(v)
        if not 0 <= v < steps:
            raise ValueError(f"trajectory index {v} outside [0, {steps})")
        if v in idx:
            raise ValueError(f"trajectory index {v} is given twice")
        idx.append(v)
    if not idx:
        raise ValueError("trajectory is an empty sequence: None turns it off")
    return sorted(idx, reverse=True)


class Spec:
    """A checked request: indices in execution order, the `what` bits of cdc_set_trace, the slot dtype."""

    def __init__(self, indices, of, dtype):
        self.indices, self.of, self.dtype = list(indices), of, dtype
        self.u8 = dtype == "uint8"
        self.what = KINDS[of] | (_lib.CDC_TRACE_U8 if self.u8 else 0)


def check_args(trajectory, trajectory_of, trajectory_dtype, steps, samples=None, eta=0, seed=None):
    """The argument rules, before anything runs -> a Spec, or None without a trajectory."""
    if trajectory is None:
        if trajectory_of != "x0" or trajectory_dtype != "float32":
            raise ValueError("trajectory_of / trajectory_dtype belong to trajectory=")
        return None
    if trajectory_of not in KINDS:
        raise ValueError(f"trajectory_of {trajectory_of!r}: one of {tuple(KINDS)}")
    if trajectory_dtype not in DTYPES:
        raise ValueError(f"trajectory_dtype {trajectory_dtype!r}: one of {DTYPES}")
    if samples is not None:
        raise ValueError("trajectory and samples=K exclude each other: a trajectory belongs to a single decode")
    if eta != 0 and seed is None:
        raise ValueError("trajectory with eta != 0 needs a seed: without one the decode runs in the host loop, which has no x0")
    return Spec(expand(trajectory, steps), trajectory_of, trajectory_dtype)


class Trajectory:
    """steps: the recorded sample indices in execution order;  train_index: their train indices (diffusion.index[steps]);
    x0 / x_t: [S, B, 3, H, W] in the container family of the reconstruction (NumPy or torch), float32 or uint8, cropped to the image's
    window as the reconstruction is; None for a kind that was not asked for."""

    def __init__(self, steps, train_index, x0=None, x_t=None):
        self.steps, self.train_index, self.x0, self.x_t = list(steps), train_index, x0, x_t

    def __len__(self):
        return len(self.steps)

    def __repr__(self):
        kinds = [k for k, v in (("x0", self.x0), ("x_t", self.x_t)) if v is not None]
        shape = tuple((self.x0 if self.x0 is not None else self.x_t).shape) if kinds else ()
        return f"Trajectory(steps={self.steps}, {'+'.join(kinds)} {shape})"


class active:
    """`with active(handle, spec, win_h, win_w):` sets the trace on the library handle and clears it again, also on error."""

    def __init__(self, handle, spec, win_h=0, win_w=0):
        self.h, self.spec, self.win = handle, spec, (int(win_h), int(win_w))

    def __enter__(self):
        idx = (ctypes.c_int * len(self.spec.indices))(*self.spec.indices)
        _lib.check(self.h, _lib.lib().cdc_set_trace(self.h, idx, len(self.spec.indices), self.spec.what, *self.win))
        return self

    def __exit__(self, *exc):
        _lib.lib().cdc_set_trace(self.h, None, 0, 0, 0, 0)
        return False


def read(handle, spec, proto, device_index):
    """The slots of the last traced decode -> {"x0": [S, B, C, h, w] or None, "x_t": ...} in `proto`'s container family (h x w: the
    frame for float32 slots, the window for uint8 ones)."""
    from .frame import _empty_like
    from .unet import _current_stream, _is_torch
    L = _lib.lib()
    v = [ctypes.c_int() for _ in range(6)]
    _lib.check(handle, L.cdc_trace_info(handle, *[ctypes.byref(c) for c in v]))
    S, B, C, H, W, what = (c.value for c in v)
    if S != len(spec.indices) or what != spec.what:
        raise _lib.CdcError(f"the library recorded {S} slots (what = {what}), {len(spec.indices)} (what = {spec.what}) were asked for")
    mem = _lib.CDC_MEM_DEVICE if _is_torch(proto) and proto.is_cuda else _lib.CDC_MEM_HOST
    out = {"x0": None, "x_t": None}
    for name, bit in (("x0", _lib.CDC_TRACE_X0), ("x_t", _lib.CDC_TRACE_XT)):
        if what & bit:
            t, p = _empty_like(proto, (S, B, C, H, W), spec.u8)
            _lib.check(handle, L.cdc_trace_read(handle, bit, 0, S, p, mem, _current_stream(mem)))
            out[name] = t
    return out
