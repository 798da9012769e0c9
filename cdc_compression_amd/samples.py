"""K seeded samples per image: the argument rules, the chunking and the library calls behind `decompress(samples=K)` and
`compress_best_of` (include/cdc_hip.h: cdc_repeat_images, cdc_decode_samples, cdc_sample_moments, cdc_sample_select; kernels in
csrc/sample_kernels.hip).

A seeded decode is a pure function of (stream, seed, gamma, eta, steps); `parallel.sample_seeds` gives sample k of image b its seed.
The K samples of B images run through the batch programs in chunks of `sample_chunk` samples per image (rows b * Kc + kk of one
library call), in order, so sample k = k0 + kk.  Arrays of samples are [B * Kc, 3, H, W] with the samples of an image in a row."""
import ctypes
import math

import numpy as np

from . import _lib, frame
from .unet import _Arg, _current_stream, _result_like

REDUCES = (None, "mean", "mean_var")
METRICS = {"psnr": True, "ms_ssim": True, "lpips": False}      # name -> higher is better
MAX_ROWS = 32                                                   # rows of one library call under the default chunk rule


def default_chunk(B, K):
    """Samples per image per library call: the largest divisor of K with B * Kc <= 32, at least 1."""
    return max([d for d in range(1, K + 1) if K % d == 0 and B * d <= MAX_ROWS], default=1)


def check_args(samples, seed, gamma, eta, init=None, reduce=None, as_uint8=False, sample_chunk=None, metric=None):
    """The argument rules of `samples=K`, checked before anything runs -> K."""
    if isinstance(samples, bool) or not hasattr(samples, "__index__") or int(samples) < 1:
        raise ValueError(f"samples must be an int >= 1, not {samples!r}")
    K = int(samples)
    if metric is not None and metric not in METRICS:
        raise ValueError(f"metric {metric!r}: one of {tuple(METRICS)}")
    if reduce not in REDUCES:
        raise ValueError(f"reduce {reduce!r}: one of {REDUCES}")
    if seed is None:
        raise ValueError("samples needs a seed: sample k of image b is the seeded decode of parallel.sample_seeds(seed, B, K)[b][k]")
    if init is not None:
        raise ValueError("samples and init exclude each other: every sample starts from gamma * randn of its own seed (or from zeros)")
    if not (gamma is not None and gamma != 0) and eta == 0:
        raise ValueError("samples needs something stochastic (gamma or eta != 0): the K decodes would be the same picture")
    if reduce == "mean_var" and K < 2:
        raise ValueError('reduce="mean_var" needs samples >= 2 (the unbiased variance divides by K - 1)')
    if reduce == "mean_var" and as_uint8:
        raise ValueError('as_uint8 has no meaning for a variance: use reduce="mean", or convert the mean yourself')
    if sample_chunk is not None and (isinstance(sample_chunk, bool) or not hasattr(sample_chunk, "__index__") or int(sample_chunk) < 1):
        raise ValueError(f"sample_chunk must be an int >= 1, not {sample_chunk!r}")
    return K


def chunks(B, K, sample_chunk=None):
    """[(k0, Kc)] of the library calls, in order."""
    Kc = default_chunk(B, K) if sample_chunk is None else min(int(sample_chunk), K)
    return [(k0, min(Kc, K - k0)) for k0 in range(0, K, Kc)]


def chunk_seeds(seeds, k0, Kc):
    """uint64 [B * Kc], row b * Kc + kk = seeds[b][k0 + kk]."""
    return np.asarray([row[k0 + kk] for row in seeds for kk in range(Kc)], dtype=np.uint64)


def better(new, old, higher):
    """Does the score `new` beat `old`?  A NaN never beats anything; a number beats a NaN; a tie keeps the earlier sample."""
    if math.isnan(new):
        return False
    if math.isnan(old):
        return True
    return new > old if higher else new < old


def argbest(scores, higher):
    """The index of the best score of a row: ties go to the lowest k, a NaN never beats a number, all NaN gives 0."""
    best = 0
    for k in range(1, len(scores)):
        if better(float(scores[k]), float(scores[best]), higher):
            best = k
    return best


# ---- the library calls ------------------------------------------------------------------------------------------------------------
def repeat_images(model, images, K):
    """[B, ...] float32 or uint8 -> [B * K, ...] in the same container family, every image K times in a row (cdc_repeat_images)."""
    h, dev = model._handle(), model.device_index
    u8 = frame.is_uint8(images)
    a = frame._ArgU8(images, dev) if u8 else _Arg(images, dev)
    B = int(a.shape[0])
    per = int(np.prod(a.shape[1:], dtype=np.int64))
    out, po = frame._empty_like(images, (B * K,) + tuple(int(d) for d in a.shape[1:]), u8)
    _lib.check(h, _lib.lib().cdc_repeat_images(h, a.ptr, po, B, int(K), per, 1 if u8 else 4, a.mem, _current_stream(a.mem)))
    return out


def decode_samples(model, context, seeds, B, Kc, H, W, gamma, eta, pred, clip, solver):
    """One cdc_decode_samples call: context pyramid of B images, seeds uint64 [B * Kc] -> [B * Kc, 3, H, W] like context[0]."""
    h, dev = model._handle(), model.device_index
    actx = [_Arg(c, dev) for c in context]
    mem = actx[0].mem
    if any(c.mem != mem for c in actx):
        raise _lib.CdcError("context tensors must all be host or all be on the model's device")
    ptrs = (ctypes.c_void_p * len(actx))(*[c.ptr for c in actx])
    out, optr, omem = _result_like(context[0], (B * Kc, 3, H, W), dev)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    _lib.check(h, _lib.lib().cdc_decode_samples(h, 0.0 if gamma is None else float(gamma), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                float(eta), ptrs, len(actx), optr, B, Kc, H, W, pred, clip, int(solver), mem,
                                                _current_stream(mem)))
    return out


def fold_moments(model, chunk, B, Kc, count_before, mean, m2, finish):
    """cdc_sample_moments: the chunk [B * Kc, ...] into the running mean / m2 [B, ...] (m2 may be None), all in one memory space."""
    h, dev = model._handle(), model.device_index
    a, am = _Arg(chunk, dev), _Arg(mean, dev)
    a2 = None if m2 is None else _Arg(m2, dev)
    if am.ptr != _ptr(mean) or (a2 is not None and a2.ptr != _ptr(m2)):
        raise _lib.CdcError("the accumulators must be contiguous float32 arrays (they are updated in place)")
    per = int(np.prod(am.shape[1:], dtype=np.int64))
    _lib.check(h, _lib.lib().cdc_sample_moments(h, a.ptr, B, Kc, per, int(count_before), am.ptr, None if a2 is None else a2.ptr,
                                                int(bool(finish)), a.mem, _current_stream(a.mem)))


def select(model, chunk, pick, best, B, Kc):
    """cdc_sample_select: best[b] <- chunk[b * Kc + pick[b]] where pick[b] >= 0, in place."""
    h, dev = model._handle(), model.device_index
    a, ab = _Arg(chunk, dev), _Arg(best, dev)
    if ab.ptr != _ptr(best):
        raise _lib.CdcError("best must be a contiguous float32 array (it is updated in place)")
    per = int(np.prod(ab.shape[1:], dtype=np.int64))
    pk = (ctypes.c_int * B)(*[int(p) for p in pick])
    _lib.check(h, _lib.lib().cdc_sample_select(h, a.ptr, pk, ab.ptr, B, Kc, per, a.mem, _current_stream(a.mem)))


def _ptr(t):
    return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data
