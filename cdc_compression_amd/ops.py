"""Single-operator entry points of libcdc_hip.so (the same kernels the U-Net program launches);
numpy in / numpy out, torch.nn.functional semantics.  Used by the parity tests."""
import ctypes

import numpy as np

from . import _lib


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return None if a is None else a.ctypes.data


class Ops:
    def __init__(self, device=0):
        def config():
            cfg = _lib.UnetConfig()
            cfg.dim, cfg.channels, cfg.context_channels, cfg.out_dim = 32, 3, 3, 3
            cfg.n_dim_mults = 1
            cfg.dim_mults[0] = 1
            cfg.n_context_dim_mults = 1
            cfg.context_dim_mults[0] = 1
            return cfg
        self._lh = _lib.Handle("cdc_create", config, _lib.device_index_of(device))
        self._h = self._lh.ptr
        self._first_op = 0

    def _mark(self):
        self._first_op = _lib.lib().cdc_prof_num_ops(self._h)

    def last_labels(self):
        """The lines of the per-op table (include/cdc_hip.h: cdc_prof_op) of the ops the last conv2d / conv_transpose2d call planned, in
        launch order: which kernel family ran it (csrc/cdc_state.h: op_label).  A call repeated by the range guard lists them twice."""
        L, out = _lib.lib(), []
        for i in range(self._first_op, L.cdc_prof_num_ops(self._h)):
            lab = ctypes.c_char_p()
            L.cdc_prof_op(self._h, i, ctypes.byref(lab), None, None, None)
            out.append(lab.value.decode())
        return out

    def status(self):
        """{"arith", "range_faults", "nonfinite_results"} of this handle (range guard of the fp16 arithmetic)."""
        return self._lh.status()

    def stress(self, repeats):
        """Every following operator call launches its program `repeats` more times and counts the executions whose result is not
        bit-identical to the first one (on the device; include/cdc_hip.h: cdc_op_stress).  0 turns it off."""
        _lib.check(self._h, _lib.lib().cdc_op_stress(self._h, int(repeats)))

    def stress_result(self):
        """(executions compared, executions that differed) of the last operator call."""
        n, d = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._h, _lib.lib().cdc_op_stress_result(self._h, ctypes.byref(n), ctypes.byref(d)))
        return n.value, d.value

    def prof(self, on=True):
        L = _lib.lib()
        L.cdc_prof_reset(self._h)
        L.cdc_prof_enable(self._h, 1 if on else 0)

    def prof_total_ms(self):
        """(total ms, launches, flops) accumulated since prof(True) over all kernel classes."""
        L = _lib.lib()
        tot, n, fl = 0.0, 0, 0.0
        for c in range(L.cdc_prof_num_classes()):
            ms, k, f, b = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            L.cdc_prof_get(self._h, c, ctypes.byref(ms), ctypes.byref(k), ctypes.byref(f), ctypes.byref(b))
            tot += ms.value; n += k.value; fl += f.value
        return tot, n, fl

    def conv2d(self, x, w, b=None, stride=1, padding=0, ln_g=None, ln_b=None, relu=False, shift=None,
               resid=None):
        x, w, b, ln_g, ln_b, shift, resid = map(_c, (x, w, b, ln_g, ln_b, shift, resid))
        B, Cin, H, W = x.shape
        Cout, _, KH, KW = w.shape
        Ho = (H + 2 * padding - KH) // stride + 1
        Wo = (W + 2 * padding - KW) // stride + 1
        y = np.empty((B, Cout, Ho, Wo), np.float32)
        if ln_g is not None:
            ln_g, ln_b = ln_g.reshape(-1), ln_b.reshape(-1)
        self._mark()
        _lib.check(self._h, _lib.lib().cdc_op_conv2d(
            self._h, _p(x), _p(w), _p(b), _p(y), B, Cin, H, W, Cout, KH, KW, stride, padding, _p(ln_g),
            _p(ln_b), int(relu), _p(shift), _p(resid)))
        return y

    def conv_transpose2d(self, x, w, b=None):
        x, w, b = map(_c, (x, w, b))
        B, Cin, H, W = x.shape
        Cout = w.shape[1]
        y = np.empty((B, Cout, 2 * H, 2 * W), np.float32)
        self._mark()
        _lib.check(self._h, _lib.lib().cdc_op_conv_transpose2d(self._h, _p(x), _p(w), _p(b), _p(y), B,
                                                               Cin, H, W, Cout))
        return y

    def chan_layernorm(self, x, g, b):
        x, g, b = _c(x), _c(g).reshape(-1), _c(b).reshape(-1)
        B, C, H, W = x.shape
        y = np.empty_like(x)
        _lib.check(self._h, _lib.lib().cdc_op_chan_layernorm(self._h, _p(x), _p(g), _p(b), _p(y), B, C,
                                                             H * W))
        return y

    def chan_layernorm_ex(self, x, g=None, b=None, relu=False, shift=None, resid=None, in_place=False, want_y=True, want_stats=False):
        """The stand-alone LayerNorm with everything a program asks of it (include/cdc_hip.h: cdc_op_chan_layernorm_ex).
        x [B, C, H, W], or [K, B, C, H, W]: K split-K slices summed on load.  -> y, (mean, rstd) [B, H, W] or (y, mean, rstd):
        want_y=False is the statistics-only pass over x; with y the statistics are those of the final values."""
        x = _c(x)
        K = x.shape[0] if x.ndim == 5 else 1
        B, C, H, W = x.shape[-4:]
        g, b, shift, resid = (None if a is None else _c(a).reshape(-1) for a in (g, b, shift, resid))
        y = np.empty((B, C, H, W), np.float32) if want_y else None
        want_stats = want_stats or not want_y
        sm, sr = (np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)) if want_stats else (None, None)
        _lib.check(self._h, _lib.lib().cdc_op_chan_layernorm_ex(self._h, _p(x), K, _p(g), _p(b), int(bool(relu)), _p(shift), _p(resid),
                                                                int(bool(in_place)), _p(y), _p(sm), _p(sr), B, C, H * W))
        if not want_y:
            return sm, sr
        return (y, sm, sr) if want_stats else y

    def ln_form(self, B, C, HW, nparts=1, aligned16=True):
        """(kind, width, np, img_major) of the LayerNorm launch over B images of C channels and HW pixels with `nparts` slices: kind 0
        ln_kernel (width = threads per workgroup), 1 ln_kernel_sliced (width = PL), 2 ln_kernel_vec (width = COLS); np 0 = the
        run-time slice loop.  Launches nothing (include/cdc_hip.h: cdc_op_ln_form)."""
        v = [ctypes.c_int() for _ in range(4)]
        _lib.check(self._h, _lib.lib().cdc_op_ln_form(self._h, int(B), int(C), int(HW), int(nparts), int(bool(aligned16)),
                                                      *[ctypes.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def sum_slices(self, x):
        """x [parts, B, n] -> [B, n]: the split-K sum pass (slice order), alone (include/cdc_hip.h: cdc_op_sum_slices)."""
        x = _c(x)
        parts, B, n = x.shape
        y = np.empty((B, n), np.float32)
        _lib.check(self._h, _lib.lib().cdc_op_sum_slices(self._h, _p(x), parts, _p(y), B, n))
        return y

    def linear_attention(self, x, norm_g, norm_b, w_qkv, w_out, b_out):
        x, norm_g, norm_b, w_qkv, w_out, b_out = map(_c, (x, norm_g, norm_b, w_qkv, w_out, b_out))
        B, C, H, W = x.shape
        y = np.empty_like(x)
        _lib.check(self._h, _lib.lib().cdc_op_linear_attention(
            self._h, _p(x), _p(norm_g.reshape(-1)), _p(norm_b.reshape(-1)), _p(w_qkv), _p(w_out),
            _p(b_out), _p(y), B, C, H, W))
        return y

    def gdn(self, x, beta, gamma, inverse=False):
        """GDN1.forward (epsilonparam network_components.py:381-412) with the raw parameters beta [C], gamma [C, C]:
        y = x / (beta' + gamma' |x|), or x * (...) when inverse."""
        x, beta, gamma = _c(x), _c(beta).reshape(-1), _c(gamma)
        B, C, H, W = x.shape
        if beta.shape != (C,) or gamma.shape != (C, C):
            raise ValueError(f"beta {beta.shape} / gamma {gamma.shape} do not belong to {C} channels")
        y = np.empty_like(x)
        _lib.check(self._h, _lib.lib().cdc_op_gdn(self._h, _p(x), _p(beta), _p(gamma), _p(y), B, C, H * W, int(bool(inverse))))
        return y

    def gdn_workgroups(self, B, HW):
        """(workgroups per image, 64-pixel tiles per image) of the grid `gdn` launches for B images of HW pixels: each workgroup walks
        the tiles w, w + per_image, ...  Launches nothing (include/cdc_hip.h: cdc_op_gdn_workgroups)."""
        per_image, tiles = ctypes.c_int(), ctypes.c_int()
        _lib.check(self._h, _lib.lib().cdc_op_gdn_workgroups(self._h, int(B), int(HW), ctypes.byref(per_image), ctypes.byref(tiles)))
        return per_image.value, tiles.value
