"""Host-side mirror of the reference denoising U-Net interface, backed by libcdc_hip.so.

Same constructor arguments, `state_dict` key names, `load_state_dict`, `.to()`, `.eval()` and
`forward(x, time, context)` as `Unet` in xparam/modules/unet.py:18-135 (and
epsilonparam/modules/unet.py:17-124, which lacks `embd_type`), so that test_xparam.py /
test_epsilonparam.py style drivers run unchanged.  All arithmetic happens in hand-written HIP
kernels behind the C-ABI; this file only moves pointers.
"""
import ctypes

import numpy as np

from . import _lib


def _is_torch(t):
    return type(t).__module__.startswith("torch")


def _as_host_f32(t):
    if _is_torch(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


class _Arg:
    """Uniform view of a numpy / torch-cpu / torch-cuda float32 tensor as (pointer, mem kind)."""

    def __init__(self, t, device_index):
        self.keep = None
        if _is_torch(t) and t.is_cuda:
            import torch
            if t.device.index != device_index:
                raise _lib.CdcError(f"tensor on cuda:{t.device.index}, model on cuda:{device_index}")
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            self.keep = t
            self.ptr = t.data_ptr()
            self.mem = _lib.CDC_MEM_DEVICE
            self.shape = tuple(t.shape)
        else:
            a = _as_host_f32(t)
            self.keep = a
            self.ptr = a.ctypes.data
            self.mem = _lib.CDC_MEM_HOST
            self.shape = a.shape


def _result_like(proto, shape, device_index):
    """Allocate the output in the same container family as `proto`."""
    if _is_torch(proto):
        import torch
        if proto.is_cuda:
            t = torch.empty(shape, dtype=torch.float32, device=proto.device)
            return t, t.data_ptr(), _lib.CDC_MEM_DEVICE
        t = torch.empty(shape, dtype=torch.float32)
        return t, t.data_ptr(), _lib.CDC_MEM_HOST
    a = np.empty(shape, np.float32)
    return a, a.ctypes.data, _lib.CDC_MEM_HOST


def _current_stream(mem):
    if mem == _lib.CDC_MEM_DEVICE:
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


class Unet:
    def __init__(self, dim, out_dim=None, dim_mults=(1, 2, 4, 8), context_dim_mults=(1, 2, 3, 3),
                 channels=3, context_channels=3, with_time_emb=True, embd_type="01", device=0):
        if not with_time_emb:
            raise NotImplementedError("with_time_emb=False is not on the decode path")
        if embd_type != "01":
            raise NotImplementedError('only embd_type="01" (unet.py:39-41) is implemented')
        self.dim = dim
        self.channels = channels
        self.context_channels = context_channels
        self.out_dim = channels if out_dim is None else out_dim
        self.dim_mults = tuple(dim_mults)
        self.context_dim_mults = tuple(context_dim_mults)
        self.embd_type = embd_type
        self.training = False
        dim_mults, context_dim_mults, out_dim = self.dim_mults, self.context_dim_mults, self.out_dim

        def config():
            cfg = _lib.UnetConfig()
            cfg.dim, cfg.channels, cfg.context_channels, cfg.out_dim = dim, channels, context_channels, out_dim
            cfg.n_dim_mults, cfg.n_context_dim_mults = len(dim_mults), len(context_dim_mults)
            for i, m in enumerate(dim_mults):
                cfg.dim_mults[i] = m
            for i, m in enumerate(context_dim_mults):
                cfg.context_dim_mults[i] = m
            return cfg
        self._chains = 0

        def setup(h):        # (a handle created anew on another device keeps the setting)
            if self._chains:
                _lib.check(h, _lib.lib().cdc_set_decode_chains(h, self._chains))
        self._lh = _lib.Handle("cdc_create", config, _lib.device_index_of(device), setup)

    # ---- handle management (_lib.Handle) --------------------------------------------------
    def _handle(self):
        return self._lh.ptr

    _h = property(lambda self: self._lh.raw)

    @_h.setter
    def _h(self, h):
        """For a caller that has destroyed the handle itself (cdc_destroy(un._h); un._h = None): it must not be destroyed twice."""
        self._lh.raw = h

    _finalized = property(lambda self: self._lh.finalized)
    device_index = property(lambda self: self._lh.device_index)

    def status(self):
        """Arithmetic mode and range-guard counters of the library handle (see _lib.handle_status)."""
        return self._lh.status()

    @property
    def range_faults(self):
        return self.status()["range_faults"]

    def set_decode_chains(self, n):
        """cdc_set_decode_chains: 0 the library's rule, 1 a batch is always one chain (the one-chain bits), 2 two half-batch chains
        on two streams whenever the call allows it."""
        _lib.check(self._handle(), _lib.lib().cdc_set_decode_chains(self._handle(), int(n)))
        self._chains = int(n)
        return self

    def decode_chains(self, B, H, W):
        """cdc_decode_chains: how many chains (1 or 2) a plain decode of B images of H x W runs on this model as it is set."""
        return int(_lib.lib().cdc_decode_chains(self._handle(), int(B), int(H), int(W)))

    def to(self, device):
        """Another device: the handle goes now; the next use creates it there, with the parameters loaded and final as they were."""
        self._lh.move(_lib.device_index_of(device))
        return self

    def eval(self):
        self.training = False
        return self

    # ---- parameters -----------------------------------------------------------------------
    def manifest(self):
        """[(name, shape)] in the order of the reference Unet.state_dict()."""
        return self._lh.manifest()

    def load_state_dict(self, state_dict, strict=True):
        names = [n for n, _ in self.manifest()]
        missing = [n for n in names if n not in state_dict]
        unexpected = [k for k in state_dict if k not in names]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Unet: missing {missing[:3]}"
                               f"{'...' if len(missing) > 3 else ''}, unexpected {unexpected[:3]}")
        for n in names:
            if n in state_dict:
                self._lh.load(n, _as_host_f32(state_dict[n]))
        self._lh.finalize()
        return self

    def state_dict(self):
        return dict(self._lh.tensors)

    # ---- forward --------------------------------------------------------------------------
    def forward(self, x, time=None, context=None):
        """Unet.forward (unet.py:131-135): x [B,C,H,W], time [B,1] or [B], context list."""
        L, h = _lib.lib(), self._handle()
        if not self._finalized:
            raise _lib.CdcError("load_state_dict() has not been called")
        if time is None or context is None:
            raise _lib.CdcError("time and context are required on the decode path")
        ax = _Arg(x, self.device_index)
        B, C, H, W = ax.shape
        mem = ax.mem
        if mem == _lib.CDC_MEM_DEVICE:
            at = _Arg(time.reshape(-1) if _is_torch(time) else time, self.device_index)
            actx = [_Arg(c, self.device_index) for c in context]
            if at.mem != mem or any(c.mem != mem for c in actx):
                raise _lib.CdcError("x, time and context must live on the same device")
        else:
            at = _Arg(_as_host_f32(time).reshape(-1), self.device_index)
            actx = [_Arg(_as_host_f32(c), self.device_index) for c in context]
        ptrs = (ctypes.c_void_p * max(len(actx), 1))(*[c.ptr for c in actx])
        out, optr, _ = _result_like(x, (B, self.out_dim, H, W), self.device_index)
        _lib.check(h, L.cdc_unet_forward(h, ax.ptr, at.ptr, ptrs, len(actx), optr, B, H, W, mem,
                                         _current_stream(mem)))
        return out

    __call__ = forward

    def tap(self, name):
        """Intermediate activation of the last forward / DDIM iteration by the reference's module path
        ("downs.0.0", "downs.1.3", "mid_block1", "ups.0", ...): what a forward hook on that module records."""
        import numpy as np
        L, h = _lib.lib(), self._handle()
        shape = (ctypes.c_int64 * 4)()
        _lib.check(h, L.cdc_unet_tap(h, name.encode(), None, shape))
        out = np.empty(tuple(shape), np.float32)
        _lib.check(h, L.cdc_unet_tap(h, name.encode(), out.ctypes.data, shape))
        return out
