"""Host-side mirror of the DECODER half of the reference context model, backed by libcdc_hip.so.

`ResnetCompressor` (xparam/modules/compress_modules.py:110-177) and `BigCompressor`
(epsilonparam/modules/compress_modules.py:112-185) keep the reference constructors' argument names;
`decode(q_latent)` (compress_modules.py:68-74) -- the synthesis transform that turns the transmitted latents
into the context pyramid of the denoising U-Net -- is SURVEY section 8f row 1; `encode(images)` / `forward(images)`
(analysis transform + hyper encoder + quantisers, :43-66, :92-103) are row 3, so that a whole
`GaussianDiffusion.compress()` runs on the GPU with no reference module in the loop.  `load_state_dict` accepts the
reference compressor's full state_dict: `dec.*` is mandatory, `hyper_dec.*` / `prior.*` / `enc.*` / `hyper_enc.*`
are taken when present (each enables the corresponding entry points: `hyper_decode` + `bpp`, `encode` + `forward`).

Decode side of the hyperprior: `hyper_decode(q_hyper_latent)` runs
`hyper_dec` (compress_modules.py:54-59) and returns `(mean, scale.clamp(min=0.1))`; `dequantize(x, offset)`
is `quantize(x, "dequantize", offset)` (utils.py:72-85).

Variable bitrate (`BigCompressor(vbr=True)`, epsilonparam compress_modules.py:125-184): every entry point that runs a
VBRCondition site takes the rate as `cond` / `bitrate_scale` -- a numpy array or torch tensor of 1 (broadcast) or B
elements, as the reference's `cond.reshape(-1, 1, 1, 1)` accepts -- and the streams of `compress_to_bytes` carry each
image's rate (container version 4), so `decompress_from_bytes` needs none.

Images of any size (cdc_compression_amd.frame states the rule): `forward`, `encode` and `compress_to_bytes` take `[B, 3, H, W]` of
any `H, W >= 1`, float32 in [-1, 1] or uint8, and run on the frame padded at the bottom / right by edge replication to this model's
multiple (`padded_size`).  Every latent and `forward()["output"]` -- the context pyramid the denoising U-Net consumes -- belong to
that PADDED frame; `bpp` counts bits over the original `H * W`; the streams record `H x W` (container version 5 / 6) unless the
image already is its own frame, in which case they are the version-3 / -4 streams they always were.  `analysis`, `decode`,
`hyper_decode` mirror the reference's modules one to one and keep requiring frame sizes.

Rate control in the encoder (no reference counterpart; include/cdc_hip.h: cdc_set_rdo states the decision): `rdo=mu` -- the price of a
bit, a scalar or B values -- makes the quantiser code, per latent symbol, the neighbour towards the mean in place of the nearest integer
where mu * (bits saved) exceeds the squared error added.  `encode`, `forward`, `latents_to_bytes` and `compress_to_bytes` take it;
`compress_to_bytes(target_bpp= | max_bytes=)` finds mu per image from `rate_sweep`'s one-pass curve.  The streams keep their format and
the decoder never learns mu; `rdo=None` runs what always ran.  What the moves do to decoded images of trained weights is unmeasured.

Region-of-interest coding (include/cdc_hip.h: cdc_set_rdo_map): with any of the three, `price_map=` -- a map in pixels at the image's
own size -- or `price_cells=` -- its cells on the latent grid, `price_cells()` -- makes the price of a bit mu * map per latent position:
0 protects a region, values above 1 make one pay.  The decision stays separable, so the streams and the decoder are untouched, and
`target_bpp` / `max_bytes` search the base mu under the map.  What a map does to decoded images of trained weights is unmeasured too.
"""
import ctypes

import numpy as np

from . import _lib, frame
from .unet import _Arg, _as_host_f32, _current_stream, _is_torch, _result_like


class NormalDistribution:
    """Holder with the attribute names of utils.py:134-145 (`loc`, `scale`, `mean`)."""

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale

    @property
    def mean(self):
        return self.loc


# ---- rate-distortion optimised quantisation: the host side of rate targeting (include/cdc_hip.h: cdc_set_rdo states the decision) ----
RDO_MAX_LADDER = 32                                                    # cdc_entropy_rate_sweep prices at most this many mu in one pass
RDO_LADDER = np.float32(2.0) ** np.arange(-8, 9, dtype=np.float32)      # the default ladder: mu = 2^-8 ... 2^8 in 17 steps
RDO_REFINE_STEPS = 17


def rdo_values(rdo, B, what="rdo"):
    """rdo / a ladder -> float32 host vector, checked before the library is touched: finite, >= 0, and 1 or B values (B=None: a ladder
    of 1 .. RDO_MAX_LADDER values)."""
    r = np.ascontiguousarray(_as_host_f32(rdo).reshape(-1))
    if B is None:
        if not 1 <= r.size <= RDO_MAX_LADDER:
            raise ValueError(f"{what}: a ladder of {r.size} values (1 .. {RDO_MAX_LADDER} expected)")
    elif r.size not in (1, B):
        raise ValueError(f"{what} has {r.size} values for a batch of {B} (1 or {B} expected)")
    if not np.all(np.isfinite(r)) or np.any(r < 0):
        raise ValueError(f"{what}={r.tolist()}: every mu must be finite and >= 0")
    return r


def segment_positions(segment, cell):
    """segment= -> the side of a stream segment in latent positions (cdc_entropy_set_segments), checked before the library is touched.
    segment is in image pixels, like tile=: an int > 0 that is a multiple of `cell`, the pixels of a latent position; None -> 0, the
    unsegmented streams."""
    if segment is None:
        return 0
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)):
        raise ValueError(f"segment={segment!r}: an int in image pixels expected")
    seg = int(segment)
    if seg <= 0 or seg % cell:
        raise ValueError(f"segment={seg}: a positive multiple of the {cell} pixels of a latent position expected")
    if seg // cell > 65535:
        raise ValueError(f"segment={seg}: at most {65535 * cell} pixels ({65535} latent positions)")
    return seg // cell


def hyper_group_channels(hyper_groups, channels, segment):
    """hyper_groups=G -> cg, the hyper channels per group (cdc_entropy_set_hyper_groups), checked before the library is touched.  G is
    the number of groups asked for, an int in 1 .. `channels`; cg = ceil(channels / G), and the stream then holds ceil(channels / cg)
    groups, which can be fewer than G (40 channels, G = 16: cg = 3, 14 groups).  Only with segment=; None -> 0, one hyper section."""
    if hyper_groups is None:
        return 0
    if isinstance(hyper_groups, bool) or not isinstance(hyper_groups, (int, np.integer)):
        raise ValueError(f"hyper_groups={hyper_groups!r}: an int expected, the number of groups")
    G = int(hyper_groups)
    if G < 1 or G > channels:
        raise ValueError(f"hyper_groups={G}: 1 .. {channels} expected (the model has {channels} hyper channels)")
    if segment is None:
        raise ValueError("hyper_groups needs segment=: grouped streams are segmented streams (container versions 19 - 22)")
    return -(-channels // G)


def rdo_exclusive(rdo=None, target_bpp=None, max_bytes=None):
    """rdo, target_bpp and max_bytes exclude each other."""
    given = [n for n, v in (("rdo", rdo), ("target_bpp", target_bpp), ("max_bytes", max_bytes)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"{' and '.join(given)} exclude each other: give one of rdo, target_bpp, max_bytes")


def price_map_values(price_map, B, H, W):
    """A pixel-domain price map -> float32 [n, H, W] (NumPy, or a torch tensor on its own device), checked before the library is
    touched.  Accepted: [H, W], [1, H, W], [B, H, W] or [B, 1, H, W] at the image's own size, float32 or bool (cast), finite and >= 0.
    B=None: any number of rows."""
    t = price_map
    torch_like = _is_torch(t)
    if torch_like:
        import torch
        if t.dtype == torch.bool:
            t = t.to(torch.float32)
        ok = t.dtype == torch.float32
    else:
        t = np.asarray(t)
        if t.dtype == np.bool_:
            t = t.astype(np.float32)
        ok = t.dtype == np.float32
    if not ok:
        raise ValueError(f"price_map must be float32 or bool, got {t.dtype}")
    shape = tuple(int(d) for d in t.shape)
    if len(shape) == 4 and shape[1] == 1:
        shape = (shape[0],) + shape[2:]
    elif len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1:] != (int(H), int(W)) or (B is not None and shape[0] not in (1, B)) or shape[0] < 1:
        raise ValueError(f"price_map of shape {tuple(price_map.shape)}: [H, W], [1, H, W], [B, H, W] or [B, 1, H, W] with "
                         f"H x W = {H} x {W}" + ("" if B is None else f" and B = {B}") + " expected")
    t = t.reshape(shape)
    if torch_like:
        import torch
        good = bool(torch.isfinite(t).all()) and bool((t >= 0).all())
        t = t.contiguous()
    else:
        good = bool(np.all(np.isfinite(t))) and bool(np.all(t >= 0))
        t = np.ascontiguousarray(t)
    if not good:
        raise ValueError("price_map: every value must be finite and >= 0")
    return t


def price_cells_values(price_cells, B, grid=None):
    """Prices already on the latent grid -> float32 host array [n, gh, gw], n = 1 or B (B=None: any), checked before the library is
    touched: [gh, gw] or [n, gh, gw], float32 or bool, finite and >= 0; grid=(gh, gw): the grid they must lie on."""
    c = price_cells.detach().cpu().numpy() if _is_torch(price_cells) else np.asarray(price_cells)
    if c.dtype == np.bool_:
        c = c.astype(np.float32)
    if c.dtype != np.float32:
        raise ValueError(f"price_cells must be float32 or bool, got {c.dtype}")
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or min(c.shape) < 1 or (B is not None and c.shape[0] not in (1, B)) or \
            (grid is not None and tuple(c.shape[1:]) != tuple(grid)):
        raise ValueError(f"price_cells of shape {tuple(price_cells.shape)}: [gh, gw] or [n, gh, gw]" +
                         ("" if grid is None else f" on the latent grid {tuple(grid)}") + ("" if B is None else f" with n = 1 or {B}") + " expected")
    if not np.all(np.isfinite(c)) or np.any(c < 0):
        raise ValueError("price_cells: every value must be finite and >= 0")
    return np.ascontiguousarray(c)


def price_args(price_map, price_cells, B, hw, rated):
    """The price-map arguments of an entry point, checked before the library is touched -> None, ("map", float32 [n, H, W]) or
    ("cells", float32 host [n, gh, gw]).  hw: the image's own size; rated: one of rdo / target_bpp / max_bytes is given (a map steers
    a price: without one there is nothing to steer)."""
    if price_map is None and price_cells is None:
        return None
    if price_map is not None and price_cells is not None:
        raise ValueError("price_map and price_cells exclude each other: the map in pixels, or its cells on the latent grid")
    if not rated:
        raise ValueError("price_map / price_cells need one of rdo, target_bpp, max_bytes: the map scales the price of a bit")
    if price_map is not None:
        return "map", price_map_values(price_map, B, hw[0], hw[1])
    return "cells", price_cells_values(price_cells, B)


def _cells_row(cells, b):
    """Image b's own row of a price map on the latent grid (None stays None)."""
    return None if cells is None else cells[b:b + 1] if cells.shape[0] > 1 else cells


def rdo_select(cost, target):
    """One row of a sweep table -> (j, met).  cost[j]: the estimated cost at ladder entry j, non-increasing along an ascending
    ladder; j is the first entry whose cost is <= target (the smallest mu that meets it).  None does: (last entry, False)."""
    cost = np.asarray(cost, np.float64).reshape(-1)
    hit = np.nonzero(cost <= float(target))[0]
    return (int(hit[0]), True) if hit.size else (cost.size - 1, False)


def rdo_refine_ladder(lo, hi, steps=RDO_REFINE_STEPS):
    """The refining ladder between two neighbouring entries lo < hi of a ladder: `steps` float32 values from lo to hi inclusive,
    geometric (linear when lo = 0, the entry below the first positive mu), ascending, without repeats."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not (0 <= lo < hi and np.isfinite(hi)) or not 2 <= steps <= RDO_MAX_LADDER:
        raise ValueError(f"rdo_refine_ladder: lo={lo}, hi={hi}, steps={steps}")
    v = np.linspace(lo, hi, steps) if lo == 0 else np.geomspace(lo, hi, steps)
    v = v.astype(np.float32)
    v[0], v[-1] = lo, hi
    return np.unique(v)


def _enable_vbr(h):
    """setup of a compressor handle of a VBR model: the manifest with the VBRCondition sites."""
    rc = _lib.lib().cdc_enable_vbr(h)
    if rc != 0:
        raise _lib.CdcError(f"cdc_enable_vbr failed ({rc}): {_lib.lib().cdc_last_error(h).decode()}")


class _ContextDecoder:
    _up_index = 1
    _ctxdec_create = "cdc_ctxdec_create"        # the library's constructors of this model's context-decoder / encoder handles
    _encoder_create = "cdc_encoder_create"

    def __init__(self, dim, dim_mults, rev_mults, hyper_dims_mults, channels, out_channels, device=0, vbr=False):
        self.vbr = bool(vbr)
        self.dim = dim
        self.dim_mults, self.hyper_dims_mults, self.channels = tuple(dim_mults), tuple(hyper_dims_mults), channels
        self.rev_mults = tuple(rev_mults)
        self.out_channels = out_channels
        self.reversed_dims = [dim * m for m in self.rev_mults] + [out_channels]
        # compress_modules.py:26-31
        self.reversed_hyper_dims = list(reversed([dim * self.dim_mults[-1] * 2] + [dim * m for m in self.hyper_dims_mults]))
        self.training = False
        self._hyper_finalized = False
        self._prior_loaded = False
        self._medians = None
        self._enc_finalized = False
        # the three library handles (_lib.Handle); their closures hold values, not self: no reference cycle delays cdc_destroy
        index, rev, dm, hm, hyper_dims = self._up_index, self.rev_mults, self.dim_mults, self.hyper_dims_mults, self.reversed_hyper_dims
        multiple, vbr_setup = self.frame_multiple, _enable_vbr if self.vbr else None

        def dec_config():
            cfg = _lib.CtxdecConfig()
            cfg.dim, cfg.out_channels, cfg.up_index = dim, out_channels, index
            cfg.n_rev_mults = len(rev)
            for i, m in enumerate(rev):
                cfg.rev_mults[i] = m
            return cfg

        def hyper_config():
            cfg = _lib.HyperdecConfig()
            cfg.n_layers = len(hyper_dims) - 1
            for i, d in enumerate(hyper_dims):
                cfg.dims[i] = d
            return cfg

        def hyper_setup(h):
            if vbr_setup:
                vbr_setup(h)
            # image pixels per hyper-latent position (the streams of images that are not their own frame need it)
            _lib.check(h, _lib.lib().cdc_entropy_set_image_scale(h, multiple))

        def enc_config():
            cfg = _lib.EncoderConfig()
            cfg.dim, cfg.channels, cfg.down_index = dim, channels, index
            cfg.n_dim_mults, cfg.n_hyper_mults = len(dm), len(hm)
            for i, m in enumerate(dm):
                cfg.dim_mults[i] = m
            for i, m in enumerate(hm):
                cfg.hyper_mults[i] = m
            return cfg
        dev = _lib.device_index_of(device)
        self._dec = _lib.Handle(self._ctxdec_create, dec_config, dev, vbr_setup)
        self._hyper = _lib.Handle("cdc_hyperdec_create", hyper_config, dev, hyper_setup)
        self._enc = _lib.Handle(self._encoder_create, enc_config, dev, vbr_setup)

    def _handle(self):
        return self._dec.ptr

    def _hyper_handle(self):
        return self._hyper.ptr

    def _enc_handle(self):
        return self._enc.ptr

    _h = property(lambda self: self._dec.raw)
    _hh = property(lambda self: self._hyper.raw)
    _eh = property(lambda self: self._enc.raw)
    _finalized = property(lambda self: self._dec.finalized)
    device_index = property(lambda self: self._dec.device_index)

    def status(self):
        """Per library handle (context decoder, hyper decoder, encoder): arithmetic mode and range-guard counters."""
        return {"dec": self._dec.status(), "hyper_dec": self._hyper.status(), "enc": self._enc.status()}

    @property
    def range_faults(self):
        return sum(v["range_faults"] for v in self.status().values())

    # ---- variable bitrate ---------------------------------------------------------------------
    def _rates(self, cond, B):
        """cond / bitrate_scale -> float32 host vector of 1 or B rates (VBR model), None (fixed-rate model)."""
        if not self.vbr:
            if cond is not None:
                raise NotImplementedError(f"{type(self).__name__}(vbr=False) takes no bitrate conditioning (cond / bitrate_scale)")
            return None
        if cond is None:
            raise ValueError(f"{type(self).__name__}(vbr=True) needs a bitrate_scale (cond): 1 or B values, e.g. in [0, 1]")
        r = np.ascontiguousarray(_as_host_f32(cond).reshape(-1))
        if r.size not in (1, B):
            raise ValueError(f"bitrate_scale has {r.size} values for a batch of {B} (1 or {B} expected)")
        return r

    def _set_rate(self, h, cond, B):
        r = self._rates(cond, B)
        if r is not None:
            _lib.check(h, _lib.lib().cdc_set_bitrate_scale(h, r.ctypes.data, int(r.size)))

    def to(self, device):
        """Another device: the three handles go now, and nothing else happens here.  The next use of each creates it on the new device
        with its parameters loaded and final as they were, so an error of that device (no such device, out of memory) surfaces at
        that use, not in .to()."""
        for lh in (self._dec, self._hyper, self._enc):
            lh.move(_lib.device_index_of(device))
        return self

    def eval(self):
        self.training = False
        return self

    # ---- parameters -----------------------------------------------------------------------
    def manifest(self):
        """[(name, shape)] of the `dec.*` entries, in the reference's registration order."""
        return self._dec.manifest()

    def load_state_dict(self, state_dict, strict=True):
        """Takes the `dec.*` entries; the encoder / hyperprior entries of a full reference state_dict are
        not this module's.  strict: every `dec.*` key must match the manifest."""
        names = [n for n, _ in self.manifest()]
        missing = [n for n in names if n not in state_dict]
        unexpected = [k for k in state_dict if k.startswith("dec.") and k not in names]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing "
                               f"{missing[:3]}{'...' if len(missing) > 3 else ''}, unexpected {unexpected[:3]}")
        for n in names:
            if n in state_dict:
                self._dec.load(n, _as_host_f32(state_dict[n]))
        self._dec.finalize()
        if any(k.startswith("hyper_dec.") for k in state_dict):
            self.load_hyper_state_dict(state_dict)      # also takes prior.* when present
        if any(k.startswith("enc.") for k in state_dict):
            self.load_encoder_state_dict(state_dict)
        return self

    def state_dict(self):
        return dict(self._dec.tensors)

    # ---- Compressor.decode ------------------------------------------------------------------
    def decode(self, input, cond=None):
        """q_latent [B, reversed_dims[0], h, w] -> [ctx@16h, ctx@8h, ctx@4h, ctx@2h] (finest first).  cond: the bitrate_scale
        of a VBR model (1 or B values)."""
        aq = _Arg(input, self.device_index)
        B, C, hl, wl = aq.shape
        self._rates(cond, B)
        L, h = _lib.lib(), self._handle()
        if not self._finalized:
            raise _lib.CdcError("load_state_dict() has not been called")
        self._set_rate(h, cond, B)
        if C != self.reversed_dims[0]:
            raise _lib.CdcError(f"q_latent has {C} channels, the decoder expects {self.reversed_dims[0]}")
        n = len(self.rev_mults)
        outs, ptrs = [], []
        for i in range(n):                     # outs[0] = finest
            lvl = n - 1 - i
            o, p, _ = _result_like(input, (B, self.reversed_dims[lvl + 1], hl << (lvl + 1), wl << (lvl + 1)),
                                   self.device_index)
            outs.append(o)
            ptrs.append(p)
        arr = (ctypes.c_void_p * n)(*ptrs)
        _lib.check(h, L.cdc_ctxdec_decode(h, aq.ptr, arr, n, B, hl, wl, aq.mem, _current_stream(aq.mem)))
        return outs

    # ---- hyperprior, decode side -----------------------------------------------------------
    def hyper_manifest(self):
        return self._hyper.manifest()

    def load_hyper_state_dict(self, state_dict):
        """`hyper_dec.*` entries of the reference compressor's state_dict."""
        names = [n for n, _ in self.hyper_manifest()]
        missing = [n for n in names if n not in state_dict]
        unexpected = [k for k in state_dict if k.startswith("hyper_dec.") and k not in names]
        if missing or unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}.hyper_dec: missing "
                               f"{missing[:3]}, unexpected {unexpected[:3]}")
        for n in names:
            self._hyper.load(n, _as_host_f32(state_dict[n]))
        # FlexiblePrior (rate estimate only): reference shapes [C,1,1,in,out] / [C,1,1,1,out], singleton axes squeezed
        self._prior_loaded = False
        pk = [k for k in state_dict if k.startswith("prior.affine.") or k.startswith("prior.a.")]
        if pk:
            C = self.reversed_hyper_dims[0]
            for k in pk:
                a = _as_host_f32(state_dict[k])
                a = np.ascontiguousarray(a.reshape((C,) + tuple(d for d in a.shape[3:] if True))
                                         if a.ndim == 5 else a)
                if a.ndim == 3 and not k.endswith(".weight"):
                    a = np.ascontiguousarray(a.reshape(C, -1))
                self._hyper.load(k, a)
            self._prior_loaded = True
        if "prior._medians" in state_dict:
            self._medians = _as_host_f32(state_dict["prior._medians"]).reshape(1, -1, 1, 1)
        self._hyper.finalize()
        self._hyper_finalized = True
        return self

    def hyper_decode(self, q_hyper_latent, scale_min=0.1, cond=None):
        """compress_modules.py:54-59: (mean, scale) of the latent distribution from q_hyper_latent (cond: VBR rate)."""
        L, h = _lib.lib(), self._hyper_handle()
        if not self._hyper_finalized:
            raise _lib.CdcError("load_hyper_state_dict() has not been called")
        aq = _Arg(q_hyper_latent, self.device_index)
        B, C, hh, wh = aq.shape
        self._set_rate(h, cond, B)
        if C != self.reversed_hyper_dims[0]:
            raise _lib.CdcError(f"q_hyper_latent has {C} channels, hyper_dec expects {self.reversed_hyper_dims[0]}")
        up = 2 ** (len(self.reversed_hyper_dims) - 2)       # one stride-2 ConvTranspose2d per hyper_dec layer but the last
        shape = (B, self.reversed_hyper_dims[-1] // 2, hh * up, wh * up)
        mean, pm, _ = _result_like(q_hyper_latent, shape, self.device_index)
        scale, ps, _ = _result_like(q_hyper_latent, shape, self.device_index)
        _lib.check(h, L.cdc_hyperdec_decode(h, aq.ptr, pm, ps, B, hh, wh, ctypes.c_float(scale_min), aq.mem,
                                            _current_stream(aq.mem)))
        return mean, scale

    def dequantize(self, x, offset):
        """quantize(x, "dequantize", offset) (utils.py:72-85)."""
        L, h = _lib.lib(), self._handle()
        ax, ao = _Arg(x, self.device_index), _Arg(offset, self.device_index)
        if ax.mem != ao.mem or ax.shape != ao.shape:
            raise _lib.CdcError("x and offset must have the same shape and live in the same memory")
        out, po, _ = _result_like(x, ax.shape, self.device_index)
        n = 1
        for d in ax.shape:
            n *= d
        _lib.check(h, L.cdc_dequantize(h, ax.ptr, ao.ptr, po, n, ax.mem, _current_stream(ax.mem)))
        return out

    def rate(self, q_hyper_latent, q_latent, mean, scale, image_hw):
        """bits per pixel of already quantised latents: the two likelihood sums of Compressor.bpp
        (compress_modules.py:84-88) on the GPU."""
        L, h = _lib.lib(), self._hyper_handle()
        if not (self._hyper_finalized and self._prior_loaded):
            raise _lib.CdcError("the prior.* tensors have not been loaded (load_state_dict with the full state_dict)")
        args = [_Arg(t, self.device_index) for t in (q_hyper_latent, q_latent, mean, scale)]
        if len({a.mem for a in args}) != 1:
            raise _lib.CdcError("all inputs must live in the same memory")
        B, _, hh, wh = args[0].shape
        up = 2 ** (len(self.reversed_hyper_dims) - 2)       # as in hyper_decode: one stride-2 ConvTranspose2d per hyper_dec layer but the last
        if args[1].shape != (B, self.reversed_hyper_dims[-1] // 2, up * hh, up * wh) or \
                args[2].shape != args[1].shape or args[3].shape != args[1].shape:
            raise _lib.CdcError(f"latent shapes {args[1].shape} do not belong to a {args[0].shape} hyper latent")
        out, po, _ = _result_like(q_hyper_latent, (B,), self.device_index)
        _lib.check(h, L.cdc_bpp(h, args[0].ptr, args[1].ptr, args[2].ptr, args[3].ptr, po, B, hh, wh,
                                int(image_hw[0]), int(image_hw[1]), args[0].mem, _current_stream(args[0].mem)))
        return out

    RATE_MAPS = {"latent": 0, "hyper": 1, "cell": 2, "latent_channels": 3, "hyper_channels": 4}     # name -> output slot of cdc_rate_map

    @property
    def hyper_upsampling(self):
        """Latent positions per hyper-latent position and side (U; 4 as published): one stride-2 ConvTranspose2d per hyper_dec layer
        but the last."""
        return 2 ** (len(self.reversed_hyper_dims) - 2)

    @property
    def rate_map_cell(self):
        """Image pixels per latent position and side: the cell of the maps of `rate_map` / `forward(return_rate_map=True)` (16 as
        published)."""
        return self.frame_multiple // self.hyper_upsampling

    @classmethod
    def _rate_map_names(cls, what):
        """The argument rule of rate_map's `what`, checked before the library is touched -> tuple of names."""
        names = (what,) if isinstance(what, str) else tuple(what)
        bad = [n for n in names if n not in cls.RATE_MAPS]
        if bad or not names:
            raise ValueError(f"rate_map: what={what!r}: names among {tuple(cls.RATE_MAPS)}")
        return names

    def rate_map(self, q_hyper_latent, q_latent, mean, scale, what=("cell",)):
        """Where the bits of `rate()` went (cdc_rate_map; the header states the sums): a dict of float32 maps in bits with the entries
        of `what` among "latent" [B, U h, U w] (the Gaussian prices summed over the channels), "hyper" [B, h, w] (the prior prices
        likewise), "cell" [B, U h, U w] (latent + hyper / U^2 of the position above: the whole rate on the latent grid, one entry per
        `rate_map_cell` x `rate_map_cell` pixels of the padded frame), "latent_channels" [B, CL] and "hyper_channels" [B, CH] (the
        prices summed over the positions).  NumPy arrays or torch tensors, following the inputs, as `rate()`; the same shape checks."""
        names = self._rate_map_names(what)
        L, h = _lib.lib(), self._hyper_handle()
        if not (self._hyper_finalized and self._prior_loaded):
            raise _lib.CdcError("the prior.* tensors have not been loaded (load_state_dict with the full state_dict)")
        args = [_Arg(t, self.device_index) for t in (q_hyper_latent, q_latent, mean, scale)]
        if len({a.mem for a in args}) != 1:
            raise _lib.CdcError("all inputs must live in the same memory")
        B, CH, hh, wh = args[0].shape
        up, CL = self.hyper_upsampling, self.reversed_hyper_dims[-1] // 2
        if CH != self.reversed_hyper_dims[0]:
            raise _lib.CdcError(f"q_hyper_latent has {CH} channels, the prior expects {self.reversed_hyper_dims[0]}")
        if args[1].shape != (B, CL, up * hh, up * wh) or args[2].shape != args[1].shape or args[3].shape != args[1].shape:
            raise _lib.CdcError(f"latent shapes {args[1].shape} do not belong to a {args[0].shape} hyper latent")
        shapes = {"latent": (B, up * hh, up * wh), "hyper": (B, hh, wh), "cell": (B, up * hh, up * wh), "latent_channels": (B, CL),
                  "hyper_channels": (B, CH)}
        out, ptrs = {}, [None] * 5
        for n in names:
            if n not in out:
                out[n], ptrs[self.RATE_MAPS[n]], _ = _result_like(q_hyper_latent, shapes[n], self.device_index)
        _lib.check(h, L.cdc_rate_map(h, args[0].ptr, args[1].ptr, args[2].ptr, args[3].ptr, *ptrs, B, hh, wh, args[0].mem,
                                     _current_stream(args[0].mem)))
        return out

    # ---- region-of-interest coding: a price per latent position (include/cdc_hip.h: cdc_set_rdo_map states the decision) -----------
    def price_cells(self, price_map, size, padded_hw=None):
        """A pixel-domain price map at the image's own size=(H, W) -> its cells, float32 NumPy [n, gh, gw], on the grid `rate_map` uses
        for that image: the latent grid of the padded frame (of `padded_hw` when the U-Net asks for a larger one), `rate_map_cell`
        pixels a side.  cdc_price_cells: a cell is the mean of the map over its pixels inside the image, a cell that lies wholly in
        the padding takes the value of the nearest one that does not.  price_map: as `price_map_values` (any number of rows)."""
        H, W = (int(d) for d in size)
        pm = price_map_values(price_map, None, H, W)
        Hp, Wp = self.padded_size(H, W) if padded_hw is None else (int(d) for d in padded_hw)
        cell = self.rate_map_cell
        if Hp % cell or Wp % cell or Hp < H or Wp < W:
            raise _lib.CdcError(f"padded_hw {(Hp, Wp)} is no frame of a {H} x {W} image for this model")
        gh, gw = Hp // cell, Wp // cell
        L, h = _lib.lib(), self._hyper_handle()
        a = _Arg(pm, self.device_index)
        n = a.shape[0]
        out, po, mem = _result_like(pm, (n, gh, gw), self.device_index)
        _lib.check(h, L.cdc_price_cells(h, a.ptr, n, n, H, W, H, W, cell, gh, gw, po, mem, _current_stream(mem)))
        return out.cpu().numpy() if _is_torch(out) else out

    def _cells_of(self, priced, hw, padded_hw=None):
        """What `price_args` returned -> the cells as a float32 host array [n, gh, gw] on the latent grid of the frame, or None."""
        if priced is None:
            return None
        kind, v = priced
        if kind == "map":
            return self.price_cells(v, hw, padded_hw)
        Hp, Wp = self.padded_size(*hw) if padded_hw is None else padded_hw
        return price_cells_values(v, None, (Hp // self.rate_map_cell, Wp // self.rate_map_cell))

    def _with_map(self, h, cells, call):
        """call() while the hyper-decoder handle holds `cells` as its price map (cdc_set_rdo_map for this call alone)."""
        if cells is None:
            return call()
        L = _lib.lib()
        n, gh, gw = cells.shape
        _lib.check(h, L.cdc_set_rdo_map(h, cells.ctypes.data, n, gh, gw, _lib.CDC_MEM_HOST, None))
        try:
            return call()
        finally:
            L.cdc_set_rdo_map(h, None, 0, 0, 0, _lib.CDC_MEM_HOST, None)

    def bpp(self, shape, state4bpp):
        """Compressor.bpp (compress_modules.py:76-90) in eval mode: quantise with the medians / the predicted
        mean, then the rate of both latents."""
        B, _, H, W = shape
        dist = state4bpp["latent_distribution"]
        mean, scale = (dist.mean, dist.scale) if hasattr(dist, "mean") else dist
        hyper = state4bpp["hyper_latent"]
        q_hyper = self.dequantize(hyper, self._medians_like(hyper))
        # encode(..., rdo=) chose the symbols: "latent" stays the unquantised latent, the rate is that of the symbols chosen
        q_latent = state4bpp["q_latent"] if "q_latent" in state4bpp else self.dequantize(state4bpp["latent"], mean)
        return self.rate(q_hyper, q_latent, mean, scale, (H, W))

    # ---- images of any size ------------------------------------------------------------------
    @property
    def frame_multiple(self):
        """Image pixels per hyper-latent position and side: what H and W of a frame must be multiples of (64 as published)."""
        return 2 ** (len(self.rev_mults) + len(self.reversed_hyper_dims) - 2)

    def padded_size(self, H, W):
        """(Hp, Wp) of the frame an H x W image is coded on (cdc_padded_size of the encoder handle: no hard-coded 64)."""
        return frame.padded_size([self._enc_handle()], H, W)

    def _framed(self, input, padded_hw=None):
        """images [B, 3, H, W] (float32 / uint8, any size) -> (float32 frame, (H, W)).  An image that is its own frame and float32
        passes through untouched.  padded_hw: a larger frame another part of the model asks for (GaussianDiffusion: the U-Net's)."""
        _, _, H, W = frame.image_shape(input)
        Hp, Wp = self.padded_size(H, W)
        if padded_hw is not None:
            if tuple(padded_hw) != self.padded_size(*padded_hw) or padded_hw[0] < Hp or padded_hw[1] < Wp:
                raise _lib.CdcError(f"padded_hw {tuple(padded_hw)} is no frame of a {H} x {W} image for this model (multiple {self.frame_multiple})")
            Hp, Wp = padded_hw
        if (Hp, Wp) == (H, W) and not frame.is_uint8(input):
            return input, (H, W)
        return frame.pad(self._enc_handle(), input, Hp, Wp, self.device_index), (H, W)

    # ---- encoder ---------------------------------------------------
    def encoder_manifest(self):
        return self._enc.manifest()

    def load_encoder_state_dict(self, state_dict):
        """`enc.*` and `hyper_enc.*` entries of the reference compressor's state_dict."""
        names = [n for n, _ in self.encoder_manifest()]
        missing = [n for n in names if n not in state_dict]
        unexpected = [k for k in state_dict if (k.startswith("enc.") or k.startswith("hyper_enc.")) and k not in names]
        if missing or unexpected:
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}.enc: missing "
                               f"{missing[:3]}, unexpected {unexpected[:3]}")
        for n in names:
            self._enc.load(n, _as_host_f32(state_dict[n]))
        self._enc.finalize()
        self._enc_finalized = True
        return self

    def analysis(self, images, cond=None):
        """The unquantised (latent, hyper_latent) of Compressor.encode (compress_modules.py:43-51); cond: VBR rate."""
        L, h = _lib.lib(), self._enc_handle()
        if not self._enc_finalized:
            raise _lib.CdcError("load_encoder_state_dict() has not been called")
        ax = _Arg(images, self.device_index)
        B, C, H, W = ax.shape
        self._set_rate(h, cond, B)
        n, nh = len(self.dim_mults), len(self.hyper_dims_mults)
        lat, pl, _ = _result_like(images, (B, self.dim * self.dim_mults[-1], H >> n, W >> n), self.device_index)
        hyp, ph, _ = _result_like(images, (B, self.dim * self.hyper_dims_mults[-1], H >> (n + nh - 1), W >> (n + nh - 1)),
                                  self.device_index)
        _lib.check(h, L.cdc_encoder_encode(h, ax.ptr, pl, ph, B, H, W, ax.mem, _current_stream(ax.mem)))
        return lat, hyp

    def _medians_like(self, t):
        shape = tuple(_Arg(t, self.device_index).shape)
        med = self._medians if self._medians is not None else np.zeros((1, shape[1], 1, 1), np.float32)
        med = np.broadcast_to(med, shape).copy()
        if type(t).__module__.startswith("torch"):
            import torch
            med = torch.from_numpy(med).to(t.device)
        return med

    def encode(self, input, cond=None, padded_hw=None, rdo=None, price_map=None, price_cells=None, segment=None, hyper_groups=None):
        """Compressor.encode (compress_modules.py:43-66): (q_latent, q_hyper_latent, state4bpp); cond: VBR rate.  Images of any
        size (float32 / uint8): the results are those of the padded frame.  rdo: the price of a bit mu >= 0, a scalar or B values
        (no reference counterpart): q_latent comes from `rdo_quantize` -- every symbol the nearest integer or, where mu * (bits saved)
        exceeds the squared error it costs, its neighbour towards the mean; state4bpp keeps the unquantised latent and gains
        "q_latent" and "rdo_moved" (int64 [B]).  None runs the reference's rounding.  price_map / price_cells (with rdo): the price of
        a bit becomes mu * the map's value at the symbol's position -- a pixel-domain map at the image's own size ([H, W], [1, H, W],
        [B, H, W] or [B, 1, H, W]; float32 >= 0 or bool), or its cells on the latent grid as `price_cells()` returns them.
        segment / hyper_groups: those of `compress_to_bytes`, checked as there; the symbols do not depend on how a stream is cut."""
        B, _, H0, W0 = frame.image_shape(input)
        segment_positions(segment, self.rate_map_cell)
        hyper_group_channels(hyper_groups, self.reversed_hyper_dims[0], segment)
        self._rates(cond, B)
        mu = None if rdo is None else rdo_values(rdo, B)
        priced = price_args(price_map, price_cells, B, (H0, W0), rdo is not None)
        input, _ = self._framed(input, padded_hw)
        cells = self._cells_of(priced, (H0, W0), tuple(frame.image_shape(input)[2:]))
        latent, hyper_latent = self.analysis(input, cond)
        q_hyper_latent = self.dequantize(hyper_latent, self._medians_like(hyper_latent))
        mean, scale = self.hyper_decode(q_hyper_latent, cond=cond)
        state4bpp = {"latent": latent, "hyper_latent": hyper_latent,
                     "latent_distribution": NormalDistribution(mean, scale)}
        if mu is None:
            q_latent = self.dequantize(latent, mean)
        else:
            q_latent, moved = self.rdo_quantize(latent, mean, scale, mu, price_cells=cells)
            state4bpp.update(q_latent=q_latent, rdo_moved=moved)
        return q_latent, q_hyper_latent, state4bpp

    def rdo_quantize(self, latent, mean, scale, rdo, price_map=None, price_cells=None):
        """cdc_op_rdo_quantize: the decision of include/cdc_hip.h on caller-supplied operands of one shape [B, ...] -> (q_latent,
        moved int64 [B] numpy).  rdo: 1 or B values.  Non-finite operands are refused (CdcError) with nothing written.
        With a price map (cdc_op_rdo_quantize_map) the operands are [B, C, ...] and a position is what follows the channel axis:
        price_cells [n, ...] holds one value per position, n = 1 or B (a NumPy array, or a tensor in the operands' memory);
        price_map is the same in pixels, for operands [B, C, h, w], at the size (h, w) * `rate_map_cell`."""
        shape = tuple(int(d) for d in latent.shape)
        if price_map is not None and price_cells is not None:
            raise ValueError("price_map and price_cells exclude each other: the map in pixels, or its cells on the latent grid")
        pixels = None
        if price_map is not None:
            if len(shape) != 4:
                raise ValueError(f"price_map needs operands [B, C, h, w], got {shape}: give price_cells, one value per position")
            size = tuple(d * self.rate_map_cell for d in shape[2:])
            pixels = price_map_values(price_map, shape[0], *size)
        args = [_Arg(t, self.device_index) for t in (latent, mean, scale)]
        if len({a.mem for a in args}) != 1 or len({tuple(a.shape) for a in args}) != 1:
            raise _lib.CdcError("latent, mean and scale must have the same shape and live in the same memory")
        B = args[0].shape[0]
        per = int(np.prod(args[0].shape[1:]))
        mu = rdo_values(rdo, B)
        mu = np.ascontiguousarray(np.broadcast_to(mu, (B,)), dtype=np.float32)
        C = shape[1] if len(shape) > 1 else 1
        gmap = None
        if pixels is not None:
            price_cells = self.price_cells(pixels, size, size)
        if price_cells is not None:
            gmap = self._op_map(price_cells, B, per // C, args[0].mem)
        L, h = _lib.lib(), self._hyper_handle()
        if not self._hyper_finalized:
            raise _lib.CdcError("load_hyper_state_dict() has not been called")
        out, po, mem = _result_like(latent, args[0].shape, self.device_index)
        if mem == _lib.CDC_MEM_DEVICE:
            import torch
            mv = torch.zeros(B, dtype=torch.int64, device=out.device)
            pm = mv.data_ptr()
        else:
            mv = np.zeros(B, np.int64)
            pm = mv.ctypes.data
        if gmap is None:
            _lib.check(h, L.cdc_op_rdo_quantize(h, args[0].ptr, args[1].ptr, args[2].ptr, mu.ctypes.data, po, pm, B, per, mem,
                                                _current_stream(mem)))
        else:
            _lib.check(h, L.cdc_op_rdo_quantize_map(h, args[0].ptr, args[1].ptr, args[2].ptr, mu.ctypes.data, gmap.ptr, gmap.shape[0], po, pm,
                                                    B, C, per // C, mem, _current_stream(mem)))
        return out, (mv.cpu().numpy() if mem == _lib.CDC_MEM_DEVICE else mv)

    def _op_map(self, price_cells, B, P, mem):
        """The map operand of cdc_op_rdo_quantize_map: [n, ...] with P values a row, n = 1 or B, float32 or bool, in the memory `mem`
        of the other operands (moved there when it lives elsewhere).  A host map is checked here (ValueError); a device map by the
        library's check kernel (CdcError, nothing written)."""
        t = price_cells
        n = int(t.shape[0]) if len(t.shape) > 1 else 1
        if n not in (1, B) or int(np.prod(tuple(t.shape))) != n * P:
            raise ValueError(f"price_cells of shape {tuple(t.shape)}: [n, ...] with n = 1 or {B} and {P} positions a row expected")
        on_device = _is_torch(t) and t.is_cuda
        if not on_device:
            t = price_cells_values(np.asarray(t.detach().numpy() if _is_torch(t) else t).reshape(n, 1, P), B).reshape(n, P)
            if mem == _lib.CDC_MEM_DEVICE:
                import torch
                t = torch.from_numpy(t).to(f"cuda:{self.device_index}")
        else:
            import torch
            if t.dtype not in (torch.float32, torch.bool):
                raise ValueError(f"price_cells must be float32 or bool, got {t.dtype}")
            t = t.to(torch.float32).reshape(n, P)
            if mem != _lib.CDC_MEM_DEVICE:
                t = t.cpu().numpy()
        a = _Arg(t, self.device_index)
        a.shape = (n, P)
        return a

    # ---- entropy coder (no reference counterpart) ---------------------
    def _median_vector(self):
        C = self.reversed_hyper_dims[0]
        med = self._medians.reshape(-1) if self._medians is not None else np.zeros(C, np.float32)
        return np.ascontiguousarray(med, dtype=np.float32)

    def compress_to_bytes(self, images, bitrate_scale=None, rdo=None, target_bpp=None, max_bytes=None, return_info=False,
                          price_map=None, price_cells=None, segment=None, hyper_groups=None):
        """images [B, 3, H, W] -> list of B bitstreams (bytes): analysis transform + hyper encoder on the GPU, then the
        range-ANS coder of include/cdc_hip.h (cdc_entropy_encode) over exactly the symbols `bpp()` prices.  A VBR model
        takes bitrate_scale (1 or B values) and records each image's rate in its stream.
        Rate control (one of three; the streams keep their format and the decoder never learns mu; downward only):
          rdo=mu         the price of a bit, a scalar or B values: rate-distortion optimised quantisation of the latent (cdc_set_rdo);
                         0 gives the bytes of rdo=None.
          target_bpp=t   a scalar or B values: per image the smallest mu whose ESTIMATED bpp (`rate()` over H * W) is <= t, found by
                         one sweep of the ladder 0, 2^-8 ... 2^8 and one refining sweep of 17 steps below the entry found
                         (`rate_sweep`: no analysis transform is repeated), then one encode.  An image that meets t already gets
                         mu = 0; one that the largest mu does not bring down to t is coded with it and reported met=False.
          max_bytes=n    the same against 8 n bits, the stream's header counted; the coder's own overhead (its 2 x 64 lane states,
                         escapes) is not in the estimate, so a stream that ends over n shrinks its image's bit target by the
                         observed ratio and is chosen again: at most 3 re-encodes.  met: len(stream) <= n.
        Region of interest (with one of the three; cdc_set_rdo_map): price_map -- [H, W], [1, H, W], [B, H, W] or [B, 1, H, W] at the
        image's own size, float32 >= 0 or bool -- or price_cells, its cells on the latent grid as `price_cells()` returns them.  The
        price of a bit becomes mu * the map at the symbol's position: 0 protects a region, 1 leaves mu as it is, larger values make
        a region pay.  Under target_bpp / max_bytes every sweep prices the ladder under the image's own map, and the "mu" reported
        is the base price the map multiplies.
        segment=s (image pixels, a multiple of `rate_map_cell`, like tile=): segmented streams (container versions 11 - 14,
        cdc_entropy_set_segments): the latent section is cut into independent sections, one per s x s window of the image, behind an
        index -- n segments code and decode on n waves, and `decompress_from_bytes(window=)` decodes only those it needs.  The symbols
        are the same; a stream grows by 8 + 12 n bytes and its segments' lane states (max_bytes counts them).  None: today's streams.
        hyper_groups=G (with segment=; container versions 19 - 22, cdc_entropy_set_hyper_groups): the hyper section as well is cut into
        independent sections, one per group of cg = ceil(Ch / G) consecutive hyper channels -- the stream holds ceil(Ch / cg) groups,
        which can be fewer than G -- coded and decoded on as many waves.  Every decode reads the form from the stream.  A stream grows
        by 8 + 12 per group and the groups' lane states, about 235 bytes a group (max_bytes counts the index).  None: one hyper section.
        return_info=True: -> (streams, {"mu", "estimated_bpp", "moved", "latent_mse", "met" (each [B]), "reencodes"})."""
        B, _, H0, W0 = frame.image_shape(images)
        rdo_exclusive(rdo, target_bpp, max_bytes)
        segment_positions(segment, self.rate_map_cell)
        hyper_group_channels(hyper_groups, self.reversed_hyper_dims[0], segment)
        self._rates(bitrate_scale, B)
        mu = None if rdo is None else rdo_values(rdo, B)
        target = None if target_bpp is None else self._targets(target_bpp, B, "target_bpp")
        budget = None if max_bytes is None else self._targets(max_bytes, B, "max_bytes")
        priced = price_args(price_map, price_cells, B, (H0, W0), not (rdo is None and target_bpp is None and max_bytes is None))
        images, hw = self._framed(images)
        cells = self._cells_of(priced, hw)
        latent, hyper = self.analysis(images, bitrate_scale)
        if target is None and budget is None:
            streams = self.latents_to_bytes(latent, hyper, bitrate_scale, image_hw=hw, rdo=mu, price_cells=cells, segment=segment,
                                            hyper_groups=hyper_groups)
            if not return_info:
                return streams
            row = self._sweep(latent, hyper, np.zeros(1, np.float32) if mu is None else mu, bitrate_scale, per_image=True, cells=cells)
            return streams, self._rdo_info(row, np.zeros(B, np.float32) if mu is None else np.broadcast_to(mu, (B,)), hw, latent,
                                           np.ones(B, bool), 0)
        ladder = np.concatenate([np.zeros(1, np.float32), RDO_LADDER])
        table = self._sweep(latent, hyper, ladder, bitrate_scale, cells=cells)
        npix = float(hw[0] * hw[1])
        if target is not None:
            goal, cost0 = target, table["bits"] / npix                  # estimated bpp against the target
        else:
            header = self._stream_header_bytes(images, hw, segment, hyper_groups)
            goal, cost0 = 8.0 * (budget - header), table["bits"]       # estimated payload bits against the budget's
        div = npix if target is not None else 1.0
        rows = [self._choose_mu(latent, hyper, bitrate_scale, b, ladder, cost0[b], goal[b], div, cells)
                for b in range(B)]
        reencodes = 0
        while True:
            mus = np.asarray([r["mu"] for r in rows], np.float32)
            streams = self.latents_to_bytes(latent, hyper, bitrate_scale, image_hw=hw, rdo=mus, price_cells=cells, segment=segment,
                                            hyper_groups=hyper_groups)
            over = [] if budget is None else [b for b in range(B) if len(streams[b]) > budget[b]]
            if not over or reencodes == 3:
                break
            reencodes += 1
            for b in over:                                              # the estimate missed the coder's overhead: aim lower by what was seen
                goal[b] *= budget[b] / len(streams[b])
                rows[b] = self._choose_mu(latent, hyper, bitrate_scale, b, ladder, cost0[b], goal[b], div, cells)
        if not return_info:
            return streams
        met = np.asarray([r["met"] for r in rows], bool) if budget is None else \
            np.asarray([len(streams[b]) <= budget[b] for b in range(B)], bool)
        row = {k: np.stack([r[k] for r in rows]) for k in ("bits", "sse", "moved")}
        return streams, self._rdo_info(row, mus, hw, latent, met, reencodes)

    @staticmethod
    def _targets(v, B, what):
        """target_bpp / max_bytes -> float64 [B], checked before the library is touched."""
        t = np.asarray(_as_host_f32(v) if type(v).__module__.startswith("torch") else v, np.float64).reshape(-1)
        if t.size not in (1, B):
            raise ValueError(f"{what} has {t.size} values for a batch of {B} (1 or {B} expected)")
        if not np.all(np.isfinite(t)) or np.any(t <= 0):
            raise ValueError(f"{what}={t.tolist()}: finite values > 0 expected")
        return np.broadcast_to(t, (B,)).copy()

    def _stream_header_bytes(self, images, hw, segment=None, hyper_groups=None):
        """Bytes of a stream that code no symbol (include/cdc_hip.h: the header's 34, + 4 with a bitrate_scale, + 8 with a recorded image
        size; of a segmented stream also the 8 bytes and the 12 of every index entry in front of its segments, and of a grouped hyper
        part the same in front of its groups)."""
        framed = tuple(frame.image_shape(images)[2:])
        seg = segment_positions(segment, self.rate_map_cell)
        index = 0
        if seg:
            c = self.rate_map_cell
            index = 8 + 12 * (-(-(framed[0] // c) // seg)) * (-(-(framed[1] // c) // seg))
        Ch = self.reversed_hyper_dims[0]
        cg = hyper_group_channels(hyper_groups, Ch, segment)
        if cg:
            index += 8 + 12 * (-(-Ch // cg))
        return 34 + (4 if self.vbr else 0) + (8 if tuple(hw) != framed else 0) + index

    def _sweep(self, latent, hyper, mus, bitrate_scale=None, per_image=False, cells=None):
        """cdc_entropy_rate_sweep on the unquantised outputs of `analysis()` -> {"bits", "sse" float64 [B, L], "moved" int64 [B, L]}.
        per_image: `mus` holds 1 or B values, one per image, and the result is [B] (image b at its own mu; the batch = batch-1
        contract makes the batch-1 calls this takes the rows of one batched call).  cells: a price map on the latent grid, float32 host
        [1 or B, gh, gw] (cdc_set_rdo_map for this call alone): every mu is priced under image b's own row."""
        L, h = _lib.lib(), self._hyper_handle()
        if not (self._hyper_finalized and self._prior_loaded):
            raise _lib.CdcError("the prior.* tensors have not been loaded (load_state_dict with the full state_dict)")
        al, ah = _Arg(latent, self.device_index), _Arg(hyper, self.device_index)
        B, _, hh, wh = ah.shape
        if per_image:
            mus = np.broadcast_to(rdo_values(mus, B), (B,))
            if len(set(mus.tolist())) == 1:
                one = self._sweep(latent, hyper, mus[:1], bitrate_scale, cells=cells)
                return {k: v[:, 0] for k, v in one.items()}
            rates = self._rates(bitrate_scale, B)
            rows = [self._sweep(latent[b:b + 1], hyper[b:b + 1], mus[b:b + 1],
                                None if rates is None else rates[b if rates.size > 1 else 0], cells=_cells_row(cells, b)) for b in range(B)]
            return {k: np.concatenate([r[k][:, 0] for r in rows]) for k in rows[0]}
        mus = rdo_values(mus, None, "mus")
        self._set_rate(h, bitrate_scale, B)
        n = int(mus.size)
        bits, sse, moved = np.empty((B, n), np.float64), np.empty((B, n), np.float64), np.empty((B, n), np.int64)
        med = self._median_vector()
        self._with_map(h, cells, lambda: _lib.check(h, L.cdc_entropy_rate_sweep(
            h, al.ptr, ah.ptr, med.ctypes.data, B, hh, wh, mus.ctypes.data, n, bits.ctypes.data, sse.ctypes.data, moved.ctypes.data, al.mem,
            _current_stream(al.mem))))
        return {"bits": bits, "sse": sse, "moved": moved}

    def _choose_mu(self, latent, hyper, bitrate_scale, b, ladder, cost, goal, div, cells=None):
        """Image b's mu for the cost goal `goal`: `cost` is its row of the first sweep over `ladder` (ascending, entry 0 = mu 0) in the
        goal's unit (bits / div) -> {"mu", "met", "bits", "sse", "moved"} at the mu chosen.  The refining sweep runs on the image's
        own rows -- its own row of the price map `cells` included: batch 1, the same values as in the batch."""
        rates = self._rates(bitrate_scale, _Arg(hyper, self.device_index).shape[0])
        rate_b = None if rates is None else rates[b if rates.size > 1 else 0]
        j, met = rdo_select(cost, goal)
        if j == 0 or not met:           # the plain symbols do, or nothing on the ladder does: no interval to refine
            sub = ladder[j:j + 1]
            k = 0
            row = self._sweep(latent[b:b + 1], hyper[b:b + 1], sub, rate_b, cells=_cells_row(cells, b))
        else:
            sub = rdo_refine_ladder(ladder[j - 1], ladder[j])
            row = self._sweep(latent[b:b + 1], hyper[b:b + 1], sub, rate_b, cells=_cells_row(cells, b))
            k, _ = rdo_select(row["bits"][0] / div, goal)               # (the interval's upper end meets the goal: it did above)
        return {"mu": np.float32(sub[k]), "met": met, "bits": row["bits"][0, k], "sse": row["sse"][0, k], "moved": row["moved"][0, k]}

    @staticmethod
    def _rdo_info(row, mus, hw, latent, met, reencodes):
        per = float(np.prod(tuple(latent.shape)[1:]))
        return {"mu": np.asarray(mus, np.float32).copy(), "estimated_bpp": np.asarray(row["bits"], np.float64) / float(hw[0] * hw[1]),
                "moved": np.asarray(row["moved"], np.int64), "latent_mse": np.asarray(row["sse"], np.float64) / per,
                "met": np.asarray(met, bool), "reencodes": int(reencodes)}

    def rate_sweep(self, images, mus, bitrate_scale=None, image_hw=None, price_map=None, price_cells=None):
        """The rate-distortion curve of the quantiser itself, for plots: images [B, 3, H, W], or the unquantised (latent, hyper) of
        `analysis()`, and a ladder `mus` of 1 .. 32 values -> {"mu" float32 [L], "bpp" [B, L] (the estimate `rate()` gives for the
        symbols chosen at mu, over H * W -- of a (latent, hyper) pair: over image_hw, default the coded extent), "latent_mse" [B, L]
        (mean squared error of the dequantised latent against the unquantised one), "moved" int64 [B, L]}.  One pass over the latent
        for the whole ladder (cdc_entropy_rate_sweep); mean and scale are the coder's own.  What the moves do to decoded images of
        trained weights is not measured by this.  price_map / price_cells: the curve under a price map (as `compress_to_bytes`; the
        pixel-domain map at the image's size, image_hw for a (latent, hyper) pair)."""
        mus = rdo_values(mus, None, "mus")
        if isinstance(images, (tuple, list)):
            latent, hyper = images
            hh, wh = tuple(hyper.shape)[2:]
            framed = (hh * self.frame_multiple, wh * self.frame_multiple)
            hw = tuple(image_hw) if image_hw is not None else framed
            cells = self._cells_of(price_args(price_map, price_cells, int(hyper.shape[0]), hw, True), hw, framed)
        else:
            B, _, H0, W0 = frame.image_shape(images)
            self._rates(bitrate_scale, B)
            priced = price_args(price_map, price_cells, B, (H0, W0), True)
            images, hw = self._framed(images)
            cells = self._cells_of(priced, hw)
            latent, hyper = self.analysis(images, bitrate_scale)
        t = self._sweep(latent, hyper, mus, bitrate_scale, cells=cells)
        per = float(np.prod(tuple(latent.shape)[1:]))
        return {"mu": mus.copy(), "bpp": t["bits"] / float(hw[0] * hw[1]), "latent_mse": t["sse"] / per, "moved": t["moved"]}

    def latents_to_bytes(self, latent, hyper, bitrate_scale=None, image_hw=None, rdo=None, price_map=None, price_cells=None, segment=None,
                         hyper_groups=None):
        """The UNquantised outputs of `analysis()` -> list of B bitstreams.  The coder's determinism contract starts here: the
        same (latent, hyper) rows give the same bytes whatever the batch they are coded in (the analysis transform itself is
        an ordinary batched forward: its last bits may depend on the batch size, like any other entry point's).
        image_hw=(H, W): the size of the original image when the latents are those of its padded frame; the streams then record it
        (container version 5 / 6) unless it equals the frame's, and are today's version 3 / 4 otherwise.
        rdo: mu, 1 or B values (cdc_set_rdo for this call alone); image b's stream depends on its own mu only.
        price_map / price_cells (with rdo; cdc_set_rdo_map for this call alone): as `compress_to_bytes`, the pixel-domain map at
        image_hw (default: the coded extent); image b's stream depends on its own mu and its own row of the map only.
        segment / hyper_groups: as `compress_to_bytes` (cdc_entropy_set_segments / cdc_entropy_set_hyper_groups for this call alone)."""
        seg = segment_positions(segment, self.rate_map_cell)
        cg = hyper_group_channels(hyper_groups, self.reversed_hyper_dims[0], segment)
        L, h = _lib.lib(), self._hyper_handle()
        al, ah = _Arg(latent, self.device_index), _Arg(hyper, self.device_index)
        B, _, hh, wh = ah.shape
        mu = None if rdo is None else rdo_values(rdo, B)
        framed = (hh * self.frame_multiple, wh * self.frame_multiple)
        hw = framed if image_hw is None else (int(image_hw[0]), int(image_hw[1]))
        cells = self._cells_of(price_args(price_map, price_cells, B, hw, rdo is not None), hw, framed)
        if not (self._hyper_finalized and self._prior_loaded):
            raise _lib.CdcError("the prior.* tensors have not been loaded (load_state_dict with the full state_dict)")
        self._set_rate(h, bitrate_scale, B)
        if seg:
            _lib.check(h, L.cdc_entropy_set_segments(h, seg))
        try:
            if cg:
                _lib.check(h, L.cdc_entropy_set_hyper_groups(h, cg))
            if mu is not None:
                _lib.check(h, L.cdc_set_rdo(h, mu.ctypes.data, int(mu.size)))
                try:
                    return self._with_map(h, cells, lambda: self._coded(L, h, al, ah, B, hh, wh, image_hw, seg, cg))
                finally:
                    L.cdc_set_rdo(h, None, 0)
            return self._coded(L, h, al, ah, B, hh, wh, image_hw, seg, cg)
        finally:
            if cg:
                L.cdc_entropy_set_hyper_groups(h, 0)
            if seg:
                L.cdc_entropy_set_segments(h, 0)

    def _coded(self, L, h, al, ah, B, hh, wh, image_hw, seg=0, cg=0):
        nsym = int(np.prod(al.shape[1:])) + int(np.prod(ah.shape[1:]))
        cap = B * (64 + 2 * 320 + 6 * nsym)              # <= 2 renormalisation bytes + a 4-byte escape payload per symbol
        if seg:                                          # the index and every segment's own 64 lane states
            cap += B * (8 + (12 + 256) * (-(-int(al.shape[2]) // seg)) * (-(-int(al.shape[3]) // seg)))
        if cg:                                           # likewise the hyper part's groups
            cap += B * (8 + (12 + 256) * (-(-int(ah.shape[1]) // cg)))
        buf = np.empty(cap, dtype=np.uint8)
        offs = (ctypes.c_size_t * (B + 1))()
        med = self._median_vector()
        if image_hw is None:
            _lib.check(h, L.cdc_entropy_encode(h, al.ptr, ah.ptr, med.ctypes.data, B, hh, wh, buf.ctypes.data, cap, offs, al.mem,
                                               _current_stream(al.mem)))
        else:
            _lib.check(h, L.cdc_entropy_encode_image(h, al.ptr, ah.ptr, med.ctypes.data, B, hh, wh, int(image_hw[0]), int(image_hw[1]),
                                                     buf.ctypes.data, cap, offs, al.mem, _current_stream(al.mem)))
        raw = buf[: offs[B]].tobytes()
        return [raw[offs[b]: offs[b + 1]] for b in range(B)]

    def decompress_from_bytes(self, streams, like=None, return_hyper=False, max_image_hw=None, return_bitrate_scale=False,
                              return_image_size=False, return_rate_map=False, window=None, return_segments=False, partial=False,
                              return_status=False):
        """list of B bitstreams -> q_latent [B, C, h, w] exactly as the encoder dequantised it (numpy, or a tensor on
        `like`'s device); all streams must have the same latent size.  max_image_hw=(H, W): refuse streams whose header
        describes a larger image before anything is allocated (untrusted input; default: the library's 2^22-position bound).
        return_bitrate_scale: also return the float32 [B] rates the streams of a VBR model carry (None for a fixed-rate model);
        `decode(q_latent, rates)` then gives the context pyramid.  return_image_size: also return (H, W), the size the streams
        record (version 5 / 6) or, for version 3 / 4, the coded extent; q_latent is that of the padded frame either way.
        return_rate_map: also return, last, `rate_map(...)["cell"]` of the decoded symbols, [B, U h, U w]: where the streams' bits
        went, without the original (the decoder holds the symbols, and runs hyper_decode once more for their mean and scale).
        window=(y0, x0, h, w) in LATENT positions (cdc_entropy_decode_window): of segmented streams only the segments that intersect
        it are decoded and verified; q_latent is full-size, equal to the full decode inside them and to hyper_decode's mean elsewhere.
        The header's checksum over all symbols is then not checked, and a corrupt segment outside the window is not noticed.
        Unsegmented streams decode whole.  return_segments: also return (segments per image, segments decoded per image).
        partial=True (cdc_entropy_decode_partial): every stream may be a prefix of a segmented stream (at least `stream_info(s)["floor"]`
        bytes; each cut where it is) and may hold damaged segments.  The segments that are wholly there and pass their checks decode as
        always; q_latent is hyper_decode's mean at every other position, and nothing is refused for them.  Sizes, rates and segments
        come from `stream_info`.  return_status: also return, last, uint8 [B, ny, nx]: 0 decoded, 1 absent (not wholly there, or outside
        window=), 2 damaged.  With partial the second number of return_segments counts the decoded (status 0) segments of IMAGE 0 only;
        the status array is the full answer.  Excludes return_rate_map; unsegmented streams are refused (segment= at the encoder is
        what makes a stream partial-decodable)."""
        if return_status and not partial:
            raise ValueError("return_status belongs to partial=True")
        if partial and return_rate_map:
            raise ValueError("partial=True excludes return_rate_map: the concealed symbols have no price")
        if window is not None:
            window = tuple(int(v) for v in window)
            if len(window) != 4 or window[0] < 0 or window[1] < 0 or window[2] < 1 or window[3] < 1:
                raise ValueError(f"window={window}: (y0, x0, h, w) in latent positions with y0, x0 >= 0 and h, w >= 1 expected")
        L, h = _lib.lib(), self._hyper_handle()
        # the limit is handle state in the library: set it on EVERY call (None -> the library's default bound), so that one
        # restricted call does not restrict the next; the product is clamped before it is handed over as a C int
        limit = 1 << 22
        if max_image_hw is not None:
            down = 2 ** (len(self.reversed_dims) - 1 + len(self.reversed_hyper_dims) - 2) if hasattr(self, "reversed_dims") else 64
            limit = min(limit, max(1, -(-int(max_image_hw[0]) // down)) * max(1, -(-int(max_image_hw[1]) // down)))
        _lib.check(h, L.cdc_entropy_set_limit(h, int(limit)))
        if not (self._hyper_finalized and self._prior_loaded):
            raise _lib.CdcError("the prior.* tensors have not been loaded (load_state_dict with the full state_dict)")
        streams = [bytes(s) for s in streams]
        B = len(streams)
        hh, wh, ar = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        dims = set()
        infos = [self.stream_info(s) for s in streams] if partial else None
        for b, s in enumerate(streams):
            if partial:
                dims.add((infos[b]["hh"], infos[b]["wh"]))
                continue
            if L.cdc_entropy_peek(s, len(s), ctypes.byref(hh), ctypes.byref(wh), ctypes.byref(ar)) != 0:
                raise _lib.CdcError("not a CDC bitstream")
            dims.add((hh.value, wh.value))
        if len(dims) != 1:
            raise _lib.CdcError("the streams of one call must share the latent size")
        hh, wh = dims.pop()
        up = 2 ** (len(self.reversed_hyper_dims) - 2)
        C = self.reversed_hyper_dims[-1] // 2
        proto = like if like is not None else np.empty(0, np.float32)
        q, pq, mem = _result_like(proto, (B, C, hh * up, wh * up), self.device_index)
        qh, ph, _ = _result_like(proto, (B, self.reversed_hyper_dims[0], hh, wh), self.device_index)
        blob = b"".join(streams)
        offs = (ctypes.c_size_t * (B + 1))()
        pos = 0
        for b, s in enumerate(streams):
            offs[b] = pos
            pos += len(s)
        offs[B] = pos
        med = self._median_vector()
        if partial:
            grids = {(i["seg"], i["ny"], i["nx"]) for i in infos}
            if len(grids) != 1:
                raise _lib.CdcError("the streams of one call must share the segment size")
            _, ny, nx = grids.pop()
            status = np.full((B, ny, nx), _lib.SEG_ABSENT, np.uint8)
            _lib.check(h, L.cdc_entropy_decode_partial(h, blob, offs, med.ctypes.data, B, None if window is None else (ctypes.c_int32 * 4)(*window),
                                                       pq, ph, status.ctypes.data, mem, _current_stream(mem)))
            out = (q, qh) if return_hyper else (q,)
            if return_bitrate_scale:
                if self.vbr and not all(i["has_rate"] for i in infos):
                    raise _lib.CdcError("a fixed-rate (version 3) stream carries no bitrate_scale")
                out = out + (np.float32([i["rate"] for i in infos]) if self.vbr else None,)
            if return_image_size:
                sizes = {(i["img_h"], i["img_w"]) if i["has_size"] else (i["hh"] * self.frame_multiple, i["wh"] * self.frame_multiple) for i in infos}
                if len(sizes) != 1:
                    raise _lib.CdcError("the streams of one call must share the image size")
                out = out + (sizes.pop(),)
            if return_segments:
                out = out + ((ny * nx, int((status[0] == _lib.SEG_OK).sum())),)
            if return_status:
                out = out + (status,)
            return out if len(out) > 1 else out[0]
        if window is None:
            _lib.check(h, L.cdc_entropy_decode(h, blob, offs, med.ctypes.data, B, pq, ph, mem, _current_stream(mem)))
        else:
            n_dec = ctypes.c_int(0)
            _lib.check(h, L.cdc_entropy_decode_window(h, blob, offs, med.ctypes.data, B, (ctypes.c_int32 * 4)(*window), pq, ph,
                                                      ctypes.byref(n_dec), mem, _current_stream(mem)))
        out = (q, qh) if return_hyper else (q,)
        if return_bitrate_scale:
            out = out + (self.bitrate_scale_of(streams) if self.vbr else None,)
        if return_image_size:
            sizes = set(self.image_size_of(streams, self.frame_multiple))
            if len(sizes) != 1:
                raise _lib.CdcError("the streams of one call must share the image size")
            out = out + (sizes.pop(),)
        if return_rate_map:
            mean, scale = self.hyper_decode(qh, cond=self.bitrate_scale_of(streams) if self.vbr else None)
            out = out + (self.rate_map(qh, q, mean, scale, ("cell",))["cell"],)
        if return_segments:
            _, ny, nx = self.segments_of(streams[:1])[0]
            out = out + ((ny * nx, ny * nx if window is None else int(n_dec.value)),)
        return out if len(out) > 1 else out[0]

    @staticmethod
    def segments_of(streams):
        """[(segment side in latent positions, ny, nx)] of the streams (cdc_entropy_peek_segments, no handle needed): (0, 1, 1) for an
        unsegmented stream (version 3 - 6), the segment size and the grid of segments of a segmented one (version 11 - 14)."""
        L = _lib.lib()
        seg, ny, nx = (ctypes.c_int() for _ in range(3))
        out = []
        for s in streams:
            s = bytes(s)
            if L.cdc_entropy_peek_segments(s, len(s), ctypes.byref(seg), ctypes.byref(ny), ctypes.byref(nx)) != 0:
                raise _lib.CdcError("not a CDC bitstream")
            out.append((seg.value, ny.value, nx.value))
        return out

    @staticmethod
    def stream_info(stream):
        """cdc_entropy_peek_partial (no handle needed) of a segmented stream or a prefix of one, as a dict: hh, wh, arith, has_rate, rate,
        has_size, img_h, img_w, seg, ny, nx, cg, ng; "declared", the length of the whole stream as its header states it; "floor", the
        bytes up to the end of the segment index (less than that decodes nothing and is refused); "complete", the leading segments, in
        raster order, that lie wholly inside the bytes given.  The `*_of` helpers refuse prefixes; this one refuses unsegmented streams."""
        s = bytes(stream)
        info = _lib.StreamInfo()
        if _lib.lib().cdc_entropy_peek_partial(s, len(s), ctypes.byref(info)) != 0:
            if len(s) >= 4 and s[:3] == b"CDC" and s[3] in (3, 4, 5, 6):
                raise _lib.CdcError(f"an unsegmented stream (version {s[3]}) is one section with nothing independent in it: segment= at the "
                                    "encoder is what makes a stream partial-decodable")
            raise _lib.CdcError("not a segmented CDC bitstream, or a prefix that ends before its segment index does (or is longer than the "
                                "stream its header declares)")
        out = {k: getattr(info, k) for k, _ in _lib.StreamInfo._fields_}
        for k in ("has_rate", "has_size"):
            out[k] = bool(out[k])
        return out

    @staticmethod
    def segment_ends(stream):
        """The byte lengths at which segments 0 .. n - 1 of a segmented stream (or of a prefix of at least `floor` bytes) complete, in
        raster order: a prefix of segment_ends(s)[k] bytes holds segments 0 .. k whole.  The last one is the declared length."""
        s = bytes(stream)
        info = _ContextDecoder.stream_info(s)
        n, floor = info["ny"] * info["nx"], info["floor"]
        sizes = np.frombuffer(s[floor - 12 * n: floor], dtype="<u4").reshape(n, 3)[:, 0].astype(np.int64)
        return [int(v) for v in floor + np.cumsum(sizes)]

    def segment_mask(self, status, seg, image_hw, as_uint8=False, like=None):
        """cdc_segment_mask: the status array [B, ny, nx] of `decompress_from_bytes(partial=True, return_status=True)` as a per-pixel mask
        [B, 1, H, W] of the H x W image: 1.0 (255 with as_uint8) where the pixel's latent position lies in a decoded segment, else 0.
        seg: the streams' segment side in latent positions (`stream_info(s)["seg"]`); like: a tensor whose device the mask goes to."""
        status = np.ascontiguousarray(status, np.uint8)
        if status.ndim != 3:
            raise ValueError(f"status must be [B, ny, nx], got {status.shape}")
        B, ny, nx = status.shape
        H, W = int(image_hw[0]), int(image_hw[1])
        proto = like if like is not None else np.empty(0, np.float32)
        out, ptr = frame._empty_like(proto, (B, 1, H, W), bool(as_uint8))
        mem = _lib.CDC_MEM_DEVICE if _is_torch(out) and out.is_cuda else _lib.CDC_MEM_HOST
        h = self._hyper_handle()
        _lib.check(h, _lib.lib().cdc_segment_mask(h, status.ctypes.data, B, ny, nx, int(seg), int(self.rate_map_cell), H, W, ptr,
                                                  _lib.CDC_ELEM_U8 if as_uint8 else _lib.CDC_ELEM_F32, mem, _current_stream(mem)))
        return out

    @staticmethod
    def hyper_groups_of(streams):
        """[(hyper channels per group, groups)] of the streams (cdc_entropy_peek_hyper_groups, no handle needed): (0, 1) for a stream
        with one hyper section (version 3 - 6, 11 - 14), cg and ng of a grouped one (version 19 - 22)."""
        L = _lib.lib()
        cg, ng = ctypes.c_int(), ctypes.c_int()
        out = []
        for s in streams:
            s = bytes(s)
            if L.cdc_entropy_peek_hyper_groups(s, len(s), ctypes.byref(cg), ctypes.byref(ng)) != 0:
                raise _lib.CdcError("not a CDC bitstream")
            out.append((cg.value, ng.value))
        return out

    @staticmethod
    def image_size_of(streams, frame_multiple=64):
        """[(H, W)] of the images the streams hold: the recorded size (version 5 / 6) or the coded extent (version 3 / 4:
        frame_multiple pixels per hyper-latent position)."""
        L = _lib.lib()
        has, H, W, hh, wh = (ctypes.c_int() for _ in range(5))
        out = []
        for s in streams:
            s = bytes(s)
            if L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(has), ctypes.byref(H), ctypes.byref(W)) != 0 or \
                    L.cdc_entropy_peek(s, len(s), ctypes.byref(hh), ctypes.byref(wh), None) != 0:
                raise _lib.CdcError("not a CDC bitstream")
            out.append((H.value, W.value) if has.value else (hh.value * frame_multiple, wh.value * frame_multiple))
        return out

    @staticmethod
    def bitrate_scale_of(streams):
        """float32 [B]: the bitrate_scale each (version-4, variable-bitrate) stream carries; a fixed-rate stream has none."""
        L = _lib.lib()
        has, r = ctypes.c_int(), ctypes.c_float()
        out = np.empty(len(streams), np.float32)
        for b, s in enumerate(streams):
            s = bytes(s)
            if L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(has), ctypes.byref(r)) != 0:
                raise _lib.CdcError("not a CDC bitstream")
            if not has.value:
                raise _lib.CdcError(f"stream {b} is a fixed-rate (version 3) stream: it carries no bitrate_scale")
            out[b] = r.value
        return out

    def forward(self, input, cond=None, padded_hw=None, return_rate_map=False, rdo=None, price_map=None, price_cells=None):
        """Compressor.forward (compress_modules.py:92-103).  Images of any size (float32 / uint8): "output" (the context pyramid the
        U-Net consumes), "q_latent" and "q_hyper_latent" are those of the PADDED frame, "bpp" counts bits over the original H * W.
        return_rate_map: also "rate_map", `rate_map(...)["cell"]` of the padded frame, [B, Hp / c, Wp / c] in bits with
        c = `rate_map_cell`; its sum over an image is bpp * H * W.  rdo: as `encode`; "bpp", "output" and "rate_map" are those of
        the symbols it chose.  price_map / price_cells: as `encode`."""
        shape = frame.image_shape(input)
        q_latent, q_hyper_latent, state4bpp = self.encode(input, cond, padded_hw, rdo, price_map, price_cells)
        out = {"output": self.decode(q_latent, cond), "bpp": self.bpp(shape, state4bpp), "q_latent": q_latent,
               "q_hyper_latent": q_hyper_latent}
        if return_rate_map:
            dist = state4bpp["latent_distribution"]
            out["rate_map"] = self.rate_map(q_hyper_latent, q_latent, dist.mean, dist.scale, ("cell",))["cell"]
        return out

    __call__ = forward


class ResnetCompressor(_ContextDecoder):
    """xparam/modules/compress_modules.py:110-177 (decoder half)."""
    _up_index = 1

    def __init__(self, dim=64, dim_mults=(1, 2, 3, 4), reverse_dim_mults=(4, 3, 2, 1),
                 hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3, device=0):
        if dim * dim_mults[-1] != dim * reverse_dim_mults[0]:
            raise AssertionError("dims[-1] == reversed_dims[0]")       # compress_modules.py:23
        super().__init__(dim, dim_mults, reverse_dim_mults, hyper_dims_mults, channels, out_channels, device)


class BigCompressor(_ContextDecoder):
    """epsilonparam/modules/compress_modules.py:112-185; vbr=True adds the VBRCondition sites (variable bitrate)."""
    _up_index = 2

    def __init__(self, dim=64, dim_mults=(1, 3, 3, 3), hyper_dims_mults=(3, 3, 3), channels=3,
                 out_channels=3, vbr=False, device=0):
        super().__init__(dim, dim_mults, tuple(reversed(dim_mults)), hyper_dims_mults, channels, out_channels, device, vbr=vbr)


class SimpleCompressor(_ContextDecoder):
    """epsilonparam/modules/compress_modules.py:187-257, the GDN context model: Conv2d(5, 2, 2) + GDN1 per `enc` level,
    ConvTranspose2d(5, 2, 2, 1) + inverse GDN1 per `dec` level (no GDN on the last level of either), hyperprior and entropy coder as
    `BigCompressor(vbr=False)`.  For the same arguments it gives a context pyramid of the same shapes, so it pairs with the same U-Net.
    vbr=True is not available: the reference raises on its first forward."""
    _ctxdec_create = "cdc_simple_ctxdec_create"
    _encoder_create = "cdc_simple_encoder_create"

    def __init__(self, dim=64, dim_mults=(1, 2, 3, 3), hyper_dims_mults=(3, 3, 3), channels=3,
                 out_channels=3, vbr=False, device=0):
        if vbr:
            # compress_modules.py:213: the last `enc` level holds an nn.Identity where Compressor.encode (:46-47) calls vbrscaler(input, cond)
            raise NotImplementedError("SimpleCompressor(vbr=True) does not run in the reference: its first forward raises "
                                      "\"TypeError: Identity.forward() takes 2 positional arguments but 3 were given\"")
        super().__init__(dim, dim_mults, tuple(reversed(dim_mults)), hyper_dims_mults, channels, out_channels, device, vbr=False)
