"""Host-side mirror of the reference GaussianDiffusion sampler interface (inference half).

  x-param   : xparam/modules/denoising_diffusion.py:12-231   (pred_mode "x", cosine schedule)
  eps-param : epsilonparam/modules/denoising_diffusion.py:12-215 (pred_mode "noise", ddim only;
              the reference's "ddpm" branch is broken: posterior_mean_coef1 is never defined)

`compress()` keeps the reference signature and return value (reconstruction, bpp); the new
`decompress()` is the decode half alone (context pyramid in, reconstruction out).  The N-step
loop runs inside libcdc_hip.so (cdc_decode); eta != 0 falls back to per-step cdc_ddim_step
calls because the reference draws torch.randn_like on the host RNG every step.

Seeded stochastic decode (no reference counterpart): with `seed=` every draw -- the per-step noise of eta != 0 and, with `gamma=`,
the start image gamma * randn -- comes from the counter-based generator inside the sampler kernels (cdc_decode_seeded;
include/cdc_hip.h states the format): same context + same seed => same picture on every host, whatever the batch or the rank.
seed: an int s (image b takes (s + b) mod 2^64) or B ints in [0, 2^64).  No torch / NumPy generator is touched.

Sampler and step grid (no reference counterpart; both opt-in, the defaults are the reference's): `sampler="dpmpp_2m"` replaces the
first-order DDIM update by the second-order multistep solver in data-prediction form (DPM-Solver++ 2M; include/cdc_hip.h states the
update and its tables; eta must be 0, `seed` / `gamma` still make the start image), `spacing="logsnr"` -- or a strictly increasing
array of train indices, whose length is then sample_steps -- replaces the reference's linspace over train indices by a grid uniform in
logSNR (cdc_compression_amd.schedule).  The two are orthogonal; the solver pays off on the logSNR grid.  `diffusion.index` and
`diffusion.sample_steps` report the grid in use.

K samples per image (no reference counterpart; cdc_compression_amd.samples): `decompress(..., samples=K)` decodes K seeded samples of
every image through the batch programs -- sample k of image b has the seed `parallel.sample_seeds(seed, B, K)[b][k]`, sample 0 being the
plain seeded decode -- and returns them, their pixel-wise mean, or mean and unbiased variance (folded on the device in a fixed order:
the result does not depend on `sample_chunk`).  `compress_best_of` is the encoder's closed loop: it scores K candidate seeds against the
original on the device and returns the winner with its seed, which `decompress(..., seed=)` reproduces.

Decode trajectory (no reference counterpart beyond a commented-out buffer.append in its p_sample_loop; cdc_compression_amd.trajectory):
`trajectory=` on p_sample_loop / decompress / compress / evaluate records the prediction x0 and / or the state x_t of chosen steps
inside the device loop (cdc_set_trace) and returns a `Trajectory` beside the usual result; the trace is set for the one call and
cleared again, also on error.

Images of any size (cdc_compression_amd.frame states the rule): `compress`, `compress_to_bytes` and `decompress` pad on the device to
the model's multiple, run on the padded frame and return the top-left `[B, 3, H, W]` window, bpp over `H * W`.  `p_sample_loop`
mirrors the reference's method and keeps requiring frame sizes (`padded_size(H, W)` tells them).

Tiled decode (no reference counterpart; cdc_compression_amd.tiles states the plan, the noise and the weights): `decompress(..., tile=,
tile_overlap=, tile_chunk=, region=)` keeps the full-frame entropy and hyper decode and runs what follows the latent on overlapping
tiles as batch rows -- `context_fn.decode` and the sampler on `tile_chunk` rows per call, all tiles of an image on the image's seed with
frame-indexed draws -- and feather-blends the decoded tiles, crop and `as_uint8` fused into the blend.  `region=(y0, x0, h, w)` decodes
only the tiles that intersect it and returns (window, info).  One tile that covers the frame is the plain path.  `compress`, `evaluate`
and `compress_best_of` pass the arguments through.  `tile=None` runs the code it ran.  What tiling does to decoded images of trained
weights is not measured.
"""
import ctypes

import numpy as np

from . import _lib, frame, lpips, picard as _picard, samples as _samples, tiles as _tiles, trajectory as _trajectory
from .parallel import expand_seeds, sample_seeds
from .schedule import SAMPLERS, SampleSchedule
from .unet import _Arg, _current_stream, _is_torch, _result_like


class _GaussianDiffusionBase:
    _param = None   # "x" | "eps"

    def _init_common(self, denoise_fn, context_fn, num_timesteps, pred_mode, var_schedule):
        assert pred_mode in ["noise", "x", "v"]
        self.denoise_fn = denoise_fn
        self.context_fn = context_fn
        self.num_timesteps = int(num_timesteps)
        self.pred_mode = pred_mode
        self.var_schedule = var_schedule
        self.sample_steps = None
        self.sampler = "ddim"
        self.training = False
        self._sched = None
        self.loss_fn_vgg = None      # LpipsVGG, when load_state_dict() found the reference's LPIPS-VGG weights

    def eval(self):
        self.training = False
        self.denoise_fn.eval()
        return self

    def to(self, device):
        self.denoise_fn.to(device)
        if hasattr(self.context_fn, "to"):
            self.context_fn.to(device)
        if self.loss_fn_vgg is not None:
            self.loss_fn_vgg.to(device)
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Accepts the reference GaussianDiffusion.state_dict(): keys "denoise_fn.*" feed the HIP
        U-Net; "context_fn.*" are forwarded to context_fn if it has load_state_dict; "loss_fn_vgg.*" (the LPIPS-VGG
        network of a checkpoint trained with an LPIPS weight) become `self.loss_fn_vgg`, an LpipsVGG whose library handle
        is created on first use, and evaluate() then reports "lpips"; train_* buffers are derived constants and ignored."""
        un = {k[len("denoise_fn."):]: v for k, v in state_dict.items() if k.startswith("denoise_fn.")}
        self.denoise_fn.load_state_dict(un, strict=strict)
        cf = {k[len("context_fn."):]: v for k, v in state_dict.items() if k.startswith("context_fn.")}
        if cf and hasattr(self.context_fn, "load_state_dict"):
            self.context_fn.load_state_dict(cf, strict=strict)
        if any(k.startswith(lpips.PREFIX) for k in state_dict):
            self.loss_fn_vgg = lpips.LpipsVGG(device=getattr(self.denoise_fn, "device_index", 0))
            self.loss_fn_vgg.load_state_dict(state_dict, prefix=lpips.PREFIX, strict=strict)
        return self

    # ---- images of any size -------------------------------------------------------------------
    def padded_size(self, H, W):
        """(Hp, Wp) of the frame an H x W image runs on: rounded up to the least common multiple of what the U-Net and the
        context model need (cdc_padded_size of their handles; 64 for both published configurations)."""
        hs = [self.denoise_fn._handle()]
        if hasattr(self.context_fn, "_enc_handle"):
            hs.append(self.context_fn._enc_handle())
        return frame.padded_size(hs, H, W)

    @staticmethod
    def _seed_args(seed, gamma, init, B=None):
        """The argument rules of a seeded decode, checked before anything runs: -> the B seeds (None without a seed)."""
        if gamma is not None and seed is None:
            raise ValueError("gamma (a start image made on the device) needs a seed")
        if gamma is not None and init is not None:
            raise ValueError("gamma and init exclude each other: the start image is either made from the seed or given")
        if seed is None or B is None:
            return None
        return expand_seeds(seed, B)

    @staticmethod
    def _sampler_args(sampler, eta):
        """The argument rules of the sampler choice, checked before anything runs."""
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler {sampler!r}: one of {SAMPLERS}")
        if sampler != "ddim" and eta != 0:
            raise ValueError(f'sampler "{sampler}" is deterministic: eta must be 0 (seed / gamma still make the start image)')

    def _steps(self, sample_steps, spacing):
        """sample_steps of a call: as given, else the length of an explicit grid, else the train steps."""
        if sample_steps is not None:
            return sample_steps
        return self.num_timesteps if isinstance(spacing, str) else len(spacing)

    def randn(self, seed, shape, draw=0, scale=1.0, like=None):
        """scale * z(seed_b, draw) of shape [B, ...], made on the device by the generator of the seeded decode (cdc_randn): draw 0 is the
        start image of `gamma=`, draw i + 1 the noise of sample index i.  A NumPy array, or a torch tensor like `like`."""
        B = int(shape[0])
        seeds = np.asarray(expand_seeds(seed, B), dtype=np.uint64)
        per = int(np.prod([int(d) for d in shape[1:]]))
        h, dev = self.denoise_fn._handle(), self.denoise_fn.device_index
        out, optr, omem = _result_like(like if like is not None else np.empty(0, np.float32), tuple(int(d) for d in shape), dev)
        _lib.check(h, _lib.lib().cdc_randn(h, seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), B, per, int(draw), float(scale),
                                           optr, omem, _current_stream(omem)))
        return out

    def _rdo_of(self, images, bitrate_scale=None, rdo=None, target_bpp=None, max_bytes=None, price_map=None, price_cells=None, segment=None,
                hyper_groups=None):
        """The rate-control arguments of compress / compress_best_of / compress_to_bytes, checked before the library is touched ->
        (mu, cells): the context model's mu (float32, 1 or B values) or None, and its price map on the latent grid of the frame the
        U-Net asks for (float32 host [1 or B, gh, gw]) or None.  target_bpp / max_bytes: the context model chooses mu as its
        compress_to_bytes does (compressor.py) -- under the map, when there is one -- and forward(rdo=mu, price_cells=cells) then
        runs with both.  segment: the segment size of the streams `compress_to_bytes(segment=)` would write (image pixels): max_bytes
        counts their larger container; it changes no symbol otherwise.  hyper_groups: likewise the groups of their hyper part."""
        from . import compressor
        compressor.rdo_exclusive(rdo, target_bpp, max_bytes)
        self._segment_arg(segment, hyper_groups)
        B, _, H, W = frame.image_shape(images)
        if rdo is not None:
            mu = compressor.rdo_values(rdo, B)
        for name, v in (("target_bpp", target_bpp), ("max_bytes", max_bytes)):
            if v is not None:
                compressor._ContextDecoder._targets(v, B, name)
        rated = not (rdo is None and target_bpp is None and max_bytes is None)
        priced = compressor.price_args(price_map, price_cells, B, (H, W), rated)
        if not rated:
            return None, None
        if not hasattr(self.context_fn, "rdo_quantize"):
            raise ValueError("rdo / target_bpp / max_bytes need a context model of this package (rate-distortion optimised quantisation)")
        cells = self.context_fn._cells_of(priced, (H, W), self.padded_size(H, W))
        if rdo is not None:
            return mu, cells
        if self.padded_size(H, W) != self.context_fn.padded_size(H, W):
            raise NotImplementedError("target_bpp / max_bytes choose mu on the context model's own frame: a U-Net that needs a larger one "
                                      f"({self.padded_size(H, W)} against {self.context_fn.padded_size(H, W)}) cannot share it")
        kw = {} if segment is None else {"segment": segment}
        if hyper_groups is not None:
            kw["hyper_groups"] = hyper_groups
        _, info = self.context_fn.compress_to_bytes(images, bitrate_scale, target_bpp=target_bpp, max_bytes=max_bytes, return_info=True,
                                                    price_cells=cells, **kw)
        return info["mu"], cells

    def _segment_arg(self, segment, hyper_groups=None):
        """The argument rules of segment= and hyper_groups= (compressor.segment_positions, compressor.hyper_group_channels), checked
        before the library is touched: a stream is cut by a context model of this package, never by a callable that only returns a
        context pyramid."""
        from . import compressor
        if hyper_groups is not None:
            if not hasattr(self.context_fn, "hyper_groups_of"):
                raise ValueError("hyper_groups needs a context model of this package (its entropy coder writes the streams): a context_fn "
                                 "that only returns a context pyramid has no stream to cut")
            compressor.hyper_group_channels(hyper_groups, self.context_fn.reversed_hyper_dims[0], segment)
        if segment is None:
            return
        if not hasattr(self.context_fn, "segments_of"):
            raise ValueError("segment needs a context model of this package (its entropy coder writes the streams): a context_fn that only "
                             "returns a context pyramid has no stream to cut")
        compressor.segment_positions(segment, self.context_fn.rate_map_cell)

    def _context_of(self, images, *ctx_args, rate_map=False, rdo=None, price_cells=None):
        """The context model on the padded frame of `images` -> (context_dict with bpp over H * W, B, H, W, Hp, Wp).  rate_map: the
        dict also holds "rate_map" (this package's compressors only).  rdo, price_cells: the context model's mu and price map
        (`_rdo_of`)."""
        B, _, H, W = frame.image_shape(images)
        Hp, Wp = self.padded_size(H, W)
        h, dev = self.denoise_fn._handle(), self.denoise_fn.device_index
        if rate_map and not hasattr(self.context_fn, "rate_map"):
            raise ValueError("maps=True needs a context model with rate_map() (a compressor of this package)")
        if rdo is not None:
            kw = {} if price_cells is None else {"price_cells": price_cells}
            context_dict = self.context_fn(images, *ctx_args, padded_hw=(Hp, Wp), return_rate_map=rate_map, rdo=rdo, **kw)
        elif rate_map:
            context_dict = self.context_fn(images, *ctx_args, padded_hw=(Hp, Wp), return_rate_map=True)
        elif hasattr(self.context_fn, "_framed"):            # this package's compressor: pads itself, bpp over H * W
            context_dict = self.context_fn(images, *ctx_args, padded_hw=(Hp, Wp))        # x :216, eps :205
        elif (Hp, Wp) == (H, W) and not frame.is_uint8(images):
            context_dict = self.context_fn(images, *ctx_args)
        else:                                                # any other context_fn sees the frame; its bpp counts the frame's pixels
            context_dict = dict(self.context_fn(frame.pad(h, images, Hp, Wp, dev), *ctx_args))
            context_dict["bpp"] = context_dict["bpp"] * ((Hp * Wp) / (H * W))
        return context_dict, B, H, W, Hp, Wp

    def _compress_frame(self, images, sample_steps, init, eta, loop, *ctx_args, sampler="ddim", spacing="index", trace=None,
                        rate_map=False, rdo=None, price_cells=None):
        """compress() of both trees up to the crop: context model and sampler on the padded frame -> (frame, bpp [B], H, W, Trajectory
        or None), and the context model's rate map of the frame as a sixth entry with rate_map=True.  trace: (trajectory,
        trajectory_of, trajectory_dtype, seed) of the call; loop(shape, context, init, spec, window)."""
        self._sampler_args(sampler, eta)
        spec = None if trace is None else self._trace_spec(*trace[:3], self._steps(sample_steps, spacing), eta, trace[3])
        context_dict, B, H, W, Hp, Wp = self._context_of(images, *ctx_args, rate_map=rate_map, rdo=rdo, price_cells=price_cells)
        h, dev = self.denoise_fn._handle(), self.denoise_fn.device_index
        self.set_sample_schedule(self._steps(sample_steps, spacing), sampler=sampler, spacing=spacing)
        rec = loop((B, 3, Hp, Wp), context_dict["output"], frame.extend_init(h, init, B, H, W, Hp, Wp, dev), spec, (H, W))
        rec, traj = rec if spec is not None else (rec, None)
        res = (rec, context_dict["bpp"], H, W, traj)
        return res + (context_dict["rate_map"],) if rate_map else res

    def _window(self, rec, H, W):
        """The reconstruction compress() returns: the frame's top-left H x W window (the frame itself when it is the image)."""
        if tuple(rec.shape[2:]) != (H, W):
            rec = frame.crop(self.denoise_fn._handle(), rec, H, W, self.denoise_fn.device_index)
        return rec

    def evaluate(self, images, *args, as_saved=True, maps=False, **kwargs):
        """compress() with the other axis of the rate-distortion plot: takes compress()'s arguments, runs its path once and returns
        {"reconstruction": what compress() returns, "bpp": [B], "psnr": float64 [B], "ms_ssim": float64 [B], or None when
        min(H, W) <= 160}, and "lpips": float64 [B] when the loaded state dict carried the LPIPS-VGG weights (self.loss_fn_vgg).
        With parallel= also "parallel": the sweep dict of decompress(return_info=True).
        The distortion is measured on the device (cdc_compression_amd.metrics), on the padded frame's H x W window
        against `images` as given (float32 or uint8); as_saved: float32 operands through the uint8 image the reference's script would
        save (metrics.psnr(model, reconstruction, images, as_saved=True) gives the same figures).
        maps=True: where the bits went and where the error remains, on one grid of "map_cell" x "map_cell" pixels (the context model's
        rate_map_cell) over the padded frame: "rate_map" float32 [B, gh, gw] in bits (its sum is bpp * H * W), "sse_map" float64 and
        "sse_count" int32 of the same shape (metrics.sse_map of the reconstruction against `images` under as_saved: sum(sse) /
        sum(count) is the MSE of "psnr"; the cells of the padding beyond the window have count 0).  With price_map= / price_cells=
        also "price_cells", float32 [1 or B, gh, gw]: the map the encoder used, so the three maps lie on one grid."""
        from . import metrics
        import inspect
        bound = dict(inspect.signature(self.compress).bind(images, *args, **kwargs).arguments)
        bound.pop("bpp_return_mean", None)                    # bpp comes per image
        par = self._parallel_arg(bound.get("parallel"), bound.get("parallel_tol"), bound.pop("return_info", False))
        tile_kw = {k: bound.pop(k, None) for k in ("tile", "tile_overlap", "tile_chunk", "region")}
        if par is not None:
            self._parallel_check(*par, False, bound.get("sample_steps"), bound.get("spacing", "index"), bound.get("sampler", "ddim"),
                                 bound.get("eta", 0), bound.get("seed"), *tile_kw.values(), bound.get("trajectory"))
        if any(v is not None for v in tile_kw.values()):
            return self._evaluate_tiled(images, bound, tile_kw, as_saved, maps)
        rate_kw = {k: bound.pop(k, None) for k in ("rdo", "target_bpp", "max_bytes", "price_map", "price_cells")}
        mu, cells = self._rdo_of(images, bound.get("bitrate_scale"), **rate_kw)
        if mu is not None:
            bound.update(rdo=mu, price_cells=cells)
        if maps:
            rec, bpp, H, W, traj, rate_map = self._frame_of(**bound, rate_map=True)
        else:
            rec, bpp, H, W, traj = self._frame_of(**bound)
        ps, ms = metrics.distortion(self.denoise_fn, rec, images, size=(H, W), as_saved=as_saved)
        out = {"reconstruction": self._window(rec, H, W), "bpp": bpp, "psnr": ps, "ms_ssim": ms}
        if maps:
            cell = self.context_fn.rate_map_cell
            sse, count = metrics.sse_map(self.denoise_fn, rec, images, cell, size=(H, W), as_saved=as_saved, grid=tuple(rate_map.shape[1:]))
            out.update({"rate_map": rate_map, "sse_map": sse, "sse_count": count, "map_cell": cell})
            if cells is not None:
                out["price_cells"] = cells
        if self.loss_fn_vgg is not None:
            out["lpips"] = metrics.lpips(self.loss_fn_vgg, rec, images, size=(H, W), as_saved=as_saved)
        if traj is not None:
            out["trajectory"] = self._score_trajectory(traj, images, as_saved)
        if par is not None:
            out["parallel"] = dict(self.parallel_info)
        return out

    def _evaluate_tiled(self, images, bound, tile_kw, as_saved, maps):
        """evaluate(tile=...): compress()'s tiled path once, the figures on its H x W window (the tiles never form the padded frame)."""
        from . import metrics
        _tiles.check_args(tile_kw["tile"], tile_kw["tile_overlap"], tile_kw["tile_chunk"], tile_kw["region"], None, bound.get("trajectory"), maps)
        if tile_kw["region"] is not None:
            raise ValueError("evaluate() measures the whole image: region belongs to compress() / decompress()")
        rec, bpp = self.compress(**bound, bpp_return_mean=False, **tile_kw)
        ps, ms = metrics.distortion(self.denoise_fn, rec, images, as_saved=as_saved)
        out = {"reconstruction": rec, "bpp": bpp, "psnr": ps, "ms_ssim": ms}
        if self.loss_fn_vgg is not None:
            out["lpips"] = metrics.lpips(self.loss_fn_vgg, rec, images, as_saved=as_saved)
        return out

    def _score_trajectory(self, traj, images, as_saved):
        """evaluate()'s "trajectory": the Trajectory with per-slot figures of x0 (of x_t when x0 was not recorded) against `images`,
        through the metric calls evaluate() itself uses: {"trajectory", "steps", "of", "psnr": [S][B], "ms_ssim": [S][B] or None,
        "lpips": [S][B] when the LPIPS-VGG weights are loaded}."""
        from . import metrics
        of = "x0" if traj.x0 is not None else "x_t"
        slots = traj.x0 if traj.x0 is not None else traj.x_t
        res = {"trajectory": traj, "steps": list(traj.steps), "of": of, "psnr": [], "ms_ssim": []}
        if self.loss_fn_vgg is not None:
            res["lpips"] = []
        for k in range(len(traj)):
            ps, ms = metrics.distortion(self.denoise_fn, slots[k], images, as_saved=as_saved)
            res["psnr"].append(ps)
            res["ms_ssim"].append(ms)
            if self.loss_fn_vgg is not None:
                res["lpips"].append(metrics.lpips(self.loss_fn_vgg, slots[k], images, as_saved=as_saved))
        if all(m is None for m in res["ms_ssim"]):
            res["ms_ssim"] = None
        return res

    # ---- schedule ---------------------------------------------------------------------------
    def set_sample_schedule(self, sample_steps, device=None, sampler="ddim", spacing="index"):
        """The step grid (`spacing`: "index", "logsnr" or an array of train indices) and the tables of `sampler` ("ddim", "dpmpp_2m")
        for the next p_sample_loop; the defaults are the reference's schedule."""
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler {sampler!r}: one of {SAMPLERS}")
        # the schedule flavour (index / time rule, sigma formula) belongs to the TREE, not to pred_mode
        s = SampleSchedule(self.num_timesteps, self.var_schedule, self._param, sample_steps, spacing=spacing)
        self.sample_steps = sample_steps
        self.sampler = sampler
        self._spacing_arg = spacing
        self._sched = s
        self.index = s.index
        self.alphas_cumprod = s.alphas_cumprod
        self.alphas_cumprod_prev = s.alphas_cumprod_prev
        self.sigma = s.sigma
        L, h = _lib.lib(), self.denoise_fn._handle()
        p = lambda a: a.ctypes.data                                   # noqa: E731
        _lib.check(h, L.cdc_set_schedule(h, s.steps, p(s.time_in), p(s.sqrt_recip), p(s.sqrt_recipm1),
                                         p(s.sqrt_ac_prev), p(s.one_minus_ac_prev), p(s.sigma)))
        if self._param == "x" and self.pred_mode == "v":             # predict_start_from_v reads two more tables (x :128-139)
            _lib.check(h, L.cdc_set_schedule_v(h, s.steps, p(s.sqrt_ac), p(s.sqrt_one_minus_ac)))
        if sampler == "dpmpp_2m":
            self._set_solver_tables(*s.solver())

    def _set_solver_tables(self, a, b, c):
        """The a / b / c tables of the multistep update for the schedule in force (cdc_set_solver)."""
        h = self.denoise_fn._handle()
        a, b, c = (np.ascontiguousarray(t, dtype=np.float32) for t in (a, b, c))
        if not a.shape == b.shape == c.shape == (self._sched.steps,):
            raise ValueError(f"solver tables must hold {self._sched.steps} values each")
        _lib.check(h, _lib.lib().cdc_set_solver(h, self._sched.steps, a.ctypes.data, b.ctypes.data, c.ctypes.data))
        self.solver_tables = (a, b, c)

    def _reschedule(self, sampler, spacing):
        """p_sample_loop's keywords: None keeps what set_sample_schedule was given; a value sets the schedule again, at its steps."""
        if sampler is None and spacing is None:
            return
        if self.sample_steps is None:
            raise ValueError("p_sample_loop(sampler= / spacing=) follows set_sample_schedule, which gives the number of steps")
        self.set_sample_schedule(self.sample_steps, sampler=self.sampler if sampler is None else sampler,
                                 spacing=self._spacing_arg if spacing is None else spacing)

    # ---- sampler ----------------------------------------------------------------------------
    def _clip_flag(self, clip_denoised):
        if self._param == "x":
            return _lib.CDC_CLIP_ALL if clip_denoised else _lib.CDC_CLIP_NONE
        if clip_denoised == "half":                       # eps :142-143: x_recon[: B // 2].clamp_(-1, 1)
            return _lib.CDC_CLIP_HALF
        return _lib.CDC_CLIP_ALL if clip_denoised == "full" else _lib.CDC_CLIP_NONE

    def _pred_flag(self):
        if self._param == "x":
            return {"x": _lib.CDC_PRED_X, "noise": _lib.CDC_PRED_NOISE_XTREE, "v": _lib.CDC_PRED_V}[self.pred_mode]
        return _lib.CDC_PRED_NOISE                        # (the eps tree's ddim ignores pred_mode: eps :137-139)

    def _trace_spec(self, trajectory, trajectory_of, trajectory_dtype, steps, eta, seed, samples=None):
        """The trajectory keywords of a call, checked before anything runs -> trajectory.Spec or None (a Spec passes through)."""
        if isinstance(trajectory, _trajectory.Spec):
            return trajectory
        if trajectory is not None and steps is None:
            raise ValueError("p_sample_loop(trajectory=) follows set_sample_schedule, which gives the number of steps")
        return _trajectory.check_args(trajectory, trajectory_of, trajectory_dtype, steps, samples, eta, seed)

    def _trajectory_result(self, slots, spec, H, W):
        """The slots as read from the library -> Trajectory, every kind cropped to the H x W window as the reconstruction is."""
        h, dev = self.denoise_fn._handle(), self.denoise_fn.device_index
        kinds = {}
        for name, t in slots.items():
            if t is not None and tuple(t.shape[3:]) != (H, W):
                S, B = int(t.shape[0]), int(t.shape[1])
                t = frame.crop(h, t.reshape((S * B,) + tuple(t.shape[2:])), H, W, dev).reshape((S, B, 3, H, W))
            kinds[name] = t
        return _trajectory.Trajectory(spec.indices, np.asarray(self.index)[spec.indices], kinds["x0"], kinds["x_t"])

    @staticmethod
    def _parallel_arg(parallel, parallel_tol, return_info=False):
        """parallel= / parallel_tol= of a call -> what _loop takes: None for the sequential loop, else the pair."""
        if parallel is None or parallel is False:
            if parallel_tol is not None:
                raise ValueError("parallel_tol belongs to parallel=")
            if return_info:
                raise ValueError("return_info belongs to parallel=")
            return None
        return (parallel, parallel_tol)

    def _parallel_check(self, parallel, parallel_tol, return_info, sample_steps, spacing, sampler, eta, seed, tile, tile_overlap, tile_chunk,
                        region, trajectory):
        """compress()'s parallel keywords, checked before the context model runs -> the pair of _parallel_arg or None."""
        par = self._parallel_arg(parallel, parallel_tol, return_info)
        if par is not None:
            tiled = next((v for v in (tile, tile_overlap, tile_chunk, region) if v is not None), None)
            _picard.check_args(parallel, parallel_tol, self._steps(sample_steps, spacing), None, sampler, eta, seed, tiled, None, trajectory)
        return par

    def _with_info(self, res, return_info):
        """(result, parallel_info) when the call asked for it."""
        return (res, dict(self.parallel_info)) if return_info else res

    def _loop(self, shape, context, clip_denoised, init, eta, seed=None, gamma=None, sampler=None, trace=None, window=None, parallel=None):
        """sampler: None runs what set_sample_schedule was given.  trace: a trajectory.Spec -> (result, Trajectory) cropped to `window`
        ((H, W) inside the frame; None: the frame).  parallel: (window, tol) of picard.check_args -> the decode by Picard sweeps
        (cdc_decode_parallel); its {"sweeps", "strides", "max_residual", ...} is left in self.parallel_info."""
        B, C, H, W = shape
        sampler = self.sampler if sampler is None else sampler
        self._sampler_args(sampler, eta)
        if sampler != self.sampler:
            raise ValueError(f'the schedule in force was set for sampler "{self.sampler}": set_sample_schedule(..., sampler="{sampler}") first')
        seeds = self._seed_args(seed, gamma, init, B)
        if parallel is not None:
            parallel = _picard.check_args(parallel[0], parallel[1], self.sample_steps, B, sampler, eta, seed, trajectory=trace)
        L, un = _lib.lib(), self.denoise_fn
        h = un._handle()
        proto = init if init is not None else context[0]
        dev = un.device_index
        actx = [_Arg(c, dev) for c in context]
        mem = actx[0].mem
        if any(c.mem != mem for c in actx):
            raise _lib.CdcError("context tensors must all be host or all be on the model's device")
        ptrs = (ctypes.c_void_p * len(actx))(*[c.ptr for c in actx])
        pred = self._pred_flag()
        clip = self._clip_flag(clip_denoised)
        out, optr, omem = _result_like(proto, (B, C, H, W), dev)
        if omem != mem:
            raise _lib.CdcError("init and context must live in the same memory space")
        stream = _current_stream(mem)
        if eta == 0 or seeds is not None:
            ai = _Arg(init, dev) if init is not None else None
            if ai is not None and ai.mem != mem:
                raise _lib.CdcError("init and context must live in the same memory space")

            sd = None if seeds is None else np.asarray(seeds, dtype=np.uint64)      # (kept alive until device_loop has run)
            sptr = None if sd is None else sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            iptr = ai.ptr if ai else None
            g = 0.0 if gamma is None else float(gamma)

            def device_loop():
                if parallel is not None:
                    strides = (ctypes.c_int * self.sample_steps)()
                    pinfo = _lib.ParallelInfo()
                    _lib.check(h, L.cdc_decode_parallel(h, iptr, g, sptr, float(eta), ptrs, len(actx), optr, B, H, W, pred, clip, parallel[0],
                                                        parallel[1], strides, ctypes.byref(pinfo), mem, stream))
                    self.parallel_info = {"window": parallel[0], "tol": parallel[1], "sweeps": int(pinfo.sweeps),
                                          "strides": [int(v) for v in strides[:pinfo.sweeps]], "max_stride": int(pinfo.max_stride),
                                          "rows_evaluated": int(pinfo.rows_evaluated), "max_residual": float(pinfo.max_residual)}
                elif sampler == "dpmpp_2m":      # the multistep update in the device loop; the seeds serve the start image only
                    _lib.check(h, L.cdc_decode_solver(h, iptr, g, sptr, ptrs, len(actx), optr, B, H, W, pred, clip, mem, stream))
                elif seeds is not None:      # every draw from the generator in the sampler kernels: any eta stays in the device loop
                    _lib.check(h, L.cdc_decode_seeded(h, iptr, g, sptr, float(eta), ptrs, len(actx), optr, B, H, W, pred, clip, mem, stream))
                else:
                    _lib.check(h, L.cdc_decode(h, iptr, ptrs, len(actx), optr, B, H, W, pred, clip, mem, stream))
            if trace is None:
                device_loop()
                return out
            wh, ww = (H, W) if window is None else window
            with _trajectory.active(h, trace, wh, ww):       # the trace is set for this call only, and cleared on error too
                device_loop()
            return out, self._trajectory_result(_trajectory.read(h, trace, out, dev), trace, wh, ww)
        if trace is not None:
            raise ValueError("trajectory with eta != 0 needs a seed: without one the decode runs in the host loop, which has no x0")
        # eta != 0: the reference draws torch.randn_like(noise) per step (x :172, eps :150)
        if init is None:
            img = out
            if _is_torch(img):
                img.zero_()
            else:
                img[...] = 0
        else:
            img = init
        for i in reversed(range(self.sample_steps)):
            if _is_torch(proto):
                import torch
                noise = torch.randn_like(img)
            else:
                noise = np.random.standard_normal(img.shape).astype(np.float32)
            ax, an = _Arg(img, dev), _Arg(noise, dev)
            _lib.check(h, L.cdc_ddim_step(h, ax.ptr, i, ptrs, len(actx), an.ptr, float(eta), optr, B, H,
                                          W, pred, clip, mem, stream))
            if _is_torch(out):
                img = out.clone()
            else:
                img = out.copy()
        return img

    def decompress(self, context, shape=None, sample_steps=None, init=None, eta=0, clip_denoised=None, bitrate_scale=None,
                   as_uint8=False, seed=None, gamma=None, sampler="ddim", spacing="index", samples=None, reduce=None, sample_chunk=None,
                   trajectory=None, trajectory_of="x0", trajectory_dtype="float32", tile=None, tile_overlap=None, tile_chunk=None, region=None,
                   partial=False, parallel=None, parallel_tol=None, return_info=False):
        """Decode half of compress(): context pyramid (= context_fn(...)["output"]) -> image.  `context`
        may also be the transmitted q_latent tensor [B, C, H/16, W/16]: it then goes through
        `context_fn.decode` first (compress_modules.py:68-74; cdc_compression_amd.compressor on the GPU) -- with
        `bitrate_scale` (1 or B values) for a variable-bitrate context model -- or the entropy-coded streams, whose
        variable-bitrate form carries each image's rate itself.
        shape: [B, 3, H, W] of the images.  None: what the streams record (container version 5 / 6), else the coded extent (the
        finest context level).  A shape the context cannot belong to -- larger than the coded extent, or a whole multiple or
        more smaller -- or one that contradicts the size the streams record is an error.  The reconstruction is the frame's top-left H x W window.
        as_uint8: the uint8 image the reference's script saves (clamp(-1, 1) / 2 + 0.5, then save_image's rounding), made on the device.
        seed / gamma: the seeded stochastic decode (module docstring): with a seed, any eta runs in the device loop with generated
        noise; gamma (needs a seed, excludes init) starts from gamma * randn made on the device.  The draws are indexed on the padded frame.
        sampler / spacing: the update rule and the step grid (module docstring); an explicit grid's length is sample_steps.
        samples: K seeded samples per image (needs a seed and gamma or eta != 0, excludes init); None is the single decode.
        reduce: None returns [B, K, 3, H, W] (uint8 with as_uint8); "mean" their pixel-wise mean [B, 3, H, W] (with as_uint8: its uint8
        form); "mean_var" (K >= 2, no as_uint8) the pair (mean, unbiased variance).  The moments are folded on the padded frame and
        cropped once.  sample_chunk: samples per image per library call (default: the largest divisor of K with B * Kc <= 32).
        trajectory / trajectory_of / trajectory_dtype (cdc_compression_amd.trajectory): x0 and / or x_t of chosen steps, recorded in the
        device loop -> (reconstruction, Trajectory), the slots [S, B, 3, H, W] cropped to the window as the reconstruction is; excludes
        samples=, and eta != 0 needs a seed.
        tile / tile_overlap / tile_chunk / region (cdc_compression_amd.tiles): the tiled decode of a q_latent or of streams.  tile,
        tile_overlap: multiples of the frame multiple `padded_size(1, 1)[0]`, ints or (h, w) pairs, 0 < overlap <= tile / 2 (default: the
        multiple); tile_chunk: rows (tiles of all images) per sampler call (default: the fewest calls of at most 32 rows);
        region=(y0, x0, h, w) in image pixels: decodes the tiles that intersect it -> (that window, {"tiles", "tiles_decoded", "region"}).
        Of segmented streams (compress_to_bytes(segment=)) only the segments under those tiles are entropy-decoded, and the dict also
        holds "segments" and "segments_decoded" (per image); of streams with a grouped hyper section (hyper_groups=) also
        "hyper_groups", the groups a stream holds -- all of them are always decoded.
        Excludes samples=, trajectory= and a context pyramid; eta != 0 needs a seed.
        partial=True (streams only; excludes samples= and trajectory=): the streams may be prefixes of segmented streams and may hold
        damaged segments (context_fn.decompress_from_bytes(partial=True)) -> (reconstruction, info): the decode, launch for launch, of the
        q_latent that holds hyper_decode's mean wherever a segment is absent or damaged.  info: "segment_status" uint8 [B, ny, nx] (0
        decoded, 1 absent, 2 damaged); "present_mask" [B, 1, H, W], 1.0 (uint8 255 with as_uint8) where a pixel's latent position lies
        in a decoded segment; "present_region" (y0, x0, h, w), the bounding box in image pixels of the leading segments that are wholly
        there, over all images of the call, or None.  With tile=, region="present" decodes only the tiles that intersect that box --
        planned before the entropy decode, so a 30 % prefix costs 30 % of the sampler's time -- and returns that window, the tile
        info merged into info (a CdcError when no segment is complete); a region tuple works as always.
        parallel / parallel_tol (cdc_compression_amd.picard; cdc_decode_parallel): the decode by Picard sweeps over a window of
        `parallel` sampler steps (True: 16; a window above sample_steps is the whole schedule) evaluated as rows of one batch program --
        for the latency of a single image.  parallel_tol: the RMS change, in the image's [-1, 1] units, below which a row counts as
        converged; default 1e-3, a quarter of the half-step of as_uint8's rounding -- a starting value, not a measured optimum.  0
        reproduces the sequential chain of the B * window-row program in `sample_steps` sweeps.  sampler "ddim" only; eta != 0 needs a
        seed; excludes tile=, samples=, trajectory= and partial=.  return_info=True -> (reconstruction, {"sweeps", "strides",
        "max_residual", "max_stride", "rows_evaluated", "window", "tol"})."""
        par = self._parallel_arg(parallel, parallel_tol, return_info)
        if par is not None:
            if partial:
                raise ValueError("parallel excludes partial=")
            tiled = next((v for v in (tile, tile_overlap, tile_chunk, region) if v is not None), None)
            _picard.check_args(parallel, parallel_tol, self._steps(sample_steps, spacing), None, sampler, eta, seed, tiled, samples, trajectory)
        if partial:
            return self._decompress_partial(context, shape, sample_steps, init, eta, clip_denoised, bitrate_scale, as_uint8, seed, gamma, sampler,
                                            spacing, samples, reduce, sample_chunk, trajectory, tile, tile_overlap, tile_chunk, region)
        if isinstance(region, str):
            raise ValueError(f"region={region!r} belongs to partial=True")
        tile_hw, overlap_hw = _tiles.check_args(tile, tile_overlap, tile_chunk, region, samples, trajectory)
        if tile_hw is not None:
            if eta != 0 and seed is None:
                raise ValueError("tile with eta != 0 needs a seed: the tiles of an image draw the noise of the frame positions they cover")
            if isinstance(context, (list, tuple)) and context and not isinstance(context[0], (bytes, bytearray)):
                raise ValueError("tile needs the latent (a q_latent tensor or streams): a context pyramid of the whole frame is not cut into tiles")
            tile_hw, overlap_hw = _tiles.check_multiples(tile_hw, overlap_hw, self.padded_size(1, 1)[0])
            if region is not None and shape is not None:
                _tiles.check_region(region, int(shape[2]), int(shape[3]))
        self._seed_args(seed, gamma, init)
        self._sampler_args(sampler, eta)
        spec = self._trace_spec(trajectory, trajectory_of, trajectory_dtype, self._steps(sample_steps, spacing), eta, seed, samples)
        if samples is None and (reduce is not None or sample_chunk is not None):
            raise ValueError("reduce / sample_chunk belong to samples=K")
        K = None if samples is None else _samples.check_args(samples, seed, gamma, eta, init, reduce, as_uint8, sample_chunk)
        recorded = seg_info = hyper_groups = None
        if isinstance(context, (bytes, bytearray)):
            context = [context]
        if isinstance(context, (list, tuple)) and context and isinstance(context[0], (bytes, bytearray)):
            # entropy-coded bitstreams (compress_to_bytes): range-ANS decode -> q_latent (+ the rates of a VBR model)
            if bitrate_scale is not None:
                raise ValueError("the streams carry their own bitrate_scale")
            # a region of segmented streams: the tiles are planned from the peeked sizes first, and only the segments under the
            # selected tiles' latent windows are entropy-decoded (unsegmented streams: the call and the info dict of always)
            cut = tile_hw is not None and region is not None and hasattr(self.context_fn, "segments_of") and \
                self.context_fn.segments_of(context[:1])[0][0] > 0
            if hasattr(self.context_fn, "hyper_groups_of") and self.context_fn.hyper_groups_of(context[:1])[0][0] > 0:
                hyper_groups = self.context_fn.hyper_groups_of(context[:1])[0][1]
            if cut:
                win = self._stream_window(context[0], tile_hw, overlap_hw, region)
                context, bitrate_scale, recorded, seg_info = self.context_fn.decompress_from_bytes(
                    context, like=init, return_bitrate_scale=True, return_image_size=True, window=win, return_segments=True)
            else:
                context, bitrate_scale, recorded = self.context_fn.decompress_from_bytes(context, like=init, return_bitrate_scale=True,
                                                                                         return_image_size=True)
        if not isinstance(context, (list, tuple)):
            if self.context_fn is None or not hasattr(self.context_fn, "decode"):
                raise RuntimeError("decompress(q_latent, ...) needs a context_fn with decode()")
            if tile_hw is not None:
                res = self._decompress_tiled(context, bitrate_scale, recorded, shape, tile_hw, overlap_hw, tile_chunk, region, sample_steps, init,
                                             eta, clip_denoised, as_uint8, seed, gamma, sampler, spacing)
                if res is not None:
                    if seg_info is not None:
                        res[1].update(segments=seg_info[0], segments_decoded=seg_info[1])
                    if hyper_groups is not None and region is not None:
                        res[1].update(hyper_groups=hyper_groups)
                    return res
            context = self.context_fn.decode(context) if bitrate_scale is None else self.context_fn.decode(context, bitrate_scale)
        if K is None:
            self._seed_args(seed, gamma, init, int(context[0].shape[0]))
        else:
            all_seeds = sample_seeds(seed, int(context[0].shape[0]), K)
        self.set_sample_schedule(self._steps(sample_steps, spacing), sampler=sampler, spacing=spacing)
        if clip_denoised is None:
            clip_denoised = True if self._param == "x" else getattr(self, "clip_noise", "none")
        B, _, Hp, Wp = (int(d) for d in context[0].shape)          # the coded extent: the finest context level
        H, W = recorded if recorded is not None else ((Hp, Wp) if shape is None else (int(shape[2]), int(shape[3])))
        if shape is not None and tuple(int(d) for d in shape) != (B, 3, H, W):
            raise _lib.CdcError(f"shape {tuple(shape)} contradicts the context, which holds {B} image(s) of {H} x {W}")
        M = self.padded_size(1, 1)[0]                               # the frame of an image is less than one multiple larger than it
        if not (0 <= Hp - H < M and 0 <= Wp - W < M):
            raise _lib.CdcError(f"a {H} x {W} image does not pad to the {Hp} x {Wp} frame of the context (multiple {M})")
        h, dev = self.denoise_fn._handle(), self.denoise_fn.device_index
        if K is not None:
            return self._decompress_samples(context, all_seeds, K, (H, W), clip_denoised, eta, gamma, sampler, reduce, sample_chunk, as_uint8)
        rec = self._loop((B, 3, Hp, Wp), context, clip_denoised, frame.extend_init(h, init, B, H, W, Hp, Wp, dev), eta,
                         seed, gamma, sampler, spec, (H, W), par)
        rec, traj = rec if spec is not None else (rec, None)
        if (Hp, Wp) != (H, W) or as_uint8:
            rec = frame.crop(h, rec, H, W, dev, as_uint8=as_uint8)
        if par is not None:
            return self._with_info(rec, return_info)
        return rec if traj is None else (rec, traj)

    # ---- tiled decode (cdc_compression_amd.tiles) --------------------------------------------------------------------------
    def _stream_window(self, stream, tile, overlap, region):
        """The latent window decompress(streams, tile=, region=) needs of the streams' q_latent: the bounding box of the selected
        tiles' latent windows (y0, x0, h, w in latent positions), planned from the sizes the stream's header holds as
        `_decompress_tiled` plans them from the q_latent; None when one tile covers the frame (the plain path decodes it whole)."""
        cf = self.context_fn
        H, W = cf.image_size_of([stream], cf.frame_multiple)[0]
        hh, wh = ctypes.c_int(), ctypes.c_int()
        if _lib.lib().cdc_entropy_peek(bytes(stream), len(stream), ctypes.byref(hh), ctypes.byref(wh), None) != 0:
            raise _lib.CdcError("not a CDC bitstream")
        return self._latent_window(H, W, hh.value, wh.value, tile, overlap, region)

    def _latent_window(self, H, W, hh, wh, tile, overlap, region):
        """`_stream_window` from the sizes a peek gave: the H x W image, hh x wh hyper-latent positions."""
        cf = self.context_fn
        cell = 1 << len(cf.rev_mults)
        Hp, Wp = hh * cf.frame_multiple, wh * cf.frame_multiple
        window = _tiles.check_region(region, H, W)
        plan = _tiles.Plan(Hp, Wp, tile, overlap)
        if plan.T == 1:
            return None
        origins = plan.origins(plan.intersecting(window))
        y0, x0 = min(y for y, _ in origins) // cell, min(x for _, x in origins) // cell
        y1, x1 = (max(y for y, _ in origins) + plan.th) // cell, (max(x for _, x in origins) + plan.tw) // cell
        return (y0, x0, y1 - y0, x1 - x0)

    # ---- partial streams (include/cdc_hip.h: cdc_entropy_decode_partial) ---------------------------------------------------------
    def _decompress_partial(self, streams, shape, sample_steps, init, eta, clip_denoised, bitrate_scale, as_uint8, seed, gamma, sampler, spacing,
                            samples, reduce, sample_chunk, trajectory, tile, tile_overlap, tile_chunk, region):
        """decompress(streams, partial=True): -> (reconstruction, info).  Everything the sampler needs to plan comes from the peek of
        the prefixes, before the entropy decode."""
        if samples is not None or reduce is not None or sample_chunk is not None or trajectory is not None:
            raise ValueError("partial=True excludes samples= and trajectory=")
        if isinstance(streams, (bytes, bytearray)):
            streams = [streams]
        if not (isinstance(streams, (list, tuple)) and streams and all(isinstance(s, (bytes, bytearray)) for s in streams)):
            raise ValueError("partial=True decodes streams (bytes): a q_latent or a context pyramid is whole already")
        if bitrate_scale is not None:
            raise ValueError("the streams carry their own bitrate_scale")
        if isinstance(region, str) and region != "present":
            raise ValueError(f"region={region!r}: a (y0, x0, h, w) tuple or \"present\"")
        if region is not None and tile is None:
            raise ValueError("region belongs to tile=")
        cf = self.context_fn
        if cf is None or not hasattr(cf, "stream_info"):
            raise RuntimeError("decompress(streams, partial=True) needs a context_fn of this package")
        infos = [cf.stream_info(s) for s in streams]
        i0 = infos[0]
        sizes = {(i["img_h"], i["img_w"]) if i["has_size"] else (i["hh"] * cf.frame_multiple, i["wh"] * cf.frame_multiple) for i in infos}
        if len(sizes) != 1 or len({(i["seg"], i["ny"], i["nx"]) for i in infos}) != 1:
            raise _lib.CdcError("the streams of one call must share the image size and the segment size")
        H, W = sizes.pop()
        B = len(streams)
        if shape is not None and tuple(int(d) for d in shape) != (B, 3, H, W):
            raise _lib.CdcError(f"shape {tuple(shape)} contradicts the streams, which hold {B} image(s) of {H} x {W}")
        # the bounding box of the segments that are wholly there, in image pixels
        span, box = i0["seg"] * int(cf.rate_map_cell), None
        for i in infos:
            for s in range(i["complete"]):
                sy, sx = divmod(s, i["nx"])
                y0, x0, y1, x1 = sy * span, sx * span, min(H, (sy + 1) * span), min(W, (sx + 1) * span)
                if y0 < H and x0 < W:
                    box = (y0, x0, y1, x1) if box is None else (min(box[0], y0), min(box[1], x0), max(box[2], y1), max(box[3], x1))
        present = None if box is None else (box[0], box[1], box[2] - box[0], box[3] - box[1])
        if region == "present":
            if present is None:
                raise _lib.CdcError("region=\"present\": no segment of these streams is complete yet (nothing to decode)")
            region = present
        tile_hw, overlap_hw = _tiles.check_args(tile, tile_overlap, tile_chunk, region, None, None)
        win = None
        if tile_hw is not None and region is not None:
            tile_hw, overlap_hw = _tiles.check_multiples(tile_hw, overlap_hw, self.padded_size(1, 1)[0])
            win = self._latent_window(H, W, i0["hh"], i0["wh"], tile_hw, overlap_hw, region)
        q, rates, _, seg_info, status = cf.decompress_from_bytes(streams, like=init, return_bitrate_scale=True, return_image_size=True, window=win,
                                                                 return_segments=True, partial=True, return_status=True)
        rec = self.decompress(q, (B, 3, H, W), sample_steps, init, eta, clip_denoised, rates, as_uint8, seed, gamma, sampler, spacing,
                              tile=tile, tile_overlap=tile_overlap, tile_chunk=tile_chunk, region=region)
        info = {"segment_status": status, "present_mask": cf.segment_mask(status, i0["seg"], (H, W), as_uint8=as_uint8, like=init),
                "present_region": present}
        if isinstance(rec, tuple):
            rec, tile_info = rec
            info.update(tile_info, segments=seg_info[0], segments_decoded=seg_info[1])
        return rec, info

    def _decompress_tiled(self, q_latent, bitrate_scale, recorded, shape, tile, overlap, tile_chunk, region, sample_steps, init, eta,
                          clip_denoised, as_uint8, seed, gamma, sampler, spacing):
        """decompress(q_latent, tile=...): -> the result, or None when one tile covers the frame and no region is asked for (the caller
        goes on with the plain path: the same launches, the same bits)."""
        cf, un = self.context_fn, self.denoise_fn
        h, dev = un._handle(), un.device_index
        M = self.padded_size(1, 1)[0]
        B, _, hl, wl = (int(d) for d in q_latent.shape)
        cell = 1 << len(cf.rev_mults)                               # image pixels per latent position and side (compressor.decode)
        Hp, Wp = hl * cell, wl * cell
        if M % cell:
            raise _lib.CdcError(f"the frame multiple {M} is no multiple of the {cell} pixels of a latent position")
        H, W = recorded if recorded is not None else ((Hp, Wp) if shape is None else (int(shape[2]), int(shape[3])))
        if shape is not None and tuple(int(d) for d in shape) != (B, 3, H, W):
            raise _lib.CdcError(f"shape {tuple(shape)} contradicts the context, which holds {B} image(s) of {H} x {W}")
        if not (0 <= Hp - H < M and 0 <= Wp - W < M):
            raise _lib.CdcError(f"a {H} x {W} image does not pad to the {Hp} x {Wp} frame of the context (multiple {M})")
        window = None if region is None else _tiles.check_region(region, H, W)
        plan = _tiles.Plan(Hp, Wp, tile, overlap)
        if plan.T == 1:
            if window is None:
                return None
            rec = self.decompress(q_latent, (B, 3, H, W), sample_steps, init, eta, clip_denoised, bitrate_scale, False, seed, gamma, sampler, spacing)
            one = _tiles.Plan(H, W, (H, W), (1, 1))                 # the image as its own single tile: the blend is a copy of the window
            return _tiles.blend(h, rec, one, B, dev, window=window, as_uint8=as_uint8), {"tiles": 1, "tiles_decoded": 1, "region": window}
        seeds = self._seed_args(seed, gamma, init, B)
        self.set_sample_schedule(self._steps(sample_steps, spacing), sampler=sampler, spacing=spacing)
        if clip_denoised is None:
            clip_denoised = True if self._param == "x" else getattr(self, "clip_noise", "none")
        sel = plan.intersecting(window)
        Ts, th, tw = len(sel), plan.th, plan.tw
        origins = plan.origins(sel)
        lat = _tiles.gather(cf._handle(), q_latent, [(y // cell, x // cell) for y, x in origins], th // cell, tw // cell, cf.device_index)
        init_rows = None
        if init is not None:
            init_rows = _tiles.gather(h, frame.extend_init(h, init, B, H, W, Hp, Wp, dev), origins, th, tw, dev)
        rates = None if bitrate_scale is None else np.broadcast_to(np.asarray(bitrate_scale, np.float32).reshape(-1), (B,))
        rows = B * Ts
        chunk = _tiles.default_chunk(rows) if tile_chunk is None else min(int(tile_chunk), rows)
        decoded = None
        for r0 in range(0, rows, chunk):
            r1 = min(rows, r0 + chunk)
            bs = [r // Ts for r in range(r0, r1)]
            ctx = cf.decode(lat[r0:r1]) if rates is None else cf.decode(lat[r0:r1], np.ascontiguousarray(rates[bs]))
            frames = None if seeds is None else [(Hp, Wp) + tuple(origins[r % Ts]) for r in range(r0, r1)]
            with _tiles.noise_frames(h, frames):
                part = self._loop((r1 - r0, 3, th, tw), ctx, clip_denoised, None if init_rows is None else init_rows[r0:r1], eta,
                                  None if seeds is None else [seeds[b] for b in bs], gamma, sampler)
            if r1 - r0 == rows:
                decoded = part
            else:
                if decoded is None:
                    decoded = frame._empty_like(part, (rows, 3, th, tw), False)[0]
                decoded[r0:r1] = part
        rec = _tiles.blend(h, decoded, plan, B, dev, window=(0, 0, H, W) if window is None else window,
                           present=None if Ts == plan.T else sel, as_uint8=as_uint8)
        return rec if window is None else (rec, {"tiles": plan.T, "tiles_decoded": Ts, "region": window})

    def _compress_tiled(self, images, ctx_args, rate_kw, bpp_return_mean, tile_kw, **dec_kw):
        """compress(tile=...) of both trees: the encoder on the whole frame (no full-frame context pyramid is made), then the tiled
        decode of its q_latent -> (reconstruction, bpp), with a region (window, bpp, info)."""
        cf = self.context_fn
        if not hasattr(cf, "encode") or not hasattr(cf, "rev_mults"):
            raise ValueError("tile needs a context model of this package (its q_latent is what is cut into tiles)")
        _tiles.check_args(tile_kw["tile"], tile_kw["tile_overlap"], tile_kw["tile_chunk"], tile_kw["region"], None, dec_kw.pop("trajectory", None))
        mu, cells = self._rdo_of(images, ctx_args[0] if ctx_args else None, **rate_kw)
        B, _, H, W = frame.image_shape(images)
        kw = {} if mu is None else ({"rdo": mu} if cells is None else {"rdo": mu, "price_cells": cells})
        q_latent, _, state = cf.encode(images, *ctx_args, padded_hw=self.padded_size(H, W), **kw)
        bpp = cf.bpp((B, 3, H, W), state)
        rec = self.decompress(q_latent, (B, 3, H, W), bitrate_scale=ctx_args[0] if ctx_args else None, **dec_kw, **tile_kw)
        bpp = bpp.mean() if bpp_return_mean else bpp
        return (rec[0], bpp, rec[1]) if tile_kw["region"] is not None else (rec, bpp)

    # ---- K samples per image (cdc_compression_amd.samples) --------------------------------------------------------------
    def _sample_chunk(self, context, seeds, k0, Kc, clip_denoised, eta, gamma, sampler):
        """Samples k0 .. k0 + Kc - 1 of every image on the padded frame: [B * Kc, 3, Hp, Wp], row b * Kc + kk (cdc_decode_samples)."""
        B, _, Hp, Wp = (int(d) for d in context[0].shape)
        return _samples.decode_samples(self.denoise_fn, context, _samples.chunk_seeds(seeds, k0, Kc), B, Kc, Hp, Wp, gamma, eta,
                                       self._pred_flag(), self._clip_flag(clip_denoised), sampler == "dpmpp_2m")

    def _decompress_samples(self, context, seeds, K, size, clip_denoised, eta, gamma, sampler, reduce, sample_chunk, as_uint8):
        un = self.denoise_fn
        h, dev = un._handle(), un.device_index
        B, _, Hp, Wp = (int(d) for d in context[0].shape)
        H, W = size
        window = lambda t, u8=False: (frame.crop(h, t, H, W, dev, as_uint8=u8) if (Hp, Wp) != (H, W) or u8 else t)   # noqa: E731
        plan = _samples.chunks(B, K, sample_chunk)
        if reduce is None:
            out = None
            for k0, Kc in plan:
                part = window(self._sample_chunk(context, seeds, k0, Kc, clip_denoised, eta, gamma, sampler), as_uint8)
                part = part.reshape((B, Kc, 3, H, W))
                if Kc == K:
                    return part
                if out is None:
                    out = frame._empty_like(part, (B, K, 3, H, W), as_uint8)[0]
                out[:, k0:k0 + Kc] = part
            return out
        mean = frame._empty_like(context[0], (B, 3, Hp, Wp), False)[0]
        m2 = frame._empty_like(context[0], (B, 3, Hp, Wp), False)[0] if reduce == "mean_var" else None
        for k0, Kc in plan:
            chunk = self._sample_chunk(context, seeds, k0, Kc, clip_denoised, eta, gamma, sampler)
            _samples.fold_moments(un, chunk, B, Kc, k0, mean, m2, finish=m2 is not None and k0 + Kc == K)
        if m2 is None:
            return window(mean, as_uint8)
        return window(mean), window(m2)

    def _best_of(self, images, samples, metric, seed, gamma, eta, sample_steps, sampler, spacing, sample_chunk, as_saved, clip_denoised,
                 *ctx_args, rdo=None, price_cells=None, tile_kw=None):
        """compress_best_of of both trees.  tile_kw (tile / tile_overlap / tile_chunk): every candidate is a tiled decode of the
        encoder's q_latent, scored and kept on the H x W window, one candidate per pass."""
        from . import metrics
        K = _samples.check_args(samples, seed, gamma, eta, sample_chunk=sample_chunk, metric=metric)
        self._sampler_args(sampler, eta)
        B, _, H, W = frame.image_shape(images)
        if metric == "lpips" and self.loss_fn_vgg is None:
            raise ValueError('metric "lpips" needs the LPIPS-VGG weights (self.loss_fn_vgg: a state dict with "loss_fn_vgg." keys)')
        if metric == "ms_ssim" and min(H, W) < metrics.MS_SSIM_MIN_SIDE:
            raise ValueError(f"MS-SSIM needs min(H, W) > 160, got {H} x {W}")
        higher = _samples.METRICS[metric]
        all_seeds = sample_seeds(seed, B, K)
        if tile_kw is not None and any(v is not None for v in tile_kw.values()):
            _tiles.check_args(tile_kw["tile"], tile_kw["tile_overlap"], tile_kw["tile_chunk"])
            cf = self.context_fn
            if not hasattr(cf, "encode") or not hasattr(cf, "rev_mults"):
                raise ValueError("tile needs a context model of this package (its q_latent is what is cut into tiles)")
            kw = {} if rdo is None else ({"rdo": rdo} if price_cells is None else {"rdo": rdo, "price_cells": price_cells})
            q_latent, _, state = cf.encode(images, *ctx_args, padded_hw=self.padded_size(H, W), **kw)
            scores = np.full((B, K), np.nan, np.float64)
            best_k, best = [0] * B, None
            for k in range(K):
                rec = self.decompress(q_latent, (B, 3, H, W), sample_steps, None, eta, clip_denoised, ctx_args[0] if ctx_args else None, False,
                                      [all_seeds[b][k] for b in range(B)], gamma, sampler, spacing, **tile_kw)
                if metric == "lpips":
                    row = metrics.lpips(self.loss_fn_vgg, rec, images, as_saved=as_saved)
                else:
                    row = getattr(metrics, metric)(self.denoise_fn, rec, images, as_saved=as_saved)
                scores[:, k] = np.asarray(row, np.float64)
                if best is None:
                    best = rec
                    continue
                for b in range(B):
                    if _samples.better(float(scores[b, k]), float(scores[b, best_k[b]]), higher):
                        best_k[b] = k
                        best[b] = rec[b]
            return {"reconstruction": best, "bpp": cf.bpp((B, 3, H, W), state),
                    "seed": np.asarray([all_seeds[b][best_k[b]] for b in range(B)], dtype=np.uint64), "sample": np.asarray(best_k, dtype=np.int64),
                    "score": scores[np.arange(B), best_k], "scores": scores}
        context_dict, B, H, W, Hp, Wp = self._context_of(images, *ctx_args, rdo=rdo, price_cells=price_cells)
        context = context_dict["output"]
        self.set_sample_schedule(self._steps(sample_steps, spacing), sampler=sampler, spacing=spacing)
        un = self.denoise_fn
        scores = np.full((B, K), np.nan, np.float64)
        best_k = [0] * B
        best = frame._empty_like(context[0], (B, 3, Hp, Wp), False)[0]
        originals = None
        for k0, Kc in _samples.chunks(B, K, sample_chunk):
            chunk = self._sample_chunk(context, all_seeds, k0, Kc, clip_denoised, eta, gamma, sampler)
            if originals is None or originals.shape[0] != B * Kc:
                originals = _samples.repeat_images(un, images, Kc)
            if metric == "lpips":
                row = metrics.lpips(self.loss_fn_vgg, chunk, originals, size=(H, W), as_saved=as_saved)
            else:
                row = getattr(metrics, metric)(un, chunk, originals, size=(H, W), as_saved=as_saved)
            scores[:, k0:k0 + Kc] = np.asarray(row, np.float64).reshape(B, Kc)
            pick = []
            for b in range(B):
                for k in range(k0, k0 + Kc):
                    if _samples.better(float(scores[b, k]), float(scores[b, best_k[b]]), higher):
                        best_k[b] = k
                pick.append(best_k[b] - k0 if best_k[b] >= k0 else -1)     # (the first chunk always picks: sample 0 when nothing beats it)
            _samples.select(un, chunk, pick, best, B, Kc)
        return {"reconstruction": self._window(best, H, W), "bpp": context_dict["bpp"],
                "seed": np.asarray([all_seeds[b][best_k[b]] for b in range(B)], dtype=np.uint64), "sample": np.asarray(best_k, dtype=np.int64),
                "score": scores[np.arange(B), best_k], "scores": scores}


    def compress_to_bytes(self, images, bitrate_scale=None, rdo=None, target_bpp=None, max_bytes=None, return_info=False,
                          price_map=None, price_cells=None, segment=None, hyper_groups=None):
        """The transmitted half of compress(): images -> one entropy-coded bitstream per image.
        `decompress(streams, shape, sample_steps, init)` reconstructs from them.  bitrate_scale: the rate of a
        variable-bitrate context model (1 or B values), recorded in each stream.  Images of any size: a stream records H x W
        unless the image is its own padded frame.  rdo / target_bpp / max_bytes / return_info: the context model's rate control
        (compressor.compress_to_bytes), price_map / price_cells its region-of-interest map; the decoder side needs nothing.
        segment (image pixels, a multiple of the pixels of a latent position): segmented streams, whose segments code and decode in
        parallel and of which `decompress(streams, tile=, region=)` entropy-decodes only what the region's tiles need.
        hyper_groups (with segment; compressor.compress_to_bytes): the hyper section too in that many groups of channels at the most,
        one wave each; every decode reads the form from the stream."""
        from . import compressor
        compressor.rdo_exclusive(rdo, target_bpp, max_bytes)
        self._segment_arg(segment, hyper_groups)
        B, _, H, W = frame.image_shape(images)
        if rdo is not None:
            compressor.rdo_values(rdo, B)
        for name, v in (("target_bpp", target_bpp), ("max_bytes", max_bytes)):
            if v is not None:
                compressor._ContextDecoder._targets(v, B, name)
        priced = compressor.price_args(price_map, price_cells, B, (H, W), not (rdo is None and target_bpp is None and max_bytes is None))
        if self.padded_size(H, W) != self.context_fn.padded_size(H, W):
            raise NotImplementedError("the stream records the image size against the context model's own multiple: a U-Net that needs a "
                                      f"larger one ({self.padded_size(H, W)} against {self.context_fn.padded_size(H, W)}) cannot share it")
        kw = {k: v for k, v in (("rdo", rdo), ("target_bpp", target_bpp), ("max_bytes", max_bytes)) if v is not None}
        if return_info:
            kw["return_info"] = True
        if segment is not None:
            kw["segment"] = segment
        if hyper_groups is not None:
            kw["hyper_groups"] = hyper_groups
        if priced is not None:
            kw["price_map" if priced[0] == "map" else "price_cells"] = priced[1]
        if bitrate_scale is None:
            return self.context_fn.compress_to_bytes(images, **kw)
        return self.context_fn.compress_to_bytes(images, bitrate_scale, **kw)


class GaussianDiffusionX(_GaussianDiffusionBase):
    """xparam/modules/denoising_diffusion.py:12-231."""
    _param = "x"

    def __init__(self, denoise_fn, context_fn, ae_fn=None, num_timesteps=1000, loss_type="l1",
                 lagrangian=1e-3, pred_mode="noise", var_schedule="linear", aux_loss_weight=0,
                 aux_loss_type="l1", use_loss_weight=False, loss_weight_min=5,
                 use_aux_loss_weight_schedule=False):
        if ae_fn is not None:
            raise NotImplementedError("ae_fn (latent diffusion) is not on the tested decode path")
        self._init_common(denoise_fn, context_fn, num_timesteps, pred_mode, var_schedule)
        self.ae_fn = None
        self.loss_type = loss_type
        self.aux_loss_weight = aux_loss_weight      # (the reference builds its LPIPS-VGG network when this is > 0)
        self.lagrangian_beta = lagrangian

    def p_sample_loop(self, shape, context, clip_denoised=False, init=None, eta=0, seed=None, gamma=None, sampler=None, spacing=None,
                      trajectory=None, trajectory_of="x0", trajectory_dtype="float32", window=None, parallel=None, parallel_tol=None,
                      return_info=False):
        """trajectory / trajectory_of / trajectory_dtype (cdc_compression_amd.trajectory): -> (image, Trajectory), the slots cropped
        to `window` ((H, W) of the image inside the frame `shape`; None: the frame).
        parallel / parallel_tol (cdc_compression_amd.picard; decompress states them): the decode by Picard sweeps over a window of
        `parallel` steps; return_info=True -> (image, {"sweeps", "strides", "max_residual", ...})."""
        spec = self._trace_spec(trajectory, trajectory_of, trajectory_dtype, self.sample_steps, eta, seed)
        self._reschedule(sampler, spacing)
        return self._with_info(self._loop(tuple(shape), context, clip_denoised, init, eta, seed, gamma, sampler, spec, window,
                                          self._parallel_arg(parallel, parallel_tol, return_info)), return_info)

    def _frame_of(self, images, sample_steps=None, init=None, eta=0, seed=None, gamma=None, sampler="ddim", spacing="index",
                  trajectory=None, trajectory_of="x0", trajectory_dtype="float32", rate_map=False, rdo=None, price_cells=None,
                  parallel=None, parallel_tol=None):
        self._seed_args(seed, gamma, init, frame.image_shape(images)[0])
        return self._compress_frame(images, sample_steps, init, eta,
                                    lambda shape, ctx, i, spec, win: self.p_sample_loop(shape, ctx, clip_denoised=True, init=i, eta=eta,
                                                                                        seed=seed, gamma=gamma, trajectory=spec,
                                                                                        window=win, parallel=parallel,
                                                                                        parallel_tol=parallel_tol),   # :223
                                    sampler=sampler, spacing=spacing, trace=(trajectory, trajectory_of, trajectory_dtype, seed),
                                    rate_map=rate_map, rdo=rdo, price_cells=price_cells)

    def compress(self, images, sample_steps=None, bpp_return_mean=True, init=None, eta=0, seed=None, gamma=None, sampler="ddim",
                 spacing="index", trajectory=None, trajectory_of="x0", trajectory_dtype="float32", rdo=None, target_bpp=None,
                 max_bytes=None, price_map=None, price_cells=None, tile=None, tile_overlap=None, tile_chunk=None, region=None, segment=None,
                 hyper_groups=None, parallel=None, parallel_tol=None, return_info=False):
        """trajectory=: -> (reconstruction, bpp, Trajectory) (cdc_compression_amd.trajectory).  rdo / target_bpp / max_bytes: the
        context model's rate control (compressor.compress_to_bytes); bpp is that of the symbols it chose.  price_map / price_cells
        (with one of them): its region-of-interest map, in pixels at the image's size or on the latent grid.
        tile / tile_overlap / tile_chunk / region: the decode half runs tiled (decompress states them); with a region
        -> (window, bpp, info).  segment / hyper_groups: the segment size and the hyper groups of the streams to be written
        (compress_to_bytes): max_bytes counts them.  parallel / parallel_tol / return_info: the decode half by Picard sweeps
        (decompress states them); return_info=True appends the sweep dict to the result."""
        par = self._parallel_check(parallel, parallel_tol, return_info, sample_steps, spacing, sampler, eta, seed, tile, tile_overlap,
                                   tile_chunk, region, trajectory)
        if not (tile is None and tile_overlap is None and tile_chunk is None and region is None):
            return self._compress_tiled(images, (), dict(rdo=rdo, target_bpp=target_bpp, max_bytes=max_bytes, price_map=price_map, price_cells=price_cells,
                                                         segment=segment, hyper_groups=hyper_groups),
                                        bpp_return_mean, dict(tile=tile, tile_overlap=tile_overlap, tile_chunk=tile_chunk, region=region),
                                        sample_steps=sample_steps, init=init, eta=eta, seed=seed, gamma=gamma, sampler=sampler, spacing=spacing,
                                        trajectory=trajectory)
        mu, cells = self._rdo_of(images, None, rdo, target_bpp, max_bytes, price_map, price_cells, segment, hyper_groups)
        rec, bpp, H, W, traj = self._frame_of(images, sample_steps, init, eta, seed, gamma, sampler, spacing, trajectory, trajectory_of,
                                              trajectory_dtype, rdo=mu, price_cells=cells, parallel=parallel, parallel_tol=parallel_tol)
        res = (self._window(rec, H, W), (bpp.mean() if bpp_return_mean else bpp))
        if par is not None and return_info:
            return res + (dict(self.parallel_info),)
        return res if traj is None else res + (traj,)


    def compress_best_of(self, images, samples, metric="psnr", seed=None, gamma=None, eta=0, sample_steps=None, sampler="ddim",
                         spacing="index", sample_chunk=None, as_saved=True, rdo=None, target_bpp=None, max_bytes=None, price_map=None,
                         price_cells=None, tile=None, tile_overlap=None, tile_chunk=None, segment=None, hyper_groups=None):
        """The encoder's closed loop: the context model once, then `samples` seeded decodes per image (seeds
        parallel.sample_seeds(seed, B, samples)), each scored on the device against `images` on the frame's H x W window
        (metric "psnr" / "ms_ssim": higher is better; "lpips": lower, needs self.loss_fn_vgg; ties go to the lowest k, a NaN never
        beats a number) -> {"reconstruction": the winner's window, "bpp": [B], "seed": uint64 [B], ready for decompress(..., seed=),
        "sample": int [B], "score": [B], "scores": [B, samples]}.  rdo / target_bpp / max_bytes / price_map / price_cells: as compress().
        tile / tile_overlap / tile_chunk: every candidate is a tiled decode (decompress states them).  segment / hyper_groups: as compress()."""
        mu, cells = self._rdo_of(images, None, rdo, target_bpp, max_bytes, price_map, price_cells, segment, hyper_groups)
        return self._best_of(images, samples, metric, seed, gamma, eta, sample_steps, sampler, spacing, sample_chunk, as_saved, True, rdo=mu,
                             price_cells=cells, tile_kw=dict(tile=tile, tile_overlap=tile_overlap, tile_chunk=tile_chunk))


class GaussianDiffusionEps(_GaussianDiffusionBase):
    """epsilonparam/modules/denoising_diffusion.py:12-215."""
    _param = "eps"

    def __init__(self, denoise_fn, context_fn, channels=3, num_timesteps=1000, loss_type="l1",
                 clip_noise="half", vbr=False, lagrangian=1e-3, pred_mode="noise", var_schedule="linear",
                 aux_loss_weight=0, aux_loss_type="l1"):
        self._init_common(denoise_fn, context_fn, num_timesteps, pred_mode, var_schedule)
        if pred_mode != "noise":
            raise NotImplementedError('eps-param tree: only pred_mode="noise" reaches ddim()')
        self.channels = channels
        self.clip_noise = clip_noise
        self.aux_loss_weight = aux_loss_weight      # (the reference builds its LPIPS-VGG network when this is > 0)
        self.vbr = vbr

    def p_sample_loop(self, shape, context, sample_mode, init=None, eta=0, seed=None, gamma=None, sampler=None, spacing=None,
                      trajectory=None, trajectory_of="x0", trajectory_dtype="float32", window=None, parallel=None, parallel_tol=None,
                      return_info=False):
        """trajectory / trajectory_of / trajectory_dtype / window / parallel / parallel_tol / return_info: as
        GaussianDiffusionX.p_sample_loop."""
        spec = self._trace_spec(trajectory, trajectory_of, trajectory_dtype, self.sample_steps, eta, seed)
        if sample_mode != "ddim":
            raise NotImplementedError('sample_mode "ddpm" raises AttributeError in the reference '
                                      "(posterior_mean_coef1 undefined); only \"ddim\" is implemented")
        self._reschedule(sampler, spacing)
        return self._with_info(self._loop(tuple(shape), context, self.clip_noise, init, eta, seed, gamma, sampler, spec, window,
                                          self._parallel_arg(parallel, parallel_tol, return_info)), return_info)

    def _frame_of(self, images, sample_steps=None, bitrate_scale=None, sample_mode="ddpm", init=None, eta=0, seed=None, gamma=None,
                  sampler="ddim", spacing="index", trajectory=None, trajectory_of="x0", trajectory_dtype="float32", rate_map=False,
                  rdo=None, price_cells=None, parallel=None, parallel_tol=None):
        self._seed_args(seed, gamma, init, frame.image_shape(images)[0])
        return self._compress_frame(images, sample_steps, init, eta,
                                    lambda shape, ctx, i, spec, win: self.p_sample_loop(shape, ctx, sample_mode, init=i, eta=eta, seed=seed,
                                                                                        gamma=gamma, trajectory=spec, window=win,
                                                                                        parallel=parallel, parallel_tol=parallel_tol),
                                    bitrate_scale, sampler=sampler, spacing=spacing,
                                    trace=(trajectory, trajectory_of, trajectory_dtype, seed), rate_map=rate_map, rdo=rdo,
                                    price_cells=price_cells)

    def compress(self, images, sample_steps=None, bitrate_scale=None, sample_mode="ddpm",
                 bpp_return_mean=True, init=None, eta=0, seed=None, gamma=None, sampler="ddim", spacing="index",
                 trajectory=None, trajectory_of="x0", trajectory_dtype="float32", rdo=None, target_bpp=None, max_bytes=None,
                 price_map=None, price_cells=None, tile=None, tile_overlap=None, tile_chunk=None, region=None, segment=None,
                 hyper_groups=None, parallel=None, parallel_tol=None, return_info=False):
        """trajectory=: -> (reconstruction, bpp, Trajectory) (cdc_compression_amd.trajectory).  rdo / target_bpp / max_bytes /
        price_map / price_cells / tile / tile_overlap / tile_chunk / region / segment / hyper_groups / parallel / parallel_tol /
        return_info: as GaussianDiffusionX.compress."""
        par = self._parallel_check(parallel, parallel_tol, return_info, sample_steps, spacing, sampler, eta, seed, tile, tile_overlap,
                                   tile_chunk, region, trajectory)
        if not (tile is None and tile_overlap is None and tile_chunk is None and region is None):
            if sample_mode != "ddim":
                raise NotImplementedError('sample_mode "ddpm" raises AttributeError in the reference; only "ddim" is implemented')
            return self._compress_tiled(images, (bitrate_scale,), dict(rdo=rdo, target_bpp=target_bpp, max_bytes=max_bytes, price_map=price_map,
                                                                      price_cells=price_cells, segment=segment, hyper_groups=hyper_groups),
                                        bpp_return_mean, dict(tile=tile, tile_overlap=tile_overlap, tile_chunk=tile_chunk, region=region),
                                        sample_steps=sample_steps, init=init, eta=eta, seed=seed, gamma=gamma, sampler=sampler, spacing=spacing,
                                        trajectory=trajectory)
        mu, cells = self._rdo_of(images, bitrate_scale, rdo, target_bpp, max_bytes, price_map, price_cells, segment, hyper_groups)
        rec, bpp, H, W, traj = self._frame_of(images, sample_steps, bitrate_scale, sample_mode, init, eta, seed, gamma, sampler, spacing,
                                              trajectory, trajectory_of, trajectory_dtype, rdo=mu, price_cells=cells, parallel=parallel,
                                              parallel_tol=parallel_tol)
        res = (self._window(rec, H, W), (bpp.mean() if bpp_return_mean else bpp))
        if par is not None and return_info:
            return res + (dict(self.parallel_info),)
        return res if traj is None else res + (traj,)

    def compress_best_of(self, images, samples, metric="psnr", seed=None, gamma=None, eta=0, sample_steps=None, sampler="ddim",
                         spacing="index", sample_chunk=None, as_saved=True, bitrate_scale=None, rdo=None, target_bpp=None, max_bytes=None,
                         price_map=None, price_cells=None, tile=None, tile_overlap=None, tile_chunk=None, segment=None, hyper_groups=None):
        """GaussianDiffusionX.compress_best_of with this tree's context argument (bitrate_scale of a variable-bitrate model)."""
        mu, cells = self._rdo_of(images, bitrate_scale, rdo, target_bpp, max_bytes, price_map, price_cells, segment, hyper_groups)
        return self._best_of(images, samples, metric, seed, gamma, eta, sample_steps, sampler, spacing, sample_chunk, as_saved,
                             self.clip_noise, bitrate_scale, rdo=mu, price_cells=cells,
                             tile_kw=dict(tile=tile, tile_overlap=tile_overlap, tile_chunk=tile_chunk))
