"""Shared pieces of the two inference scripts (counterparts of the reference's test_xparam.py / test_epsilonparam.py):
image IO without torchvision, checkpoint unwrapping, the options both scripts share (--device_seed), the per-image loop."""
import os
import pathlib
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _shared_options():
    """Options both scripts share, taken off the command line here, before the scripts' own parsers (which mirror the reference's
    argument lists) see it:
      --device_seed N   init is made on the device from N and --gamma by the library's counter-based generator (the k-th image of the
                        folder takes seed N + k): the same picture on every host.  Without it init = torch.randn * gamma, as before.
      --metrics         print PSNR and MS-SSIM of the saved image against the input beside bpp (computed on the device from the
                        reconstruction that is already there: cdc_compression_amd.metrics).  Without it the output is unchanged.
      --sampler S       "ddim" (default, the reference's update) or "dpmpp_2m", the second-order multistep solver (eta = 0 only).
      --spacing G       "index" (default, the reference's linspace over train indices) or "logsnr", the grid uniform in logSNR on
                        which the second-order solver pays off.  Without the two the output is unchanged.
      --samples K       the encoder's closed loop (compress_best_of): K seeded decodes per image, seeds
                        parallel.sample_seeds(N + k, 1, K) with N = --device_seed (0 without it), each scored against the input on the
                        device; the best one is saved, and its scores, sample index and seed are printed -- decompress(..., seed=)
                        with that seed reproduces the saved picture.
      --select METRIC   the score of --samples: "psnr" (default), "ms_ssim" or "lpips".  Without the two the output is unchanged.
      --trajectory N    progressive previews: the prediction x0 of every N-th executed step (and of the last), recorded inside the
                        device loop as uint8 (compress(..., trajectory=N, trajectory_dtype="uint8")) and saved beside the image as
                        name.stepNNNN.png, NNNN the sample index.  Not with --samples.  Without it the output is unchanged.
      --maps_dir DIR    where the bits went and where the error remains: evaluate(..., maps=True) instead of compress(), and per image
                        DIR/name.rate_map.npy (float32 [gh, gw], bits per cell of the padded frame) and DIR/name.sse_map.npy (float64,
                        squared error of the saved image per cell; np.kron(map, np.ones((c, c))) / c ** 2 with the printed cell size c
                        lays either over the picture).  Not with --samples or --trajectory.  Without it the output is unchanged."""
    import argparse
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--device_seed", type=int, default=None)
    p.add_argument("--metrics", action="store_true")
    p.add_argument("--sampler", choices=("ddim", "dpmpp_2m"), default=None)
    p.add_argument("--spacing", choices=("index", "logsnr"), default=None)
    p.add_argument("--samples", type=int, default=None)
    p.add_argument("--select", choices=("psnr", "ms_ssim", "lpips"), default=None)
    p.add_argument("--trajectory", type=int, default=None)
    p.add_argument("--maps_dir", type=str, default=None)
    opts, sys.argv[1:] = p.parse_known_args(sys.argv[1:])
    if opts.select is not None and opts.samples is None:
        p.error("--select METRIC scores the candidates of --samples K")
    if opts.trajectory is not None and (opts.trajectory < 1 or opts.samples is not None):
        p.error("--trajectory N needs N >= 1 and excludes --samples")
    if opts.maps_dir is not None and (opts.samples is not None or opts.trajectory is not None):
        p.error("--maps_dir DIR excludes --samples and --trajectory")
    return opts


SHARED = _shared_options()


def read_image(path, device):
    """torchvision.io.read_image(path).unsqueeze(0)  ->  uint8 [1, 3, H, W] on `device`, any H and W (the library converts it,
    `/ 255 * 2 - 1` as the reference's script, and pads it on the device)."""
    import torch
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.transpose(2, 0, 1).copy()).unsqueeze(0).to(device)


def save_image(u8, path):
    """One uint8 [1, 3, H, W] image (what torchvision.utils.save_image writes: the library's uint8 form does its rounding)."""
    from PIL import Image
    Image.fromarray(u8[0].detach().cpu().numpy().transpose(1, 2, 0)).save(path)


def ema_model_state(ema_state):
    """State of `ema.ema_model` from an ema_pytorch.EMA state_dict (test_xparam.py:62-68 loads the EMA wrapper and
    then uses its `ema_model`): keys "ema_model.<name>"; "online_model.*", "initted", "step" are the wrapper's."""
    out = {k[len("ema_model."):]: v for k, v in ema_state.items() if k.startswith("ema_model.")}
    if not out:
        raise KeyError('no "ema_model.*" entries: is this an ema_pytorch.EMA state_dict?')
    return out


def load_checkpoint(path):
    import torch
    return torch.load(path, map_location="cpu", weights_only=False)


def synthetic_state(diffusion, seed_unet=0, seed_ctx=15, eps=False, lpips=None):
    """Deterministic stand-in parameters (there is no network for the published checkpoints): the generator the
    parity fixtures use (cdc_compression_amd.synth).  lpips: with the "loss_fn_vgg.*" entries of a checkpoint trained with an
    LPIPS weight (stand-in LPIPS-VGG weights); None: when the model was built with one, as the reference's is (--lpips_weight
    other than 0 goes to the diffusion's aux_loss_weight)."""
    from cdc_compression_amd import synth
    if lpips is None:
        lpips = getattr(diffusion, "aux_loss_weight", 0) != 0
    sd = synth.lpips_vgg_state_dict(seed=seed_unet, prefix="loss_fn_vgg.", with_duplicates=True) if lpips else {}
    for k, v in synth.unet_state_dict(diffusion.denoise_fn.manifest(), seed=seed_unet,
                                      final_gain=0.2 if eps else 1.0).items():
        sd["denoise_fn." + k] = v
    comp = diffusion.context_fn
    man = comp.manifest() + comp.hyper_manifest() + comp.encoder_manifest()
    # FlexiblePrior entries in the reference's shapes (network_components.py:316-336; dims 1-3-3-3-1): with them the state is the one
    # the parity fixtures were made with (tests/golden: synth.unet_state_dict over the reference compressor's state_dict names)
    C0 = comp.reversed_hyper_dims[0]
    pd = (1, 3, 3, 3, 1)
    for i in range(4):
        man += [(f"prior.affine.{i}.weight", (C0, 1, 1, pd[i], pd[i + 1])), (f"prior.affine.{i}.bias", (C0, 1, 1, 1, pd[i + 1]))]
        if i < 3:
            man.append((f"prior.a.{i}", (C0, 1, 1, 1, pd[i + 1])))
    csd = synth.unet_state_dict(man, seed=seed_ctx)
    csd["prior._medians"] = np.zeros((1, C0, 1, 1), np.float32)
    for k, v in csd.items():
        sd["context_fn." + k] = v
    return sd


def run_folder(diffusion, config, rank, compress_kwargs):
    """The per-image loop of both reference scripts (test_xparam.py:72-84 / test_epsilonparam.py:67-80), for images of any size:
    the uint8 image goes straight to compress(), which pads it on the device and returns the H x W reconstruction; the saved
    image is that reconstruction in the library's uint8 form (clamp(-1, 1) / 2 + 0.5, then save_image's rounding)."""
    import torch
    from cdc_compression_amd import frame, synth
    if getattr(config, "seed", None) is not None:
        torch.manual_seed(config.seed)
    device_seed, k = SHARED.device_seed, 0
    if SHARED.sampler is not None:
        compress_kwargs = dict(compress_kwargs, sampler=SHARED.sampler)
    if SHARED.spacing is not None:
        compress_kwargs = dict(compress_kwargs, spacing=SHARED.spacing)
    for img in sorted(os.listdir(config.img_dir)):
        if img.endswith(".png") or img.endswith(".jpg"):
            to_be_compressed = read_image(os.path.join(config.img_dir, img), rank)
            shape = tuple(to_be_compressed.shape)
            best = None
            if SHARED.samples is not None:
                # --samples K: K candidate seeds per image, the best by --select is kept (bpp is the context model's, as compress()'s)
                kw = {n: compress_kwargs[n] for n in ("sampler", "spacing", "bitrate_scale", "eta") if n in compress_kwargs}
                best = diffusion.compress_best_of(to_be_compressed, SHARED.samples, metric=SHARED.select or "psnr",
                                                  seed=((device_seed or 0) + k) % 2 ** 64, gamma=config.gamma,
                                                  sample_steps=config.n_denoise_step, **kw)
                k += 1
                compressed = best["reconstruction"]
                bpp = best["bpp"].mean() if compress_kwargs.get("bpp_return_mean", True) else best["bpp"]
            elif device_seed is not None:
                # --device_seed N: init = gamma * randn made on the device from seed N + k for the k-th image of the folder (the
                # library's counter-based generator: the same picture on every host; no torch generator is involved)
                init = None
                compress_kwargs = dict(compress_kwargs, seed=(device_seed + k) % 2 ** 64, gamma=config.gamma)
                k += 1
            elif os.environ.get("CDC_SYNTHETIC_INIT"):        # seed of a device-independent start noise (the parity fixtures' generator)
                init = torch.from_numpy(synth.normal("init", shape, seed=int(os.environ["CDC_SYNTHETIC_INIT"]),
                                                     std=config.gamma)).to(to_be_compressed.device)
            else:
                init = torch.randn(shape, device=to_be_compressed.device) * config.gamma
            traj, maps = None, None
            if best is None and SHARED.maps_dir is not None:
                maps = diffusion.evaluate(to_be_compressed, sample_steps=config.n_denoise_step, init=init, maps=True, **compress_kwargs)
                compressed = maps["reconstruction"]
                bpp = maps["bpp"].mean() if compress_kwargs.get("bpp_return_mean", True) else maps["bpp"]
            elif best is None and SHARED.trajectory is not None:
                compressed, bpp, traj = diffusion.compress(to_be_compressed, sample_steps=config.n_denoise_step, init=init,
                                                           trajectory=SHARED.trajectory, trajectory_dtype="uint8", **compress_kwargs)
            elif best is None:
                compressed, bpp = diffusion.compress(
                    to_be_compressed,
                    sample_steps=config.n_denoise_step,
                    init=init,
                    **compress_kwargs,
                )
            un = diffusion.denoise_fn
            lp = None
            if diffusion.loss_fn_vgg is not None and min(shape[2:]) >= 16:   # the checkpoint carried the LPIPS-VGG weights
                lp = diffusion.loss_fn_vgg(compressed, to_be_compressed, as_saved=True)
            if SHARED.metrics:                                # the float reconstruction as it is saved, against the uint8 input
                from cdc_compression_amd import metrics
                ps, ms = metrics.distortion(un, compressed, to_be_compressed, as_saved=True)
            compressed = frame.crop(un._handle(), compressed, shape[2], shape[3], un.device_index, as_uint8=True)
            pathlib.Path(config.out_dir).mkdir(parents=True, exist_ok=True)
            save_image(compressed, os.path.join(config.out_dir, img))
            if traj is not None:                              # name.stepNNNN.png: the x0 the update of sample index NNNN used
                stem = os.path.splitext(img)[0]
                for slot, i in enumerate(traj.steps):
                    save_image(traj.x0[slot], os.path.join(config.out_dir, f"{stem}.step{i:04d}.png"))
            if maps is not None:
                pathlib.Path(SHARED.maps_dir).mkdir(parents=True, exist_ok=True)
                stem = os.path.splitext(img)[0]
                rate_map = maps["rate_map"]
                rate_map = rate_map.detach().cpu().numpy() if hasattr(rate_map, "detach") else np.asarray(rate_map)
                np.save(os.path.join(SHARED.maps_dir, f"{stem}.rate_map.npy"), rate_map[0])
                np.save(os.path.join(SHARED.maps_dir, f"{stem}.sse_map.npy"), maps["sse_map"][0])
            print("image:", img)
            print("bpp:", bpp)
            if maps is not None:
                print("map cell:", int(maps["map_cell"]))
            if SHARED.metrics:
                print("psnr:", float(ps[0]))
                print("ms_ssim:", "n/a (needs min(H, W) > 160)" if ms is None else float(ms[0]))
            if lp is not None:
                print("lpips:", float(lp[0]))
            if best is not None:
                print("scores:", " ".join(repr(float(v)) for v in best["scores"][0]))
                print("sample:", int(best["sample"][0]))
                print("chosen seed:", int(best["seed"][0]))
