#!/usr/bin/env python3
"""Golden vectors for images of any size, from the REAL reference.

Same rules as make_golden.py, whose helpers this imports: the reference's own modules run on the PyTorch CPU path with the
deterministic synthetic parameters of cdc_compression_amd.synth, and only data is stored.

    python tests/golden/make_golden_anysize.py          # ~6 min on 8 cores (one 65-step run at 512 x 384)

The reference cannot take these images at all (its torch.cat sites fail unless H and W are multiples of 64), so the fixture is
what the padding rule defines: the reference's compress() on the REPLICATE-PADDED image (bottom / right, to the model's multiple)
with the ZERO-EXTENDED init, its reconstruction cropped to the top-left H x W window, its bpp multiplied by Hp Wp / (H W).

Stored per case: the unpadded uint8 image, a digest of the padded float input the reference was actually given (so that the rule
can be restated in numpy without the reference), q_latent (of the padded frame), the rescaled bpp, the cropped reconstruction
(full for the small models, digest for the full one).  The init is NOT stored: synth.normal("init", [B,3,H,W], seed 1, std 0.8).

Every case is also run through the reference's compressor in float64: an image with a q_latent / q_hyper_latent symbol that differs
between float32 and float64 is refused (assert) -- a fixture the reference cannot reproduce against itself cannot pin the GPU
(one flipped symbol moves the reference's own bpp by more than the 1e-5 the tests allow).

  anysize_images.npz    the uint8 windows of the reference's imgs/1.png .. 3.png
  anysize_full_x.npz    full x-param model (ResnetCompressor dim 64 + U-Net dim 64), B = 1:
                          500x333   top-left window of imgs/1.png (odd width, both sides padded, frame 512 x 384): 4 steps and 65 steps
                                    (the reference script's default), in anysize_full_x_500x333.npz; the 65-step result also as the
                                    uint8 image the script would save, with a mask of the pixels whose float lies within the decode
                                    bound of a rounding boundary, in anysize_full_x_500x333_saved.npz
                          64x100    top-left window (one side exact), 4 steps
                          10x10     rows / cols 300.. (margin larger than the image), 4 steps
                          256x256   top-left window (nothing to pad), 4 steps
  anysize_small.npz     small models, full tensors:
                          x_10x10     small x-param model, the 10x10 window above, 4 steps
                          eps_33x48   small eps model, B = 3 (top-left windows of imgs/1..3.png), 3 steps, ddim
                          vbr_33x48   the same with the variable-bitrate context model at three distinct rates
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import digest, import_reference, synth  # noqa: E402

KEEP = ("enc.", "hyper_enc.", "hyper_dec.", "dec.", "prior.affine", "prior.a.")
SMALL_X_COMP = dict(dim=16, dim_mults=[1, 2], reverse_dim_mults=[2, 1], hyper_dims_mults=[2, 2, 2], channels=3, out_channels=8)
SMALL_EPS_COMP = dict(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3)
VBR_RATES = [0.0, 0.37, 1.0]
SEED_CTX, SEED_VBR = 15, 25
DECODE_BOUND = 3e-5           # the long-run decode bound of the tests (test_kodak_crops_500_steps_match_reference)


def window(i, y0, x0, H, W):
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(mg.REF, "imgs", f"{i}.png")).convert("RGB"))
    return np.ascontiguousarray(im[y0:y0 + H, x0:x0 + W].transpose(2, 0, 1))          # [3, H, W] uint8


def to_unit(u8):
    """The reference script's conversion (test_xparam.py:74,76)."""
    return torch.from_numpy(u8).float() / 255.0 * 2.0 - 1.0


def multiple(comp, unet_kw):
    n, nh = len(comp.enc), len(comp.hyper_enc)
    return max(2 ** (n + nh - 1), 2 ** (len(unet_kw["dim_mults"]) - 1))


def no_flip(comp, xp, cond):
    """float32 against the same module in float64: no symbol of q_latent / q_hyper_latent may differ."""
    args = () if cond is None else (cond,)
    with torch.no_grad():
        a = comp(xp, *args)
        comp.double()
        b = comp(xp.double(), *(() if cond is None else (cond.double(),)))
        comp.float()
    for k in ("q_latent", "q_hyper_latent"):
        d = (a[k].double() - b[k]).abs()
        flips = int((d > 0.5).sum())
        assert flips == 0, f"{k}: {flips} symbols differ between float32 and float64 -- choose another image"
    rel = float(((a["bpp"].double() - b["bpp"]).abs() / b["bpp"].abs()).max())
    return a, rel


def run_case(diff, comp, M, u8, steps_list, rec_store, tag, rec, full, cond=None, **ckw):
    """u8 [B, 3, H, W] -> reference compress() on the padded frame for every step count."""
    B, _, H, W = u8.shape
    Hp, Wp = -(-H // M) * M, -(-W // M) * M
    x = to_unit(u8)
    xp = F.pad(x, (0, Wp - W, 0, Hp - H), mode="replicate") if (Hp, Wp) != (H, W) else x
    init = torch.from_numpy(synth.normal("init", (B, 3, H, W), seed=1, std=0.8).copy())
    initp = F.pad(init, (0, Wp - W, 0, Hp - H), value=0.0)
    cd, rel = no_flip(comp, xp, cond)
    d = digest(xp.numpy(), nsample=256)
    rec.update({f"{tag}_hw": np.array([H, W]), f"{tag}_padded_hw": np.array([Hp, Wp]), f"{tag}_q_latent": cd["q_latent"].numpy(),
                f"{tag}_padded_idx": d["idx"], f"{tag}_padded_val": d["val"], f"{tag}_padded_sum": np.array(d["sum"]),
                f"{tag}_f64_bpp_rel": np.array(rel)})
    for steps in steps_list:
        with torch.no_grad():
            if cond is None:
                r, bpp = diff.compress(xp, sample_steps=steps, bpp_return_mean=False, init=initp.clone(), **ckw)
            else:
                r, bpp = diff.compress(xp, sample_steps=steps, bitrate_scale=cond, bpp_return_mean=False, init=initp.clone(), **ckw)
        r = r[:, :, :H, :W].contiguous()
        rec[f"{tag}_bpp"] = bpp.double().numpy() * (Hp * Wp) / (H * W)
        if full:
            rec[f"{tag}_rec{steps}"] = r.numpy()
        else:
            dr = digest(r.numpy(), nsample=256)
            rec.update({f"{tag}_rec{steps}_idx": dr["idx"], f"{tag}_rec{steps}_val": dr["val"], f"{tag}_rec{steps}_sum": np.array(dr["sum"])})
        if steps in rec_store:
            # what the reference script saves (test_xparam.py:81,83), and where the float lies within the decode bound of a rounding boundary
            y = r.clamp(-1, 1) / 2.0 + 0.5
            t = y * 255.0 + 0.5
            rec[f"{tag}_u8_{steps}"] = t.clamp(0, 255).to(torch.uint8).numpy()
            frac = (t.double() - t.double().floor()).numpy()
            # |dx| < DECODE_BOUND moves t = (x / 2 + .5) 255 + .5 by < 127.5 DECODE_BOUND, plus the float32 roundings of its three operations at <= 256
            near = np.minimum(frac, 1.0 - frac) < DECODE_BOUND * 127.5 + 3 * 2.0 ** -16
            rec[f"{tag}_near_{steps}"] = np.packbits(near.reshape(-1))
        print(tag, steps, "bpp", rec[f"{tag}_bpp"], "f32/f64 bpp rel", rel, flush=True)


def load_comp(comp, seed, vbr=False):
    man = [(k, list(v.shape)) for k, v in comp.state_dict().items() if k.startswith(KEEP)]
    sd = (synth.compressor_state_dict if vbr else synth.unet_state_dict)(man, seed=seed)
    comp.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    comp.eval()
    return man


def gen_images():
    rec = {"w500x333": window(1, 0, 0, 500, 333)[None], "w64x100": window(1, 0, 0, 64, 100)[None], "w10x10": window(1, 300, 300, 10, 10)[None],
           "w256x256": window(1, 0, 0, 256, 256)[None], "w33x48": np.stack([window(i, 0, 0, 33, 48) for i in (1, 2, 3)])}
    np.savez_compressed(os.path.join(HERE, "anysize_images.npz"), **rec)
    return rec


def gen_full_x(img):
    tree = "xparam"
    ref = import_reference(tree)
    _, kw, _, _, _, _ = mg.CONFIGS["full_x"]
    net = ref.unet.Unet(**kw)
    mg.load_synth(net, seed=0)
    comp = ref.cm.ResnetCompressor(**mg.ENCODER["encoder_full_x"][2])
    load_comp(comp, SEED_CTX)
    diff = ref.dd.GaussianDiffusion(denoise_fn=net, context_fn=comp, ae_fn=None, **mg.DIFF[tree])
    diff.eval()
    M = multiple(comp, kw)
    assert M == 64
    rec = {}
    run_case(diff, comp, M, img["w64x100"], [4], (), "64x100", rec, False)
    run_case(diff, comp, M, img["w10x10"], [4], (), "10x10", rec, False)
    run_case(diff, comp, M, img["w256x256"], [4], (), "256x256", rec, False)
    np.savez_compressed(os.path.join(HERE, "anysize_full_x.npz"), **rec)
    rec = {}
    run_case(diff, comp, M, img["w500x333"], [4, 65], (65,), "500x333", rec, False)
    saved = {k: rec.pop(k) for k in ("500x333_u8_65", "500x333_near_65")}        # (three files: each stays below 1 MiB)
    np.savez_compressed(os.path.join(HERE, "anysize_full_x_500x333.npz"), **rec)
    np.savez_compressed(os.path.join(HERE, "anysize_full_x_500x333_saved.npz"), **saved)


def gen_small(img):
    rec = {}
    meta = {}
    # small x-param model
    ref = import_reference("xparam")
    _, kw, _, _, _, _ = mg.CONFIGS["small_x"]
    net = ref.unet.Unet(**kw)
    mg.load_synth(net, seed=0)
    comp = ref.cm.ResnetCompressor(**SMALL_X_COMP)
    meta["x"] = {"unet_kwargs": kw, "unet_manifest": mg.manifest_of(net), "comp_kwargs": SMALL_X_COMP, "comp_manifest": load_comp(comp, SEED_CTX),
                 "seed": SEED_CTX}
    diff = ref.dd.GaussianDiffusion(denoise_fn=net, context_fn=comp, ae_fn=None, **mg.DIFF["xparam"])
    diff.eval()
    run_case(diff, comp, multiple(comp, kw), img["w10x10"], [4], (), "x_10x10", rec, True)
    # small eps model, fixed rate and variable bitrate
    ref = import_reference("epsilonparam")
    _, kw, _, _, _, _ = mg.CONFIGS["small_eps"]
    for tag, vbr, seed in (("eps", False, SEED_CTX), ("vbr", True, SEED_VBR)):
        net = ref.unet.Unet(**kw)
        mg.load_synth(net, seed=0, final_gain=0.2)
        comp = ref.cm.BigCompressor(vbr=vbr, **SMALL_EPS_COMP)
        meta[tag] = {"unet_kwargs": kw, "unet_manifest": mg.manifest_of(net), "comp_kwargs": dict(SMALL_EPS_COMP, vbr=vbr),
                     "comp_manifest": load_comp(comp, seed, vbr), "seed": seed, "rates": VBR_RATES if vbr else None}
        diff = ref.dd.GaussianDiffusion(denoise_fn=net, context_fn=comp, **dict(mg.DIFF["epsilonparam"], vbr=vbr))
        diff.eval()
        cond = torch.tensor(VBR_RATES, dtype=torch.float32) if vbr else None
        run_case(diff, comp, multiple(comp, kw), img["w33x48"], [3], (), f"{tag}_33x48", rec, True, cond=cond, sample_mode="ddim")
    json.dump(meta, open(os.path.join(HERE, "manifest_anysize_small.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "anysize_small.npz"), **rec)


if __name__ == "__main__":
    torch.set_num_threads(8)
    images = gen_images()
    which = sys.argv[1:] or ["small", "full_x"]
    if "small" in which:
        gen_small(images)
    if "full_x" in which:
        gen_full_x(images)
