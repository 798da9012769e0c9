#!/usr/bin/env python3
"""Golden vectors of the variable-bitrate context model (epsilonparam BigCompressor(vbr=True)) from the REAL reference.

Same rules as make_golden.py, whose helpers this imports: the reference's own modules run on the PyTorch CPU path with the
deterministic synthetic parameters of cdc_compression_amd.synth (`compressor_state_dict`: the VBRCondition scalers kept O(1)),
and only data is stored.

    python tests/golden/make_golden_vbr.py          # ~1 min

vbr_small (dim 8: full tensors) and vbr_full (dim 64, the width of the test script: digests), each at three rate cases:
  distinct  B = 3, one rate per image;
  bcast     B = 2, one rate for the batch;
  neg       B = 2, an extrapolated rate at which EVERY VBRCondition site has a negative scale in some channel (asserted), and a
            second image at an ordinary rate.
For each: decode (synthesis transform), hyper_dec, encode (latent, hyper_latent) and forward (q_latent, q_hyper_latent, bpp,
context pyramid).  vbr_e2e: GaussianDiffusion.compress(images, 3, bitrate_scale, "ddim", init) with the small eps U-Net.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import digest, import_reference, synth  # noqa: E402

KEEP = ("enc.", "hyper_enc.", "hyper_dec.", "dec.", "prior.affine", "prior.a.")
VBR = {
    # name: (ctor kwargs, full tensors?)
    "vbr_small": (dict(dim=8, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3), True),
    "vbr_full": (dict(dim=64, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3), False),
}
DISTINCT = [0.0, 0.37, 1.0]
BCAST = [0.6]
ORDINARY = 0.37
SEED_W, SEED_IMG, SEED_Q, SEED_QH = 25, 26, 27, 28
IMG_HW, LAT_HW, HYP_HW = (64, 64), (2, 2), (2, 2)


def vbr_sites(net):
    return [m for m in net.modules() if type(m).__name__ == "VBRCondition"]


def negative_rate(net):
    """The smallest rate r = k / 4 > 1 at which scale(r) = W r + b < 0 in at least one channel of every site."""
    for k in range(5, 200):
        r = k / 4.0
        if all(bool(((s.scale.weight.reshape(-1) * r + s.scale.bias) < 0).any()) for s in vbr_sites(net)):
            return r
    raise AssertionError("no rate below 50 turns a scale negative at every VBR site")


def put(rec, key, a, full):
    a = np.asarray(a, np.float32)
    if full or a.size <= 12288:
        rec[key] = a
    d = digest(a)
    rec.update({f"{key}_shape": np.array(a.shape), f"{key}_idx": d["idx"], f"{key}_val": d["val"], f"{key}_sum": d["sum"]})


def run_case(ref, net, rates, B, full, rec, tag):
    import modules.utils as ut                              # (the tree import_reference loaded last)
    cond = torch.tensor(rates, dtype=torch.float32)
    x = synth.normal("vbr_image", (3, 3) + IMG_HW, seed=SEED_IMG, std=0.5).clip(-1, 1).astype(np.float32)[:B]
    c0 = net.reversed_dims[0]
    q = np.round(synth.normal("vbr_q_latent", (3, c0) + LAT_HW, seed=SEED_Q, std=2.0)).astype(np.float32)[:B]
    ch = net.reversed_hyper_dims[0]
    qh = (np.round(synth.normal("vbr_q_hyper", (3, ch) + HYP_HW, seed=SEED_QH, std=2.0)) + 0.25).astype(np.float32)[:B]
    with torch.no_grad():
        outs = net.decode(torch.from_numpy(q), cond)
        h = torch.from_numpy(qh)
        n = len(net.hyper_dec)
        for i, (deconv, vbr, act) in enumerate(net.hyper_dec):
            h = deconv(h)
            if i != n - 1:
                h = vbr(h, cond)
            h = act(h)
        mean, scale = h.chunk(2, 1)
        scale = scale.clamp(min=0.1)
        q_latent, q_hyper, st = net.encode(torch.from_numpy(x), cond)
        fwd = net(torch.from_numpy(x), cond)
    assert ut is not None
    for i, o in enumerate(outs):
        put(rec, f"{tag}_dec{i}", o.numpy(), full)
    put(rec, f"{tag}_mean", mean.numpy(), full)
    put(rec, f"{tag}_scale", scale.numpy(), full)
    put(rec, f"{tag}_latent", st["latent"].numpy(), full)
    put(rec, f"{tag}_hyper_latent", st["hyper_latent"].numpy(), full)
    put(rec, f"{tag}_q_latent", fwd["q_latent"].numpy(), full)
    put(rec, f"{tag}_q_hyper_latent", fwd["q_hyper_latent"].numpy(), full)
    rec[f"{tag}_bpp"] = fwd["bpp"].numpy()
    for i, o in enumerate(fwd["output"]):
        put(rec, f"{tag}_ctx{i}", o.numpy(), False)
    rec[f"{tag}_rates"] = np.array(rates, np.float32)
    rec[f"{tag}_B"] = np.array(B)
    return fwd


def gen_vbr(name):
    kw, full = VBR[name]
    ref = import_reference("epsilonparam")
    net = ref.cm.BigCompressor(vbr=True, **kw)
    man = [(k, list(v.shape)) for k, v in net.state_dict().items() if k.startswith(KEEP)]
    sd = synth.compressor_state_dict(man, seed=SEED_W)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net.eval()
    rneg = negative_rate(net)
    for s in vbr_sites(net):                                  # the assertion the negative-rate case stands on
        assert bool(((s.scale.weight.reshape(-1) * rneg + s.scale.bias) < 0).any())
    cases = {"distinct": (DISTINCT, 3), "bcast": (BCAST, 2), "neg": ([rneg, ORDINARY], 2)}
    rec = {}
    for tag, (rates, B) in cases.items():
        run_case(ref, net, rates, B, full, rec, tag)
    json.dump({"kwargs": {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()}, "vbr": True,
               "class": "BigCompressor", "tree": "epsilonparam", "manifest": man, "seed": SEED_W,
               "medians_shape": list(net.prior.medians.shape), "cases": {k: {"rates": v[0], "B": v[1]} for k, v in cases.items()},
               "negative_rate": rneg, "image_hw": list(IMG_HW), "latent_hw": list(LAT_HW), "hyper_hw": list(HYP_HW),
               "seeds": {"image": SEED_IMG, "q_latent": SEED_Q, "q_hyper": SEED_QH}},
              open(os.path.join(HERE, f"manifest_{name}.json"), "w"))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    print(name, "ok, negative rate", rneg, {t: rec[f"{t}_bpp"] for t in cases})


E2E_COMP = dict(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3)
E2E_RATES = [0.0, 0.37, 1.0]


def gen_vbr_e2e(steps=3):
    """GaussianDiffusion.compress of the real reference with a VBR context model: the small eps U-Net (CONFIGS small_eps,
    synthetic parameters as in make_golden.gen_unet), 32 x 32 images, three images at three rates, DDIM, fixed init."""
    tree = "epsilonparam"
    ref = import_reference(tree)
    _, ukw, _, H, W, _ = mg.CONFIGS["small_eps"]
    un = ref.unet.Unet(**ukw)
    mg.load_synth(un, seed=0, final_gain=0.2)
    comp = ref.cm.BigCompressor(vbr=True, **E2E_COMP)
    man = [(k, list(v.shape)) for k, v in comp.state_dict().items() if k.startswith(KEEP)]
    sd = synth.compressor_state_dict(man, seed=SEED_W)
    comp.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    comp.eval()
    B = len(E2E_RATES)
    x = synth.normal("vbr_e2e_image", (B, 3, H, W), seed=SEED_IMG, std=0.5).clip(-1, 1).astype(np.float32)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    dkw = dict(mg.DIFF[tree], vbr=True)
    diff = ref.dd.GaussianDiffusion(denoise_fn=un, context_fn=comp, **dkw)
    diff.eval()
    with torch.no_grad():
        rec, bpp = diff.compress(torch.from_numpy(x), sample_steps=steps, bitrate_scale=torch.tensor(E2E_RATES),
                                 sample_mode="ddim", bpp_return_mean=False, init=torch.from_numpy(init.copy()))
    json.dump({"unet_kwargs": ukw, "comp_kwargs": E2E_COMP, "comp_manifest": man, "unet_manifest": mg.manifest_of(un),
               "diffusion": dkw, "rates": E2E_RATES, "steps": steps, "H": H, "W": W, "seed": SEED_W},
              open(os.path.join(HERE, "manifest_vbr_e2e.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "vbr_e2e.npz"), rec=rec.numpy(), bpp=bpp.numpy(), rates=np.array(E2E_RATES, np.float32))
    print("vbr_e2e ok", bpp.numpy(), float(np.abs(rec.numpy()).max()))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for n in VBR:
        gen_vbr(n)
    gen_vbr_e2e()
