#!/usr/bin/env python3
"""Golden vectors of the GDN context model (epsilonparam SimpleCompressor) and of its GDN1 operator from the REAL reference.

Same rules as make_golden.py, whose helpers this imports: the reference's own modules run on the PyTorch CPU path with the
deterministic synthetic parameters of cdc_compression_amd.synth (`simple_compressor_state_dict`), and only data is stored.

    python tests/golden/make_golden_simple.py          # ~1 min

gdn_ops.npz        per case k of GDN_SHAPES: raw beta / gamma, the reference's float32 beta' / gamma' (GDN.forward's expressions),
                   and -- for every case but the largest -- the outputs of the reference GDN1 module, forward (`y`) and inverse
                   (`yinv`).  The inputs are synth.gdn_input(shape, seed) (bit-identical on every host), so they are not stored.
gdn_ops_b3_y.npz / gdn_ops_b3_yinv.npz   the two outputs of the largest case (3, 48, 33, 31), one file each (file size limit).
simple_small       dim 16, full tensors; simple_full: dim 64, digests.  Each: decode from a synthetic rounded q_latent, hyper_dec,
                   encode (latent, hyper_latent), forward (q_latent, q_hyper_latent, bpp, pyramid); manifest_simple_*.json has
                   the reference's key order and shapes.  Every encode also runs in float64 (net.double()): the number of symbols
                   in which the float32 reference differs from it is asserted to be <= max(1, 1e-4 n) and stored (`flips_*`).
simple_e2e         GaussianDiffusion.compress(images, 3, None, "ddim", init) on a 1 x 3 x 64 x 64 image: the small eps U-Net of
                   make_golden.py + a small SimpleCompressor of as many levels as that U-Net concatenates (E2E_COMP; the reference's
                   Unet.encode concatenates EVERY level it is given, so the four-level simple_small does not pair with it).
"""
import copy
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
GDN_SHAPES = [(1, 16, 5, 7), (3, 48, 33, 31), (2, 64, 16, 16), (1, 192, 9, 20)]
GDN_SPLIT = 1                     # the case whose outputs go to files of their own
SEED_GDN = 41
SIMPLE = {
    # name: (ctor kwargs, image shape, full tensors?)
    "simple_small": (dict(dim=16, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3), (2, 3, 64, 128), True),
    "simple_full": (dict(dim=64, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=3), (1, 3, 64, 64), False),
}
SEED_W, SEED_IMG, SEED_Q, SEED_QH = 35, 36, 37, 38


def gen_gdn_ops():
    ref = import_reference("epsilonparam")
    rec = {"shapes": np.array(GDN_SHAPES), "seed": np.array(SEED_GDN)}
    for k, shape in enumerate(GDN_SHAPES):
        C = shape[1]
        beta, gamma = synth.gdn_layer_params(C, seed=SEED_GDN + k)
        x = synth.gdn_input(shape, seed=SEED_GDN + k)
        outs = {}
        for inverse in (False, True):
            m = ref.nc.GDN1(C, inverse)
            with torch.no_grad():
                m.beta.copy_(torch.from_numpy(beta))
                m.gamma.copy_(torch.from_numpy(gamma))
                outs["yinv" if inverse else "y"] = m(torch.from_numpy(x)).numpy()
                # GDN.forward's own expressions (network_components.py:392-397)
                import modules.utils as ut
                b2 = ut.LowerBound.apply(m.beta, m.beta_bound) ** 2 - m.pedestal
                g2 = ut.LowerBound.apply(m.gamma, m.gamma_bound) ** 2 - m.pedestal
        assert b2.dtype == torch.float32 and g2.dtype == torch.float32
        assert float(beta[0]) < m.beta_bound and (gamma < m.gamma_bound).mean() > 0.3       # the clamps act
        assert np.isfinite(outs["y"]).all() and np.isfinite(outs["yinv"]).all()
        rec.update({f"c{k}_beta": beta, f"c{k}_gamma": gamma, f"c{k}_beta_r": b2.numpy(), f"c{k}_gamma_r": g2.numpy()})
        if k == GDN_SPLIT:
            for key, v in outs.items():
                np.savez_compressed(os.path.join(HERE, f"gdn_ops_b3_{key}.npz"), **{key: v})
        else:
            rec.update({f"c{k}_{key}": v for key, v in outs.items()})
    np.savez_compressed(os.path.join(HERE, "gdn_ops.npz"), **rec)
    print("gdn_ops ok")


def put(rec, key, a, full):
    a = np.asarray(a, np.float32)
    if full or a.size <= 12288:
        rec[key] = a
    d = digest(a)
    rec.update({f"{key}_shape": np.array(a.shape), f"{key}_idx": d["idx"], f"{key}_val": d["val"], f"{key}_sum": d["sum"]})


def build(ref, kw):
    net = ref.cm.SimpleCompressor(**kw)
    man = [(k, list(v.shape)) for k, v in net.state_dict().items() if k.startswith(KEEP)]
    sd = synth.simple_compressor_state_dict(man, seed=SEED_W)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net.eval()
    return net, man


def flips(a32, a64):
    """Symbols in which the float32 reference differs from its float64 evaluation, with the cap the GPU test allows itself."""
    d = np.abs(np.asarray(a32, np.float64) - np.asarray(a64, np.float64))
    near = d <= 1.5e-5 * max(1.0, float(np.abs(a64).max()))        # the dequantised symbols carry the predicted mean: round-off
    assert (near | (np.abs(d - 1.0) <= 1e-3)).all()                # ... or one quantisation step
    n = int((~near).sum())
    cap = max(1, int(1e-4 * a32.size))
    assert n <= cap, (n, cap, "pick another image seed")
    return n


def inputs(net, shape):
    B, _, H, W = shape
    n, nh = len(net.enc), len(net.hyper_enc)
    x = synth.normal("simple_image", shape, seed=SEED_IMG, std=0.5).clip(-1, 1).astype(np.float32)
    q = np.round(synth.normal("simple_q_latent", (B, net.reversed_dims[0], H >> n, W >> n), seed=SEED_Q, std=2.0)).astype(np.float32)
    qh = (np.round(synth.normal("simple_q_hyper", (B, net.reversed_hyper_dims[0], H >> (n + nh - 1), W >> (n + nh - 1)), seed=SEED_QH,
                                std=2.0)) + 0.25).astype(np.float32)
    return x, q, qh


def gen_simple(name):
    kw, shape, full = SIMPLE[name]
    ref = import_reference("epsilonparam")
    net, man = build(ref, kw)
    x, q, qh = inputs(net, shape)
    rec = {}
    with torch.no_grad():
        outs = net.decode(torch.from_numpy(q))
        h = torch.from_numpy(qh)
        for deconv, _, act in net.hyper_dec:
            h = act(deconv(h))
        mean, scale = h.chunk(2, 1)
        scale = scale.clamp(min=0.1)
        fwd = net(torch.from_numpy(x))
        q_latent, q_hyper, st = net.encode(torch.from_numpy(x))
        net64 = copy.deepcopy(net).double()
        q_latent64, q_hyper64, _ = net64.encode(torch.from_numpy(x).double())
    for i, o in enumerate(outs):
        put(rec, f"dec{i}", o.numpy(), full)
    put(rec, "mean", mean.numpy(), full)
    put(rec, "scale", scale.numpy(), full)
    put(rec, "latent", st["latent"].numpy(), full)
    put(rec, "hyper_latent", st["hyper_latent"].numpy(), full)
    put(rec, "q_latent", fwd["q_latent"].numpy(), True)
    put(rec, "q_hyper_latent", fwd["q_hyper_latent"].numpy(), True)
    rec["bpp"] = fwd["bpp"].numpy()
    for i, o in enumerate(fwd["output"]):
        put(rec, f"ctx{i}", o.numpy(), False)
    rec["flips_q_latent"] = np.array(flips(q_latent.numpy(), q_latent64.numpy()))
    rec["flips_q_hyper_latent"] = np.array(flips(q_hyper.numpy(), q_hyper64.numpy()))
    json.dump({"kwargs": {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()}, "class": "SimpleCompressor",
               "tree": "epsilonparam", "manifest": man, "seed": SEED_W, "image_shape": list(shape),
               "seeds": {"image": SEED_IMG, "q_latent": SEED_Q, "q_hyper": SEED_QH}},
              open(os.path.join(HERE, f"manifest_{name}.json"), "w"))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    print(name, "ok bpp", rec["bpp"], "flips", int(rec["flips_q_latent"]), int(rec["flips_q_hyper_latent"]),
          "max |ctx|", [float(o.abs().max()) for o in fwd["output"]])


E2E_COMP = dict(dim=16, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2), channels=3, out_channels=3)


def gen_simple_e2e(steps=3):
    tree = "epsilonparam"
    ref = import_reference(tree)
    _, ukw, _, _, _, _ = mg.CONFIGS["small_eps"]
    un = ref.unet.Unet(**ukw)
    mg.load_synth(un, seed=0, final_gain=0.2)
    ckw = E2E_COMP
    comp, man = build(ref, ckw)
    B, H, W = 1, 64, 64
    x = synth.normal("simple_e2e_image", (B, 3, H, W), seed=SEED_IMG, std=0.5).clip(-1, 1).astype(np.float32)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    dkw = dict(mg.DIFF[tree])
    diff = ref.dd.GaussianDiffusion(denoise_fn=un, context_fn=comp, **dkw)
    diff.eval()
    with torch.no_grad():
        rec, bpp = diff.compress(torch.from_numpy(x), steps, None, "ddim", bpp_return_mean=False, init=torch.from_numpy(init.copy()))
        q32 = comp(torch.from_numpy(x))["q_latent"].numpy()
        q64 = copy.deepcopy(comp).double()(torch.from_numpy(x).double())["q_latent"].numpy()
    nflip = flips(q32, q64)
    json.dump({"unet_kwargs": ukw, "comp_kwargs": {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in ckw.items()},
               "comp_manifest": man, "unet_manifest": mg.manifest_of(un), "diffusion": dkw, "steps": steps, "H": H, "W": W, "seed": SEED_W,
               "image_seed": SEED_IMG},
              open(os.path.join(HERE, "manifest_simple_e2e.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "simple_e2e.npz"), rec=rec.numpy(), bpp=bpp.numpy(), flips_q_latent=np.array(nflip))
    print("simple_e2e ok", bpp.numpy(), float(np.abs(rec.numpy()).max()), "flips", nflip)


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_gdn_ops()
    for n in SIMPLE:
        gen_simple(n)
    gen_simple_e2e()
