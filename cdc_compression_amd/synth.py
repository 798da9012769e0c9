"""Deterministic synthetic weights / inputs for tests and bench (no checkpoints offline).

Counter-based generator built only from exact operations (uint64 hashing, integer sums, one
float64 multiply, one cast) so that this container, the GPU box and any future host produce
bit-identical float32 tensors -- unlike torch's or numpy's normal samplers, whose libm paths can
differ by an ulp between CPUs.  Used to inject identical parameters into the real reference
(tests/golden/make_golden.py), the CPU oracle and the HIP path.
"""
import numpy as np

_MASK = (1 << 64) - 1
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _fnv1a(s):
    h = 0xCBF29CE484222325
    for ch in s.encode():
        h ^= ch
        h = (h * 0x100000001B3) & _MASK
    return h


def _splitmix64(z):
    with np.errstate(over="ignore"):
        z = (z + _GOLD)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


_STD4 = float(np.sqrt(4.0 * (65536.0 ** 2 - 1.0) / 12.0))


def normal(name, shape, seed=0, std=1.0, mean=0.0):
    """Approximately N(mean, std^2) float32 tensor (Irwin-Hall n=4), a pure function of
    (name, seed, element index)."""
    n = int(np.prod(shape)) if len(shape) else 1
    base = np.uint64((_fnv1a(name) ^ (seed * 0xD6E8FEB86659FD93)) & _MASK)
    with np.errstate(over="ignore"):
        ctr = base + np.arange(n, dtype=np.uint64) * _GOLD
    r = _splitmix64(ctr)
    m = np.uint64(0xFFFF)
    s = ((r & m) + ((r >> np.uint64(16)) & m) + ((r >> np.uint64(32)) & m)
         + ((r >> np.uint64(48)) & m)).astype(np.int64) - 2 * 65535
    z = s.astype(np.float64) * (float(std) / _STD4) + float(mean)
    return z.astype(np.float32).reshape(shape)


def uniform(name, shape, seed=0, lo=0.0, hi=1.0):
    """U[lo, hi) float64 tensor, a pure function of (name, seed, element index): the top 53 bits of the same counter hash, times
    2^-53 (exact), then one multiply and one add.  The caller casts."""
    n = int(np.prod(shape)) if len(shape) else 1
    base = np.uint64((_fnv1a(name) ^ (seed * 0xD6E8FEB86659FD93)) & _MASK)
    with np.errstate(over="ignore"):
        ctr = base + np.arange(n, dtype=np.uint64) * _GOLD
    u = (_splitmix64(ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (u * (float(hi) - float(lo)) + float(lo)).reshape(shape)


def unet_state_dict(manifest, seed=0, final_gain=1.0):
    """Synthetic parameters for a Unet manifest [(name, shape), ...].

    Gains: conv/linear weights N(0, 1/fan_in); biases N(0, 0.1^2); LayerNorm g = 1 + N(0, 0.2^2),
    b = N(0, 0.2^2); to_qkv weights x2 (so the k-softmax is not flat); final conv x final_gain."""
    sd = {}
    for name, shape in manifest:
        shape = tuple(shape)
        if name.endswith(".g"):
            t = normal(name, shape, seed, 0.2, 1.0)
        elif name.endswith(".b"):
            t = normal(name, shape, seed, 0.2)
        elif name.endswith(".bias"):
            t = normal(name, shape, seed, 0.1)
        else:
            if name.endswith(".conv.weight") and len(shape) == 4 and shape[-1] == 4:
                fan_in = shape[0] * 4          # ConvTranspose2d [Cin][Cout][4][4], 2x2 taps/output
            else:
                fan_in = int(np.prod(shape[1:]))
            std = 1.0 / np.sqrt(max(fan_in, 1))
            if "to_qkv" in name:
                std *= 2.0
            if name.startswith("final_conv.1") or name.endswith("final_conv.1.weight"):
                std *= final_gain
            if name == "time_mlp.0.weight":
                std = 1.0
            t = normal(name, shape, seed, std)
        sd[name] = t
    return sd


def context_pyramid(cfg_context_channels, B, H, W, seed=3, std=0.5):
    """N(0, std^2) stand-in for `context_fn.decode(q_latent)`: list of [B, C_l, H/2^l, W/2^l]."""
    return [normal(f"ctx{l}", (B, c, H >> l, W >> l), seed, std)
            for l, c in enumerate(cfg_context_channels)]


def is_vbr_key(name):
    """A VBRCondition parameter (epsilonparam network_components.py:304-314): `<site>.scale.*` / `<site>.shift.*`."""
    parts = name.split(".")
    return len(parts) >= 2 and parts[-2] in ("scale", "shift") and parts[-1] in ("weight", "bias")


def compressor_state_dict(manifest, seed=0):
    """Synthetic parameters for a compressor manifest: `unet_state_dict` for every entry but the VBRCondition scalers,
    which keep the affine O(1) -- scale = 1 + N(0, 0.05^2) + N(0, 0.2^2) r, shift = N(0, 0.05^2) + N(0, 0.05^2) r -- instead of
    the N(0, 0.1^2) bias / N(0, 1) weight draws that would make the activations vanish.  The scale still changes sign in some
    channels at an extrapolated rate r (|r| of a few), which the golden generator pins."""
    sd = unet_state_dict([(n, s) for n, s in manifest if not is_vbr_key(n)], seed=seed)
    for name, shape in manifest:
        if not is_vbr_key(name):
            continue
        shape = tuple(shape)
        if name.endswith(".scale.weight"):
            t = normal(name, shape, seed, 0.2)
        elif name.endswith(".scale.bias"):
            t = normal(name, shape, seed, 0.05, 1.0)
        else:
            t = normal(name, shape, seed, 0.05)
        sd[name] = t
    return {n: sd[n] for n, _ in manifest}


def is_gdn_key(name):
    """A GDN1 parameter (epsilonparam network_components.py:330-345): `<layer>.beta` / `<layer>.gamma`."""
    return name.endswith(".beta") or name.endswith(".gamma")


def simple_compressor_state_dict(manifest, seed=0):
    """Synthetic parameters for a SimpleCompressor manifest: `unet_state_dict` for the convolutions and biases; per GDN1 layer
    beta = 1 + N(0, 0.1^2) with beta[0] = 0 (below the reparametrisation's bound: the clamp acts) and
    gamma = sqrt(0.1) I + N(0, 0.05^2) (about half of the off-diagonal entries are negative and clamp to the bound).  The
    normalisation pool stays near 1, so the activations stay O(1) through the levels."""
    sd = unet_state_dict([(n, s) for n, s in manifest if not is_gdn_key(n)], seed=seed)
    for name, shape in manifest:
        shape = tuple(shape)
        if name.endswith(".beta"):
            t = normal(name, shape, seed, 0.1, 1.0)
            t[0] = 0.0
        elif name.endswith(".gamma"):
            t = (normal(name, shape, seed, 0.05).astype(np.float64) + np.sqrt(0.1) * np.eye(shape[0])).astype(np.float32)
        else:
            continue
        sd[name] = t
    return {n: sd[n] for n, _ in manifest}


def gdn_layer_params(C, seed=0, name="gdn"):
    """(beta [C], gamma [C, C]) of one GDN1 layer, drawn as `simple_compressor_state_dict` draws them."""
    sd = simple_compressor_state_dict([(f"{name}.beta", (C,)), (f"{name}.gamma", (C, C))], seed=seed)
    return sd[f"{name}.beta"], sd[f"{name}.gamma"]


def gdn_input(shape, seed=0, name="gdn_x"):
    """N(0, 1) activations [B, C, H, W] for a GDN1 layer with a few special entries: flat indices 0, 7, 14, ... (every 7th of the
    first 35) are exact zeros, flat index 3 is +1e4 and the last element is -1e4."""
    x = normal(name, shape, seed, 1.0)
    flat = x.reshape(-1)
    flat[0:35:7] = 0.0
    flat[3] = 1e4
    flat[-1] = -1e4
    return x


# VGG16's convolutions inside lpips 0.1.4's LPIPS(net="vgg"): (slice, index in torchvision's vgg16().features, Cin, Cout)
LPIPS_VGG_CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256),
                   (3, 14, 256, 256), (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512),
                   (5, 28, 512, 512))
LPIPS_VGG_TAP_CHANNELS = (64, 128, 256, 512, 512)


def lpips_vgg_manifest():
    """[(name, shape)] of the LPIPS-VGG parameters below their prefix (include/cdc_hip.h: cdc_lpips), in the library's order."""
    man = []
    for sl, idx, cin, cout in LPIPS_VGG_CONVS:
        man += [(f"net.slice{sl}.{idx}.weight", (cout, cin, 3, 3)), (f"net.slice{sl}.{idx}.bias", (cout,))]
    return man + [(f"lin{k}.model.1.weight", (1, c, 1, 1)) for k, c in enumerate(LPIPS_VGG_TAP_CHANNELS)]


def lpips_vgg_state_dict(seed=0, prefix="", with_duplicates=False):
    """Synthetic LPIPS-VGG parameters: He-scaled convolutions N(0, 2 / fan_in), biases 0.05 + N(0, 0.01^2), non-negative `lin`
    weights |N(0, 1 / 32^2)| -- activations stay O(1) through the thirteen layers (below 20 on smoothed random images) and a copy of
    such an image with Gaussian noise of sigma 0.02 ... 0.3 scores 6e-4 ... 3e-2.
    with_duplicates: also the `lins.{k}` copies that the package's ModuleList registers."""
    sd = {}
    for name, shape in lpips_vgg_manifest():
        if name.endswith(".bias"):
            t = normal(name, shape, seed, 0.01, 0.05)
        elif name.startswith("lin"):
            t = np.abs(normal(name, shape, seed, 1.0 / 32.0))
        else:
            t = normal(name, shape, seed, float(np.sqrt(2.0 / (shape[1] * 9))))
        sd[prefix + name] = t
        if with_duplicates and name.startswith("lin"):
            sd[prefix + "lins." + name[3:]] = t.copy()
    return sd
