"""Float64 restatements of the LPIPS-VGG definition of include/cdc_hip.h (cdc_lpips), for the tests only.  Two of them, built
differently so that a slip in one shows against the other (tests/test_lpips_host.py holds them to 1e-12 relative):
  lpips_torch   torch CPU conv2d / max_pool2d in float64
  lpips_numpy   NumPy im2col + einsum, the pooling by reshape
Both take the operands' windows as given (float32 in [-1, 1], uint8, or float32 "as saved") and map them as metrics_ref.to_unit does.
The product never imports this module."""
import numpy as np

import metrics_ref as R
from cdc_compression_amd import synth

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
LEVELS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))       # indices into synth.LPIPS_VGG_CONVS; a pooling between levels


def _params(sd, prefix):
    g = lambda k: np.asarray(sd[prefix + k], np.float64)             # noqa: E731
    convs = [(g(f"net.slice{s}.{i}.weight"), g(f"net.slice{s}.{i}.bias")) for s, i, _, _ in synth.LPIPS_VGG_CONVS]
    lins = [g(f"lin{k}.model.1.weight").reshape(-1) for k in range(5)]
    shift = g("scaling_layer.shift").reshape(3) if prefix + "scaling_layer.shift" in sd else np.array(SHIFT)
    scale = g("scaling_layer.scale").reshape(3) if prefix + "scaling_layer.scale" in sd else np.array(SCALE)
    return convs, lins, shift, scale


def net_input(x, as_saved, shift, scale):
    """An operand's window -> the scaled network input, float64 [B, 3, H, W]."""
    return (2.0 * R.to_unit(x, as_saved) - 1.0 - shift[None, :, None, None]) / scale[None, :, None, None]


def _head(f0, f1, w):
    """One tap, float64 [B, C, h, w] each -> [B]: the direct form."""
    n0 = f0 / (np.sqrt((f0 * f0).sum(1, keepdims=True)) + EPS)
    n1 = f1 / (np.sqrt((f1 * f1).sum(1, keepdims=True)) + EPS)
    return (w[None, :, None, None] * (n0 - n1) ** 2).sum(1).mean(axis=(1, 2))


def _taps(x, convs, conv, pool):
    """The five taps of one operand (each operand runs on its own: identical operands then give identical features)."""
    out = []
    for l, idx in enumerate(LEVELS):
        if l:
            x = pool(x)
        for i in idx:
            x = np.maximum(conv(x, *convs[i]), 0.0)
        out.append(x)
    return out


def _lpips(sd, a, b, saved_a, saved_b, prefix, conv, pool):
    convs, lins, shift, scale = _params(sd, prefix)
    f0 = _taps(net_input(a, saved_a, shift, scale), convs, conv, pool)
    f1 = _taps(net_input(b, saved_b, shift, scale), convs, conv, pool)
    layers = np.stack([_head(f0[l], f1[l], lins[l]) for l in range(5)], axis=1)
    return layers.sum(1), layers


def pool_reshape(x):
    """max_pool2d(2, 2), floor mode: an odd side loses its last row / column."""
    B, C, H, W = x.shape
    return x[:, :, : H // 2 * 2, : W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def _conv_im2col(x, w, bias):
    B, C, H, W = x.shape
    p = np.zeros((B, C, H + 2, W + 2), np.float64)
    p[:, :, 1:-1, 1:-1] = x
    cols = np.stack([p[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=2)      # [B, C, 9, H, W]
    return np.einsum("bckhw,ock->bohw", cols, w.reshape(w.shape[0], C, 9), optimize=True) + bias[None, :, None, None]


def lpips_numpy(sd, a, b, saved_a=False, saved_b=False, prefix=""):
    """-> (lpips [B], layers [B, 5]) in float64."""
    return _lpips(sd, a, b, saved_a, saved_b, prefix, _conv_im2col, pool_reshape)


def lpips_torch(sd, a, b, saved_a=False, saved_b=False, prefix="", dtype="float64"):
    """-> (lpips [B], layers [B, 5]); dtype "float32" runs the convolutions and the pooling in torch's float32 (how far plain
    float32 arithmetic sits from the definition)."""
    import torch
    import torch.nn.functional as F
    td = getattr(torch, dtype)

    def conv(x, w, bias):
        y = F.conv2d(torch.from_numpy(x).to(td), torch.from_numpy(w).to(td), torch.from_numpy(bias).to(td), padding=1)
        return y.double().numpy()

    def pool(x):
        return F.max_pool2d(torch.from_numpy(x), 2, 2).numpy()

    return _lpips(sd, a, b, saved_a, saved_b, prefix, conv, pool)


def operands(B, H, W, seed=0):
    """A smoothed random picture and the picture plus Gaussian noise, sigma from 0.02 (image 0) to 0.3 (the last image),
    float64 in [0, 1]: -> (p, q)."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    p = rng.uniform(0.0, 1.0, (B, 3, H + 4, W + 4))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    p = sum(k[i] * p[:, :, i:i + H, :] for i in range(5))
    p = sum(k[i] * p[:, :, :, i:i + W] for i in range(5))
    p = np.clip(0.5 + 2.0 * (p - 0.5), 0.0, 1.0)
    sig = np.geomspace(0.02, 0.3, B) if B > 1 else np.array([0.05])
    q = np.clip(p + rng.normal(0.0, 1.0, p.shape) * sig[:, None, None, None], 0.0, 1.0)
    return p, q
