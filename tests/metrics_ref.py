"""Float64 restatement of the distortion definition of include/cdc_hip.h (cdc_distortion), for the tests only: NumPy, explicit
separable loops and explicit pooling.  The product never imports this module."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss():
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def saved_u8(x):
    """The byte cdc_frame_crop(..., CDC_ELEM_U8) writes: torch's float32 sequence clamp(-1, 1) / 2 + 0.5, * 255 + 0.5, clamp, truncate."""
    t = np.clip(x.astype(np.float32), np.float32(-1), np.float32(1)) * np.float32(0.5) + np.float32(0.5)
    t = t * np.float32(255) + np.float32(0.5)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def to_unit(x, as_saved=False):
    """An operand's window in [0, 1], float64."""
    if x.dtype == np.uint8:
        return x.astype(np.float64) / 255.0
    if as_saved:
        return saved_u8(x).astype(np.float64) / 255.0
    return np.clip(x.astype(np.float64), -1.0, 1.0) * 0.5 + 0.5


def to_bytes(x, as_saved=False):
    return x if x.dtype == np.uint8 else (saved_u8(x) if as_saved else None)


def psnr(a, b, saved_a=False, saved_b=False):
    """Per-image PSNR, float64 [B]: exact integer MSE for two byte operands, float64 otherwise."""
    ba, bb = to_bytes(a, saved_a), to_bytes(b, saved_b)
    out = np.empty(a.shape[0], np.float64)
    for i in range(a.shape[0]):
        if ba is not None and bb is not None:
            d = ba[i].astype(np.int64) - bb[i].astype(np.int64)
            mse = int((d * d).sum()) / (65025 * d.size)
        else:
            d = to_unit(a[i], saved_a) - to_unit(b[i], saved_b)
            mse = float((d * d).mean())
        out[i] = np.inf if mse == 0 else 10.0 * np.log10(1.0 / mse)
    return out


def next_side(s):
    return (s + 2 * (s % 2) - 2) // 2 + 1


def pyramid_sizes(H, W):
    out = [(H, W)]
    for _ in range(4):
        H, W = next_side(H), next_side(W)
        out.append((H, W))
    return out


def _filter_valid(x, g):
    """[..., H, W] -> [..., H - 10, W - 10]: the window along the rows, then along the columns."""
    H, W = x.shape[-2:]
    t = np.zeros(x.shape[:-2] + (H - 10, W), np.float64)
    for k in range(11):
        t += g[k] * x[..., k:k + H - 10, :]
    o = np.zeros(x.shape[:-2] + (H - 10, W - 10), np.float64)
    for k in range(11):
        o += g[k] * t[..., :, k:k + W - 10]
    return o


def _pool(x):
    """avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2)), the pad counted: one zero row / column at the top / left of an odd side."""
    H, W = x.shape[-2:]
    ph, pw = H % 2, W % 2
    p = np.zeros(x.shape[:-2] + (H + ph, W + pw), np.float64)
    p[..., ph:, pw:] = x
    return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) / 4.0


def ms_ssim_unit(x, y):
    """x, y float64 [B, 3, H, W] in [0, 1] -> (msssim [B], components after relu [B, 5, 3], components before relu [B, 5, 3])."""
    g = gauss()
    B = x.shape[0]
    pre = np.empty((B, 5, 3), np.float64)
    for l in range(5):
        m1, m2 = _filter_valid(x, g), _filter_valid(y, g)
        s1 = _filter_valid(x * x, g) - m1 * m1
        s2 = _filter_valid(y * y, g) - m2 * m2
        s12 = _filter_valid(x * y, g) - m1 * m2
        cs = (2.0 * s12 + C2) / (s1 + s2 + C2)
        ss = (2.0 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs
        pre[:, l, :] = (cs if l < 4 else ss).mean(axis=(-2, -1))
        if l < 4:
            x, y = _pool(x), _pool(y)
    comp = np.maximum(pre, 0.0)
    w = np.array(WEIGHTS, np.float64)
    return np.prod(comp ** w[None, :, None], axis=1).mean(axis=1), comp, pre


def ms_ssim(a, b, saved_a=False, saved_b=False):
    return ms_ssim_unit(to_unit(a, saved_a), to_unit(b, saved_b))


def picture(B, H, W, seed=0):
    """Smooth sinusoid pictures with a constant block in one corner, float64 [B, 3, H, W] in [0, 1]; image i differs from image j."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((B, 3, H, W), np.float64)
    for i in range(B):
        for c in range(3):
            f = 0.03 + 0.011 * c + 0.007 * (i + seed)
            out[i, c] = 0.5 + 0.3 * np.sin(f * x + 0.5 * c + i) * np.cos(0.8 * f * y + 0.3 * i) + 0.1 * np.sin(0.21 * x + 0.17 * y + c)
        out[i, :, : max(1, H // 4), : max(1, W // 3)] = 0.25 + 0.1 * i
    return np.clip(out, 0.0, 1.0)


def noisy(p, sigma, seed):
    """p plus Gaussian noise, clipped to [0, 1]."""
    return np.clip(p + np.random.default_rng(seed).normal(0.0, sigma, p.shape), 0.0, 1.0)


def as_f32(unit):
    """[0, 1] -> the float32 operand in [-1, 1]."""
    return (unit * 2.0 - 1.0).astype(np.float32)


def as_u8(unit):
    return np.round(unit * 255.0).astype(np.uint8)
