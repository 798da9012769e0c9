"""Float64 statement, derived bound, input classes and measures of the channel LayerNorm edge tests, shared by
tests/test_ln_ref_host.py (no GPU: the preconditions) and tests/test_gpu_ln_edges.py (the 25 kernels of csrc/aux_kernels.hip).

Statement.  x = sum of the K split-K slices (float64); per pixel mu = mean_c x, var = mean_c (x - mu)^2 (biased), D = sqrt(var + eps)
with eps = float32(1e-5); yhat = (x - mu) / D; y = yhat g + b, then ReLU, + shift[b, c], + resid.  The statistics of a call are
(mu, 1 / D); with an output they are those of the FINAL values, computed here from the array the caller passes (in the GPU test the
kernel's own y), so they carry the bound of a plain one-slice LayerNorm over that array.

Bound, element-wise, first order in u = 2^-24, for ANY order of the float32 sums (so one formula serves every kernel), with per
pixel S1 = sum_c sum_k |slice_k,c|, d = x - mu:
    e_x(c)  = (K - 1) u sum_k |slice_k,c|                        K - 1 additions of partial sums no larger than that
    e_mu    = (C + 1) u S1 / C + mean_c e_x                      C - 1 additions + the division (or fl(1 / C) and a product: 2)
    e_d(c)  = e_x + e_mu + u |d_c|
    e_var   = [(C + 3) u sum d^2 + 2 sum |d| e_d + sum e_d^2] / C
    r_D     = e_var / (2 D^2) + 2 u                              the addition of eps and the root
    e_y(c)  = |g_c| (e_d / D + |yhat_c| (r_D + 2 u)) + 2 u (|g_c yhat_c| + |b_c|)
              + u |y + shift| (with a shift) + u |y + shift + resid| (with a residual)          ReLU is 1-Lipschitz
    bound   = 1.05 e_y + 2^-149;   the mean is held to 1.05 e_mu + 2^-149, rstd to 1.05 (r_D + 2 u) / D.
1.05 covers the second-order terms (at most 3e-3 of the first-order ones on the classes below).  tests/test_ln_ref_host.py shows that
float32 restatements in every kernel's summation order stay inside it, and that a one-pass variance, a misplaced or wrong eps, a
division by C - 1 and statistics taken before the residual leave it.

Classes (every draw through cdc_compression_amd.synth: a case is a pure function of its arguments):
  normal    0.5 + 2 n.
  offset    1024 + n: the cancellation in x - mu (at C = 48 the bound is 2 % of a unit-variance result at most, its median 0.6 %).
  small     1e-4 n: var < eps, eps decides.
  wide      n 2^e, e an integer uniform in [-20, 12).
  big       1e15 n: squares near 1e30, finite.
  constant  every value 0.75 and C a power of two (the 16-byte kernels multiply by fl(1 / C), exact only then): every sum is exact,
            the mean is 0.75 bit for bit, x - mu = 0 and y is the float32 chain b, ReLU, + shift, + resid bit for bit.
  index     normal x, g = 0, b_c = c - 8, shift[b, c] = 1024 b + c, resid[b, c, p] = (p mod 300) + 300 c + 153600 (b mod 64): all
            integers whose sums stay below 2^24, so y = max(c - 8, 0) + shift + resid exactly and a wrong channel, image or pixel
            index is an error of at least 1.
Slices (K > 1): slice_k = fl(x w_k) with seeded w_k > 0, sum w_k = 1, the last slice the float32 remainder x - slice_0 - ...; no slice
exceeds |x| (asserted in the host test), so the bound stays at the one-slice level."""
import numpy as np

from cdc_compression_amd import synth

U = 2.0 ** -24
EPS = np.float32(1e-5)
TINY = 2.0 ** -149
CLASSES = ("normal", "offset", "small", "wide", "big", "constant", "index")
NUMERIC_CLASSES = ("offset", "small", "wide", "big")

CHANNEL_EDGES = (1, 3, 31, 32, 33, 40, 127, 128, 129, 320, 383, 384)
PIXEL_EDGES = (1, 3, 4, 5, 7, 8, 31, 32, 33, 36, 63, 64, 65, 68, 255, 256, 260)
RULE_SHAPES = (          # (B, HW, (kind, width, img_major)): the smallest shapes at which the production rule picks each form
    (32, 256, (2, 8, 0)), (16, 256, (2, 4, 1)), (17, 256, (2, 4, 0)), (2, 64, (2, 2, 0)), (8, 16, (2, 2, 1)),
    (2, 63, (1, 8, 0)), (2, 65, (1, 8, 0)), (86, 65, (1, 32, 0)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp_distance(a, b):
    """Largest distance in float32 steps between two finite float32 arrays."""
    def key(v):
        i = bits(v).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if np.size(a) else 0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def ln_x(cls, B, C, HW, seed=0):
    shape = (B, C, 1, HW)
    n = synth.normal(f"ln_edge_x_{cls}", shape, seed).astype(np.float64)
    if cls in ("normal", "index"):
        x = 0.5 + 2.0 * n
    elif cls == "offset":
        x = 1024.0 + n
    elif cls == "small":
        x = 1e-4 * n
    elif cls == "wide":
        x = n * 2.0 ** np.floor(synth.uniform("ln_edge_x_wide_e", shape, seed, -20.0, 12.0))
    elif cls == "big":
        x = 1e15 * n
    elif cls == "constant":
        x = np.full(shape, 0.75)
    else:
        raise ValueError(cls)
    return x.astype(np.float32)


def make_slices(x, K, seed=0):
    """[K, *x.shape] float32 with the properties of the module docstring; K = 1: x itself."""
    if K == 1:
        return x[None].copy()
    w = synth.uniform("ln_edge_slice_w", (K,), seed, 0.5, 1.5)
    w = (w / w.sum()).astype(np.float32)
    out = np.empty((K,) + x.shape, np.float32)
    rest = x.copy()
    for k in range(K - 1):
        out[k] = x * w[k]
        rest = rest - out[k]
    out[K - 1] = rest
    return out


def ln_case(cls, B, C, HW, K=1, seed=0):
    """{"slices" [K, B, C, 1, HW], "g", "b" [C], "shift" [B, C], "resid" [B, C, 1, HW]} of class `cls`, float32."""
    x = ln_x(cls, B, C, HW, seed)
    if cls == "index":
        c, b, p = np.arange(C), np.arange(B), np.arange(HW)
        g = np.zeros(C, np.float32)
        bb = (c - 8).astype(np.float32)
        shift = (1024 * b[:, None] + c[None, :]).astype(np.float32)
        resid = ((p % 300)[None, None, :] + 300 * c[None, :, None] + 153600 * (b % 64)[:, None, None]).astype(np.float32).reshape(B, C, 1, HW)
    else:
        g = synth.normal("ln_edge_g", (C,), seed, 0.2, 1.0)
        bb = synth.normal("ln_edge_b", (C,), seed, 0.5, 0.3)
        shift = synth.normal("ln_edge_shift", (B, C), seed, 0.5)
        resid = synth.normal("ln_edge_resid", (B, C, 1, HW), seed, 1.0)
    return {"slices": make_slices(x, K, seed), "g": g, "b": bb, "shift": shift, "resid": resid}


def index_closed_form(case):
    """y of class `index` with ReLU, shift and residual, exactly."""
    B, C = case["shift"].shape
    return (np.maximum(case["b"], 0).reshape(1, C, 1, 1) + case["shift"].reshape(B, C, 1, 1) + case["resid"]).astype(np.float32)


def constant_closed_form(case, relu=True, shift=True, resid=True):
    """y of class `constant`: the float32 chain b, ReLU, + shift, + resid."""
    B, C = case["shift"].shape
    y = np.broadcast_to(case["b"].reshape(1, C, 1, 1), case["resid"].shape).astype(np.float32)
    if relu:
        y = np.maximum(y, np.float32(0))
    if shift:
        y = y + case["shift"].reshape(B, C, 1, 1)
    if resid:
        y = y + case["resid"]
    return y.astype(np.float32)


def sum_slices32(slices):
    """The float32 serial sum in slice order, as every kernel adds them on load."""
    v = np.array(slices[0], np.float32)
    for k in range(1, len(slices)):
        v = v + np.asarray(slices[k], np.float32)
    return v


# ---- float64 statement and bound ------------------------------------------------------------------------------------------------
def _stats64(x):
    mu = x.mean(axis=1, keepdims=True)
    d = x - mu
    var = (d * d).mean(axis=1, keepdims=True)
    return mu, d, var, np.sqrt(var + float(EPS))


def ln_f64(slices, g=None, b=None, relu=False, shift=None, resid=None):
    """-> {"mean", "rstd" [B, 1, HW], "y" [B, C, 1, HW] (None without g)}, float64, of the statement above."""
    x = np.asarray(slices, np.float64).sum(axis=0)
    B, C = x.shape[:2]
    mu, d, var, D = _stats64(x)
    out = {"mean": mu[:, 0], "rstd": 1.0 / D[:, 0], "y": None}
    if g is not None:
        y = d / D * np.asarray(g, np.float64).reshape(1, C, 1, 1) + np.asarray(b, np.float64).reshape(1, C, 1, 1)
        if relu:
            y = np.maximum(y, 0.0)
        if shift is not None:
            y = y + np.asarray(shift, np.float64).reshape(B, C, 1, 1)
        if resid is not None:
            y = y + np.asarray(resid, np.float64)
        out["y"] = y
    return out


def ln_bound(slices, g=None, b=None, relu=False, shift=None, resid=None):
    """-> {"mean", "rstd", "y"}: the element-wise bounds of the module docstring for the same arguments as ln_f64."""
    s = np.asarray(slices, np.float64)
    K, B, C = s.shape[:3]
    x = s.sum(axis=0)
    sabs = np.abs(s).sum(axis=0)
    e_x = (K - 1) * U * sabs
    S1 = sabs.sum(axis=1, keepdims=True)
    e_mu = (C + 1) * U * S1 / C + e_x.mean(axis=1, keepdims=True)
    mu, d, var, D = _stats64(x)
    e_d = e_x + e_mu + U * np.abs(d)
    e_var = ((C + 3) * U * (d * d).sum(axis=1, keepdims=True) + 2 * (np.abs(d) * e_d).sum(axis=1, keepdims=True)
             + (e_d * e_d).sum(axis=1, keepdims=True)) / C
    r_D = e_var / (2 * D * D) + 2 * U
    out = {"mean": 1.05 * e_mu[:, 0] + TINY, "rstd": 1.05 * (r_D + 2 * U)[:, 0] / D[:, 0], "y": None}
    if g is not None:
        g64, b64 = np.asarray(g, np.float64).reshape(1, C, 1, 1), np.asarray(b, np.float64).reshape(1, C, 1, 1)
        yhat = d / D
        e_y = np.abs(g64) * (e_d / D + np.abs(yhat) * (r_D + 2 * U)) + 2 * U * (np.abs(g64 * yhat) + np.abs(b64))
        y = yhat * g64 + b64
        if relu:
            y = np.maximum(y, 0.0)
        if shift is not None:
            y = y + np.asarray(shift, np.float64).reshape(B, C, 1, 1)
            e_y = e_y + U * np.abs(y)
        if resid is not None:
            y = y + np.asarray(resid, np.float64)
            e_y = e_y + U * np.abs(y)
        out["y"] = 1.05 * e_y + TINY
    return out


def worst_fraction(got, want, bound, what):
    """Prints, then asserts: max |got - want| / bound <= 1 (a non-finite result counts as infinite).  -> the fraction."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(want) == np.shape(bound), (what, got.dtype, got.shape, np.shape(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got.astype(np.float64) - want) / bound
    r = np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)
    f = float(r.max()) if r.size else 0.0
    print(f"[ln-edges] {what}: worst error {f:.3f} of the bound")
    assert f <= 1.0, (what, f, np.unravel_index(int(np.argmax(r)), r.shape))
    return f


def fraction(got, want, bound):
    """worst_fraction without the print and the assertion (for the variants that must LEAVE the bound)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(np.asarray(got, np.float64) - want) / bound
    return float(np.where(np.isfinite(r), r, np.inf).max())


def final_stats_f64(y):
    """(mean, rstd, bound of the mean, bound of rstd) of the final values `y` (float32: the kernel's own output)."""
    ref, bnd = ln_f64(y[None]), ln_bound(y[None])
    return ref["mean"], ref["rstd"], bnd["mean"], bnd["rstd"]


# ---- the former form rule -------------------------------------------------------------------------------------------------------
def old_form(B, C, HW, nparts=1, aligned=True, no_vec=False, vec_cols=None, no_img_major=False, min_wgs=256):
    """(kind, width, np, img_major) as ln_launch chose them before ln_form owned the choice (C > 384 with nparts > 1 is refused)."""
    def cd(a, b):
        return -(-a // b)
    if C <= 384 and 1 <= nparts <= 6 and HW % 4 == 0 and (B * C * HW) % 4 == 0 and aligned and not no_vec:
        cols = 8 if cd(HW, 32) * B >= min_wgs else (4 if cd(HW, 16) * B >= min_wgs else 2)
        if vec_cols in (8, 4, 2):
            cols = vec_cols
        if nparts > 4:
            cols = 2
        return 2, cols, nparts, int(cols < 8 and B % 8 == 0 and HW > 4 * cols and not no_img_major)
    if C <= 384:
        pl8 = HW <= 64 or cd(HW, 32) * B < min_wgs
        return 1, 8 if pl8 else 32, nparts if 1 <= nparts <= 4 else 0, 0
    return 0, 256 if HW >= 256 else 64, 1, 0


# ---- float32 restatements in each kind's reduction order (figures; the host test holds them to the bound) ------------------------
def _serial(a, axis, square=False):
    """Serial float32 sum along `axis`; square: of the squares, s = s + fl(a a)."""
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0)
    s = np.zeros_like(a[0]) if square else a[0].copy()
    for i in range(0 if square else 1, a.shape[0]):
        s = s + a[i] * a[i] if square else s + a[i]
    return s


def _channel_sum32(v, kind, width, square=False):
    """sum over axis 1 of v [B, C, 1, HW] float32 (of its squares with `square`) in the order of the kernel `kind` at `width`;
    -> [B, 1, 1, HW].  No fused operation: ln_kernel_vec is compiled that way, the other two are restated that way."""
    B, C = v.shape[:2]
    sq = bool(square)
    if kind == 0:
        return _serial(v, 1, sq)[:, None]
    CS = 256 // width
    NV = 384 // CS
    pad = np.zeros((B, CS * NV) + v.shape[2:], np.float32)
    pad[:, :C] = v
    part = _serial(pad.reshape((B, NV, CS) + v.shape[2:]), 1, sq)      # thread cs: channels cs + CS i, i ascending
    if kind == 1:
        return _serial(part, 1)[:, None]                              # slices 0, 1, ..., CS - 1 through LDS
    per_wave = 64 // width                                             # kind 2: butterfly inside a wave, then the four waves
    w = part.reshape((B, 4, per_wave) + v.shape[2:])
    while w.shape[2] > 1:
        w = w[:, :, 0::2] + w[:, :, 1::2]
    return _serial(w[:, :, 0], 1)[:, None]


def ln_f32(slices, kind, width, g=None, b=None, relu=False, shift=None, resid=None, want_final_stats=False, one_pass=False,
           eps_outside=False, eps=EPS, ddof=0, stats_before_resid=False):
    """Float32 restatement of the kernel `kind` (0 ln_kernel, 1 sliced, 2 vec) at `width`, every operation rounded on its own: that
    is how ln_kernel_vec is compiled; in the other two the compiler fuses some pairs (figures in profiles/ln_edges.md).  The keyword
    variants are the WRONG kernels of the host test.  -> {"mean", "rstd", "y"} (the statistics of the final values with
    want_final_stats)."""
    v = sum_slices32(slices)
    B, C = v.shape[:2]
    f32 = np.float32

    def stats(t):
        tot = _channel_sum32(t, kind, width)
        mean = tot * (f32(1) / f32(C)) if kind == 2 else tot / f32(C)
        if one_pass:
            var = _channel_sum32(t, kind, width, square=True) / f32(C) - mean * mean
        else:
            d = t - mean
            var = _channel_sum32(d, kind, width, square=True)
            var = var * (f32(1) / f32(C - ddof)) if kind == 2 else var / f32(C - ddof)
        with np.errstate(invalid="ignore"):
            den = (np.sqrt(var) + f32(eps)) if eps_outside else np.sqrt(var + f32(eps))
        return mean, den
    mean, den = stats(v)
    out = {"mean": mean[:, 0], "rstd": (f32(1) / den)[:, 0], "y": None}
    if g is None:
        return out
    g32, b32 = np.asarray(g, f32).reshape(1, C, 1, 1), np.asarray(b, f32).reshape(1, C, 1, 1)
    yhat = (v - mean) / den
    y = yhat * g32 + b32
    if relu:
        y = np.maximum(y, f32(0))
    if shift is not None:
        y = y + np.asarray(shift, f32).reshape(B, C, 1, 1)
    before = y
    if resid is not None:
        y = y + np.asarray(resid, f32)
    out["y"] = y
    if want_final_stats:
        m2, d2 = stats(before if stats_before_resid else y)
        out["mean"], out["rstd"] = m2[:, 0], (f32(1) / d2)[:, 0]
    return out
