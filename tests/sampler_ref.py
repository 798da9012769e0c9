"""The sampler kernels' arithmetic stated in NumPy: one DDIM update in float64 with a derived elementwise rounding bound, the same update
operation by operation in float32, the prediction x0 both update rules share, and the row combine of the final convolution's planes.
Test infrastructure without a GPU: tests/test_sampler_ref_host.py checks it against itself, tests/test_gpu_ddim_update.py and
tests/test_gpu_solver.py check the kernels against it.

Operation order: the reference's ddim() (x tree: xparam/modules/denoising_diffusion.py:152-174, eps tree:
epsilonparam/modules/denoising_diffusion.py:137-152):
    x0   = fx | sqrt_recip x - sqrt_recipm1 fx | sqrt_ac x - sqrt_one_minus_ac fx          (pred_mode x | noise | v), then the clamp
    eps  = fx  (pred_mode noise)   |   (sqrt_recip x - x0) / sqrt_recipm1                  (x, v: from the CLAMPED x0)
    sig  = eta sigma;   var = one_minus_ac_prev - sig^2,  x tree only: .clamp(min=0);   c_eps = sqrt(var)
    x'   = (sqrt_ac_prev x0 + c_eps eps) + sig noise
"""
import math
from fractions import Fraction

import numpy as np

from cdc_compression_amd import _lib
from cdc_compression_amd.schedule import SampleSchedule

U = 2.0 ** -24        # unit roundoff of float32
PRED_X, PRED_NOISE, PRED_NOISE_XTREE, PRED_V = _lib.CDC_PRED_X, _lib.CDC_PRED_NOISE, _lib.CDC_PRED_NOISE_XTREE, _lib.CDC_PRED_V
CLIP_NONE, CLIP_ALL, CLIP_HALF = _lib.CDC_CLIP_NONE, _lib.CDC_CLIP_ALL, _lib.CDC_CLIP_HALF
PREDS = (PRED_X, PRED_NOISE, PRED_NOISE_XTREE, PRED_V)
CLIPS = (CLIP_ALL, CLIP_NONE, CLIP_HALF)

# ---- the cases both DDIM test files run ------------------------------------------------------------------------------------------
STEPS = 5
STEP_LIST = (4, 2, 0)                 # 4: the first step a decode runs; 0: the last (one_minus_ac_prev = sigma = 0, smallest sqrt_recipm1)
ETAS = (0.0, 0.5, 1.0)                # no noise; a tensor; a tensor with var = one_minus_ac_prev - sigma^2 cancelling
ETA_OVER = 1.5                        # var < 0 at OVER_STEP in both trees, whichever way the compiler contracts it
OVER_STEP = 2
SHAPES = [(3, 3, 24, 44), (3, 3, 24, 42), (2, 3, 4, 4), (3, 3, 5, 7), (3, 3, 344, 342), (1, 65540, 1, 4)]
BIG = (3, 3, 344, 342)                # the grid-stride loop: two combinations only
BIG_COMBOS = ((PRED_X, CLIP_HALF, 0.5), (PRED_NOISE, CLIP_ALL, 1.0))


def schedules():
    """-> {"x": 5-step cosine x-tree schedule, "eps": 5-step linear eps-tree schedule}: what the two handles of the GPU test hold."""
    return {"x": SampleSchedule(8193, "cosine", "x", STEPS), "eps": SampleSchedule(20000, "linear", "eps", STEPS)}


def tree_of(pred):
    return "eps" if pred == PRED_NOISE else "x"


def combos(shape):
    """(pred, clip, eta) of the float64 comparison at `shape`."""
    if tuple(shape) == BIG:
        return list(BIG_COMBOS)
    return [(p, c, e) for p in PREDS for c in CLIPS for e in ETAS]


def inputs(shape, seed=5):
    """fx, x, noise: float32 tensors of `shape`."""
    from cdc_compression_amd import synth
    return tuple(synth.normal(n, shape, seed=seed, std=sd) for n, sd in (("fx", 1.2), ("x", 0.8), ("noise", 1.0)))


def n_clipped(B, clip):
    return {CLIP_NONE: 0, CLIP_ALL: B, CLIP_HALF: B // 2}[clip]


# ---- x0, shared by both update rules -----------------------------------------------------------------------------------------------
def predict_x0_f64(s, i, fx, x, pred, clip):
    """-> (x0 float64, clamp applied; e0: its rounding bound where the kernel computes it).  fx, x: float64 views of the float32
    tensors.  e0 = U (|p x| + |q fx| + |p x - q fx|): two products and one difference, each rounded once; 0 for pred_mode x."""
    d = lambda t: np.float64(t[i])                                   # noqa: E731
    if pred == PRED_X:
        x0, e0 = fx, np.zeros_like(fx)
    else:
        p, q = (d(s.sqrt_ac), d(s.sqrt_one_minus_ac)) if pred == PRED_V else (d(s.sqrt_recip), d(s.sqrt_recipm1))
        x0 = p * x - q * fx
        e0 = U * (np.abs(p * x) + np.abs(q * fx) + np.abs(x0))       # two products and one difference, each rounded once
    nclip = n_clipped(x.shape[0], clip)
    x0 = x0.copy()
    x0[:nclip] = np.clip(x0[:nclip], -1.0, 1.0)                       # (the clamp is exact and does not enlarge an error)
    return x0, e0


# ---- the step's scalars --------------------------------------------------------------------------------------------------------------
def _round_f32(fr):
    """The float32 nearest the rational fr, ties to even: one rounding, as a fused multiply-add rounds."""
    c = np.float32(float(fr))                                         # within one float32 step of the answer
    cands = sorted({float(c), float(np.nextafter(c, np.float32(-np.inf))), float(np.nextafter(c, np.float32(np.inf)))})
    even = lambda v: (int(np.float32(v).view(np.uint32)) & 1) == 0    # noqa: E731
    return np.float32(min(cands, key=lambda v: (abs(Fraction(v) - fr), not even(v))))


def step_scalars(s, i, eta, pred):
    """The float32 scalars a thread forms before its pixels (DdimRule's constructor), whose contraction is the compiler's:
        sig = fl(eta sigma[i])                                   one product: one value
        var = fl(one_minus_ac_prev[i] - fl(sig sig))             the product rounded (what the reference's tensor operations do)
           or fl(one_minus_ac_prev[i] - sig sig)                 the product exact (a fused multiply-add), by exact rational arithmetic
        x tree (pred != noise-of-the-eps-tree): var = max(var, 0);   c_eps = fl(sqrt(var))   (NaN for var < 0 in the eps tree)
    -> dict(sig, c_acp, c_1macp: float32; var: the two float32 candidates; c_eps: the two float32 candidates; c_eps64: sqrt of the
    exact var (clamped alike) in float64, NaN below zero; dc = max |candidate - c_eps64|: the spread and the candidates' own roundings)."""
    f = np.float32
    sig = f(f(eta) * f(s.sigma[i]))
    c1 = f(s.one_minus_ac_prev[i])
    exact = Fraction(float(c1)) - Fraction(float(sig)) ** 2
    var = [f(c1 - f(sig * sig)), _round_f32(exact)]
    if pred != PRED_NOISE:
        var = [max(v, f(0)) for v in var]
        exact = max(exact, Fraction(0))
    with np.errstate(invalid="ignore"):
        c_eps = [np.sqrt(v) for v in var]
    c64 = math.sqrt(exact) if exact >= 0 else float("nan")
    dc = max(abs(float(c) - c64) for c in c_eps)
    return dict(sig=sig, c_acp=f(s.sqrt_ac_prev[i]), c_1macp=c1, var=var, c_eps=c_eps, c_eps64=c64, dc=dc)


# ---- one DDIM update -------------------------------------------------------------------------------------------------------------------
def ddim_update_f64(s, i, fx, x, noise, eta, pred, clip):
    """One DDIM update in float64 from the float32 tables of the SampleSchedule `s`, and its elementwise rounding bound.
    fx, x, noise: float32 [B][C][H][W]; noise is None exactly when eta == 0.  -> (x_next, bound), float64.

    The bound (first order in U = 2^-24; every product, difference, quotient and sum of pixel values rounds once, nothing is fused):
        e0   = U (|p x| + |q fx| + |x0|)                        0 for pred_mode x; the clamp is exact and enlarges nothing, and where
                                                                the unclamped x0 is further than e0 outside [-1, 1] both sides clamp to
                                                                the same end: e0 = 0 there
        t    = sqrt_recip x,  d = t - x0,  eps = d / m          pred_mode x and v, m = sqrt_recipm1
        e_d  = U |t| + e0 + U |d|                               the product, x0's own error, the difference
        e_e  = e_d / |m| + U |eps|                              the quotient amplifies by 1 / |m|;  0 where eps = fx
        A = c_acp x0,  B = c_eps eps,  S = A + B,  N = sig noise,  R = S + N
        e_A  = c_acp e0 + U |A|
        e_B  = c e_e + U c |eps| + dc |eps|                     c: the larger float32 candidate of c_eps, dc: step_scalars' spread
        e_S  = e_A + e_B + U |S|
        e_R  = e_S + U |N| + U |R|                              with noise; e_S without
        bound = e_R (1 + 16 U)                                  the factor covers the terms of order U^2 of at most eight roundings
    sig is one float32 value (a single product), so the statement uses it as it is.  Where c_eps64 is NaN (eps tree, var < 0) the result
    and the bound are NaN everywhere, as the reference's are."""
    k = step_scalars(s, i, eta, pred)
    fx, x = fx.astype(np.float64), x.astype(np.float64)
    x0, e0 = predict_x0_f64(s, i, fx, x, pred, clip)
    free, _ = predict_x0_f64(s, i, fx, x, pred, CLIP_NONE)
    e0 = np.where((x0 != free) & (np.abs(free) - e0 * (1 + 16 * U) > 1.0), 0.0, e0)
    m = np.float64(s.sqrt_recipm1[i])
    if pred in (PRED_X, PRED_V):
        t = np.float64(s.sqrt_recip[i]) * x
        d = t - x0
        eps = d / m
        e_e = (U * np.abs(t) + e0 + U * np.abs(d)) / abs(m) + U * np.abs(eps)
    else:
        eps, e_e = fx, np.zeros_like(fx)
    c_acp, c64, sig = float(k["c_acp"]), k["c_eps64"], float(k["sig"])
    if math.isnan(c64):
        nan = np.full_like(x, np.nan)
        return nan, nan.copy()
    c = max(float(v) for v in k["c_eps"])
    A, Bt = c_acp * x0, c64 * eps
    S = A + Bt
    e_S = (c_acp * e0 + U * np.abs(A)) + (c * e_e + U * c * np.abs(eps) + k["dc"] * np.abs(eps)) + U * np.abs(S)
    if noise is None:
        assert eta == 0
        return S, e_S * (1 + 16 * U)
    N = sig * noise.astype(np.float64)
    R = S + N
    return R, (e_S + U * np.abs(N) + U * np.abs(R)) * (1 + 16 * U)


def ddim_update_f32(s, i, fx, x, noise, eta, pred, clip, c_eps=None, fused=False):
    """The same update operation by operation in float32: what the reference's element-wise tensor operations compute, and -- the kernels
    fuse nothing -- what they hold bit for bit, for one of step_scalars' two c_eps candidates (`c_eps`; default: the reference's, the
    rounded product).  fused=True: the WRONG form `fma(sqrt_recip, x, -x0)` of eps's numerator (the product not rounded)."""
    f = np.float32
    k = step_scalars(s, i, eta, pred)
    c_eps = f(k["c_eps"][0] if c_eps is None else c_eps)
    r, m = f(s.sqrt_recip[i]), f(s.sqrt_recipm1[i])
    if pred == PRED_X:
        x0 = fx.copy()
    elif pred == PRED_V:
        x0 = f(s.sqrt_ac[i]) * x - f(s.sqrt_one_minus_ac[i]) * fx
    else:
        x0 = r * x - m * fx
    nclip = n_clipped(x.shape[0], clip)
    x0[:nclip] = np.clip(x0[:nclip], f(-1), f(1))
    if pred in (PRED_X, PRED_V):
        if fused:
            num = (np.float64(r) * x.astype(np.float64) - x0.astype(np.float64)).astype(f)      # (the product is exact in float64)
        else:
            num = r * x - x0
        eps = num / m
    else:
        eps = fx
    with np.errstate(invalid="ignore"):
        out = k["c_acp"] * x0 + c_eps * eps
        if noise is not None:
            out = out + k["sig"] * noise
    assert out.dtype == np.float32
    return out


# ---- the row combine of the final convolution's partial planes ----------------------------------------------------------------------
def combine(planes, bias, pad, dtype=np.float32):
    """fx[b][c][y][x] = bias[c] + sum over ky ascending, rows inside the image, of planes[b][c][ky][y + ky - pad][x], summed in `dtype` in
    that order (additions only: in float32 the bits are defined).  planes [B][C][KH][H][W]; bias [C] or None.
    -> (fx, the sum of the terms' magnitudes in float64)."""
    B, C, KH, H, W = planes.shape
    fx = np.zeros((B, C, H, W), dtype)
    mag = np.zeros((B, C, H, W), np.float64)
    if bias is not None:
        fx += bias.astype(dtype)[None, :, None, None]
        mag += np.abs(bias.astype(np.float64))[None, :, None, None]
    for ky in range(KH):
        lo, hi = max(0, pad - ky), min(H, H + pad - ky)               # rows y with 0 <= y + ky - pad < H
        if lo < hi:
            term = planes[:, :, ky, lo + ky - pad:hi + ky - pad]
            fx[:, :, lo:hi] += term.astype(dtype)
            mag[:, :, lo:hi] += np.abs(term.astype(np.float64))
    return fx, mag
