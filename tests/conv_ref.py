"""Float64 statement, input classes, derived element-wise bound, rms measure and float32 restatements of the convolution edge tests,
shared by tests/test_conv_ref_host.py (no GPU: the preconditions, the restatements, the wrong kernels) and
tests/test_gpu_conv_edges.py (every convolution family behind Ops.conv2d / Ops.conv_transpose2d).

Statement (float64).  y = conv(x, w) + bias (k x k, stride s, zero padding p), or the 4 x 4 / stride 2 / pad 1 transposed convolution;
then, where asked, the channel LayerNorm + ReLU of ln_ref.ln_f64, + shift[b, c], + resid.  Per output element the statement also gives
S = sum |x| |w| (the same convolution of |x| with |w|), X1 = sum |x| and W1 = sum |w| over its receptive field, and K, its number of
in-bounds products.

The three arithmetics (csrc/cdc_weights.hip: pack_conv, csrc/conv_kernel.h: split2h, csrc/conv_split_kernel.h), restated with numpy
float16 / bit masks and float64 products (all of them exact there):
  f16x2   activations h = fp16(a), l' = fp16((a - h) 2^11) (act_planes); weight scale s = 14 - e with max |w| = m 2^e, m in [0.5, 1),
          over the whole tensor, clamped to +-100 (weight_scale); WH = fp16(w 2^s), WL = fp16(w 2^s - WH), WH2 = fp16(WH 2^-11)
          (weight_planes); result (sum h WH + h WL + l' WH2) 2^-s.  Some kernels keep sum l' WH in a second accumulator and scale it
          by 2^-11 at the end: the same terms wherever WH2 is exact.
  bf16x3  CDC_ARITH=0: a = a1 + a2 + a3 and w = w1 + w2 + w3 by truncation to 8 significant bits (exact, split3), six product groups
          a1 w1, a1 w2, a2 w1, a1 w3, a2 w2, a3 w1.
  f32     conv_mfma_kernel: the float32 products themselves.

Exact classes: every product and every partial sum, in ANY order and any split into accumulators, is exactly representable, so the
float32 result equals the float64 one bit for bit, in all three arithmetics.  The quantum is the spacing of the values an accumulator
can hold; an error of one plane, scale, tap, channel, halo or image is at least one quantum.
  planes   x = 64 i + j / 16, integer 3 <= |i| <= I, j in {-1, 0, 1}: h = 64 i, l' = 128 j.  (|i| >= 3: 1 / 16, 64 + 1 / 16 and 128 - 1 / 16
           are fp16 numbers themselves, so with |i| < 3 such a value sits in h alone and l' = 0: the identity does not hold for every
           |i| <= I, and with |i| <= 1 no element would reach the l' plane at all.)  w an integer in [-3, 3], one of them 3: s = 12, WL = 0,
           WH2 = 2 w (normal).  bias, shift, resid multiples of 1 / 16.  Budget, per output element:
           S + |bias| + |shift| + |resid| < 2^20 = 2^24 quanta of 2^-4.  I is the largest value <= 7 with
           3 Kmax (64 I + 1 / 16) + 5 < 2^20 (Kmax = Cin k^2, Cin 4 transposed; 5 bounds the three addends): 7 up to Kmax = 780.  Where
           that gives I < 3 (Kmax > 1819), I = 3 and x is thinned as in `wplanes` until a receptive field holds at most 1819 non-zero
           values.
  wplanes  x in {-1, 0, 1}, non-zero only where (c + row + column) mod m = 0, m the smallest number that leaves at most 1365 non-zero
           values in a receptive field.  w = i + j 2^-12, integer |i| <= 3 (one of them 3), j in {-1, 0, 1}: WH + WL = w 2^12 exactly,
           WL = j wherever i != 0.  Budget S + |bias| + |shift| + |resid| < 2^12 = 2^24 quanta of 2^-12.  A lost h WL term is at least one
           quantum.
  wsmall   (added here: no class above has a weight whose WH2 is an fp16 subnormal.)  `planes` with w, bias, shift and resid of every
           output channel c = 1 mod 4 scaled by 2^-18: there WH = w 2^-6 (normal) and WH2 = w 2^-17 = 128 w 2^-24, an exact fp16
           SUBNORMAL; every product and sum of such a channel is the `planes` one times 2^-18, so the budget is the same.  A kernel or a
           matrix core that flushes the subnormal WH2 loses the l' plane of these channels: at least one quantum.
  lround   (added here: no class above gives l' anything to round.)  x = any normal draw, kept only at one channel of every k-th row
           and column (2nd for the transposed form), so a receptive field holds at most ONE non-zero value; w in {0, +-1, +-2}, one of
           them 2 (s = 12, WL = 0, WH2 = 2 w), bias 0.  In f16x2 the result is w (h + l' 2^-11): x rounded to nearest twice, 22 - 23
           bits, an exact float32 number, so the kernel must equal the float64 statement OF THE ROUNDED INPUT xq = h + l' 2^-11 bit for
           bit (lround_input); in bf16x3 and f32 it equals the statement of x itself.  An l' taken by truncation, or an h / l' pair
           that carries fewer bits, differs in the last place of about a tenth of the non-zero results (a float32 value needs l' rounded in one case of four).

Bound classes (every draw through cdc_compression_amd.synth: a case is a pure function of its arguments):
  normal   x ~ n, w ~ n / sqrt(Kmax), bias 0.1 n, shift 0.3 n, resid n.
  tiny     x = 1e-6 n (h is an fp16 subnormal), bias, shift and resid scaled alike.
  top      |x| log-uniform in [1, 65504] with a random sign, every 97th value exactly +-65504; no range fault may be reported.
  wide_w   w = n 2^e / sqrt(Kmax) with an integer e in [-20, 0] per OUTPUT CHANNEL (channel 0: e = 0): whole channels sit 17 - 20
           binades below the layer's largest weight, where WL and WH2 are fp16 subnormals (csrc/cdc_weights.hip: "|WH| < 2^-3 may
           round"), and the bound below is what such a channel may lose.  bias, shift and resid of a channel carry its 2^e, so that a
           small channel's result is not its bias.

Element-wise bound, first order in u = 2^-24, for ANY order of the float32 sums.  Per product a w 2^s:
  f16x2   a = h + l' 2^-11 + ra with |ra| <= 2^-22 |a| (h to 11 bits, the rest to 11 more), w 2^s = WH + WL + rw with
          |rw| <= 2^-22 |w 2^s|, and the product l' 2^-11 WL <= 2^-22 |a w 2^s| is not formed: 3 x 2^-22 = 12 u per product.  The three
          terms per product are added with at most one rounding each of a partial sum that is at most S: 3 K u S.  Below the
          fp16 normal range the planes have the absolute spacing 2^-24: l' loses up to 2^-25 x 2^-11 = 2^-36 per activation, times
          |w| summed: 2^-36 W1; WL and WH2 lose up to 2^-25 each per weight, times |h| resp. |l'| <= |a|, summed and scaled back:
          2^-24 2^-s X1.
              E = (12 u + 3 K u) S + 2^-36 W1 + 2^-24 2^-s X1
  f32     each product rounded once (u S in all), K - 1 additions: E = (K + 1) u S.
  bf16x3  the planes come from TRUNCATION to 8 significant bits, so |a2| < 2^-7 |a| and |a3| < 2^-15 |a| (not 2^-8 and 2^-16, the
          figures of a rounded split); the products not formed, a2 w3 + a3 w2 + a3 w3, are below (2 x 2^-22 + 2^-30) |a w| < 8.04 u |a w|.
          (A rounded split would give 3 u; the figure is this line's reasoning, not a measurement.)  Six additions per
          product:   E = (8.04 u + 6 K u) S.
  every epilogue addition (bias, shift, resid) adds u |its result|;   bound = 1.05 E + 2^-149 (1.05: the second-order terms).
  LayerNorm behind an EXACT class: the convolution result is exact, so ln_ref.ln_bound holds unchanged with it as the single slice.

Sharp measure.  r = rms over the tensor of err / S.  Its limit is 2 x the same figure of the SERIAL-order float32 restatement of the
same case in the same arithmetic (emulate, order "serial"), computed here on the CPU over a seeded sample of output elements, never from
a kernel: the serial chain is the worst plain order and every kernel sums in blocks (the 16-deep blocked restatement sits 3 - 4 x
below it); 2 leaves conv_mfma_kernel's nearly serial 2-deep steps room for sampling noise.

The wrong kernels of the host test (emulate's `mutant`) and the check that catches each:
  lp_zero_chunk   l' zero in one tap of one 16-channel chunk        planes (Cin = 384): not bit-equal
  acc2_unscaled   l' WH instead of l' WH2 in one 32-channel block   planes: not bit-equal
  drop_hWL        the h WL term missing                             wplanes: not bit-equal
  lp_trunc        l' by truncation                                  lround: not bit-equal (its rms on `normal` stays inside the limit:
                                                                    the float32 sums hide a one-bit loss of l')
  wh2_flush       WH2 = 0 below 2^-14                               wsmall: not bit-equal; wide_w: 34 x its rms limit (0.4 - 0.5 of the element-wise
                                                                    bound: the lost terms have random signs, the bound adds magnitudes; on
                                                                    `normal` no weight is that small)
  ftz             fp16 subnormals of h and l' flushed               tiny: outside the element-wise bound and the rms limit"""
import numpy as np
import torch
import torch.nn.functional as F

import ln_ref
from cdc_compression_amd import synth

U = 2.0 ** -24
TINY = 2.0 ** -149
EXACT_CLASSES = ("planes", "wplanes", "wsmall", "lround")
BOUND_CLASSES = ("normal", "tiny", "top", "wide_w")
ARITHS = ("f16x2", "bf16x3", "f32")
MUTANTS = ("lp_zero_chunk", "acc2_unscaled", "drop_hWL", "lp_trunc", "wh2_flush", "ftz")

# ---- the forms of tests/test_gpu_conv_edges.py: (family, switches, shape, epilogues) ------------------------------------------------
# shape: (B, Cin, H, W, Cout, k, stride, pad) or, transposed, (B, Cin, H, W, Cout).  epilogues: "bias", "sr" (bias + shift + resid),
# "r" (bias + resid), "ln" (bias, LayerNorm + ReLU + shift + resid).  Every shape and switch set is one tests/test_gpu_parity.py runs.
_PF1 = {"CDC_PF": "1", "CDC_PF_MAXPIX": "0"}
_PF = {**_PF1, "CDC_WS_MIN_WGS": "1000000000", "CDC_PF_MIN_WAVES": "1", "CDC_OP_REQUIRE_PF": "1"}   # as tests/test_gpu_determinism.py runs conv_pf_kernel
_WS = {"CDC_WS_MIN_WGS": "1", "CDC_OP_REQUIRE_WS": "1"}
_PW = {"CDC_PW_MIN_WAVES": "1"}
ARITH_OF = {"mfma": "f32", "split": "bf16x3", "split2": "bf16x3", "split2h": "f16x2", "pf": "f16x2", "pf s2": "f16x2", "pf tz4": "f16x2", "pf3": "f16x2",
            "pw": "f16x2", "ws": "f16x2", "ws1": "f16x2"}


def _both(fam):
    return {"bias": fam, "sr": fam}


def _ws1(npb):
    return {"CDC_WS1_MIN_WGS": "1", "CDC_WS1_NPB": npb}


# (switches, shape, {epilogue: family that runs it on an MI355X}); a row is named after its first family.  Where the family differs from
# the one the shape was listed for, the comment says so: the row stays, under the family it runs.
FORMS = (
    ({}, (2, 5, 9, 11, 7, 3, 1, 1), _both("mfma")),
    ({}, (1, 3, 10, 9, 4, 7, 1, 3), _both("mfma")),
    ({}, (2, 6, 5, 5, 9, 1, 1, 0), _both("mfma")),
    # listed for conv_split2 with the fused LayerNorm: bias-only and LayerNorm calls are on conv_ws_kernel (+ the LayerNorm pass), only the
    # call with a shift and a residual is on conv_split2
    ({}, (2, 64, 32, 32, 64, 3, 1, 1), {"sr": "split2h", "bias": "ws", "ln": "ws"}),
    ({"CDC_ARITH": "0"}, (2, 64, 32, 32, 64, 3, 1, 1), {"bias": "split2", "sr": "split2", "ln": "split2"}),      # bf16x3, LayerNorm fused
    # stride 2 down to 8 x 8: with a residual alone split-K (ks4) + the sum pass; bias-only is on conv_ws_kernel's stride-2 form, shift + residual on
    # conv_split_kernel (three bf16 planes, also in F16X2)
    ({}, (2, 320, 16, 16, 320, 3, 2, 1), {"r": "split2h", "bias": "ws", "sr": "split"}),
    ({}, (1, 24, 24, 40, 24, 3, 1, 1), {"bias": "split2h", "sr": "split2h", "ln": "split2h"}),     # Cout % 32 != 0: the LayerNorm is a pass of its own
    # conv_pf_kernel, stride 1: the three shapes listed run other kernels under CDC_PF=1 CDC_PF_MAXPIX=0 (CDC_OP_REQUIRE_PF refuses them) ...
    (_PF1, (1, 16, 32, 32, 32, 3, 1, 1), _both("split2h")),
    (_PF1, (1, 64, 33, 48, 64, 3, 1, 1), {"bias": "split2h", "sr": "split2h", "ln": "split2h"}),   # ragged in both directions, LayerNorm fused
    (_PF1, (2, 384, 32, 32, 128, 1, 1, 0), _both("ws1")),
    # ... and the nearest shapes that do run it, with the switches of tests/test_gpu_determinism.py
    (_PF, (2, 384, 32, 32, 128, 1, 1, 0), _both("pf")),
    (_PF, (1, 192, 36, 32, 192, 3, 1, 1), {"bias": "pf", "sr": "pf", "ln": "pf"}),                 # eight waves, ragged rows, LayerNorm fused
    ({**_PF1, "CDC_PF_S2_MIN_WGS": "1", "CDC_OP_REQUIRE_PF": "1"}, (1, 32, 64, 64, 192, 3, 2, 1), _both("pf s2")),
    ({**_PF1, "CDC_PF_TZ_MIN_WGS": "1", "CDC_OP_REQUIRE_PF": "1"}, (1, 32, 8, 32, 64), {"bias": "pf tz4"}),
    ({**_PF1, "CDC_PF_TZ_MIN_WGS": "1", "CDC_OP_REQUIRE_PF": "1"}, (1, 64, 16, 48, 64), {"bias": "pf tz4"}),
    (_PF1, (4, 64, 128, 256, 64, 3, 1, 1), {"bias": "pf3", "sr": "pf3", "ln": "pf3"}),             # (at B = 2 and 1 the planner stays on conv_pf_kernel)
    # conv_pw_kernel: the two shapes listed are few-pixel launches, which conv_ws1_kernel takes; (2, 64, 36, 64, 64) is the one shape of
    # tests/test_gpu_parity.py: PW_CASES that runs conv_pw_kernel
    (_PW, (1, 48, 12, 16, 64, 1, 1, 0), _both("ws1")),
    (_PW, (3, 320, 16, 16, 128, 1, 1, 0), _both("ws1")),
    (_PW, (2, 64, 36, 64, 64, 1, 1, 0), _both("pw")),
    ({**_WS, "CDC_WS_NPB": "2"}, (2, 48, 8, 8, 32, 3, 1, 1), {"bias": "ws", "ln": "ws"}),
    ({**_WS, "CDC_WS_NPB": "4"}, (2, 48, 8, 8, 32, 3, 1, 1), {"bias": "ws", "ln": "ws"}),
    ({**_WS, "CDC_WS_NPB": "2"}, (1, 64, 32, 32, 96, 3, 1, 1), {"bias": "ws", "ln": "ws"}),
    ({**_WS, "CDC_WS_NPB": "4"}, (1, 64, 32, 32, 96, 3, 1, 1), {"bias": "ws", "ln": "ws"}),
    (_WS, (1, 64, 64, 64, 64, 3, 2, 1), {"bias": "ws"}),        # stride 2: 64-pixel tiles only (CDC_WS_NPB=4 is refused), as the suite runs it
    (_ws1("2"), (2, 48, 8, 8, 32, 1, 1, 0), _both("ws1")),
    (_ws1("4"), (2, 48, 8, 8, 32, 1, 1, 0), _both("ws1")),
    # listed for conv_ws1_kernel: 96 pixels do not divide into its tiles, the call is on conv_split2; (1, 128, 16, 64, 128) is the nearest of WS1_CASES
    (_ws1("2"), (1, 64, 4, 24, 96, 1, 1, 0), _both("split2h")),
    (_ws1("4"), (1, 64, 4, 24, 96, 1, 1, 0), _both("split2h")),
    (_ws1("2"), (1, 128, 16, 64, 128, 1, 1, 0), _both("ws1")),
    (_ws1("4"), (1, 128, 16, 64, 128, 1, 1, 0), _both("ws1")),
    ({}, (2, 5, 6, 7, 4), {"bias": "mfma"}),                    # generic transposed
    ({}, (1, 64, 16, 16, 64), {"bias": "split2h"}),
)
PF3_CLASSES = ("planes", "normal")          # the large form: its float64 references take the longest


def form_id(form):
    env, shape, eps = form
    npb = env.get("CDC_WS_NPB") or env.get("CDC_WS1_NPB")
    tag = "pfenv-" if env.get("CDC_PF") and next(iter(eps.values())) not in ("pf", "pf s2", "pf tz4", "pf3") else ("pwenv-" if env.get("CDC_PW_MIN_WAVES") else "")
    return f"{tag}{next(iter(eps.values())).replace(' ', '_')}{'-npb' + npb if npb else ''}{'-bf16x3' if env.get('CDC_ARITH') == '0' else ''}-{shape_id(shape)}"


def family_of(label):
    """The kernel family of a convolution's line of the per-op table (csrc/cdc_state.h: op_label); None: not a convolution."""
    if not label.startswith("conv "):
        return None
    words = label.split()
    for tag, name in (("WS1", "ws1"), ("WS", "ws"), ("PF3", "pf3"), ("PW", "pw"), ("SPLIT2H", "split2h"), ("SPLIT2", "split2"), ("SPLIT", "split")):
        if tag in words:
            return name
    if "PF" in words:
        return "pf tz4" if "TZ4" in words else ("pf s2" if words[2] == "s2" else "pf")
    return "mfma"


def shape_id(shape):
    return ("T" if len(shape) == 5 else "") + "x".join(map(str, shape))


def geometry(shape):
    """-> (B, Cin, H, W, Cout, k, stride, pad, transposed, Ho, Wo, Kmax, window): window = side of the receptive field in the input."""
    if len(shape) == 5:
        B, Ci, H, W, Co = shape
        return B, Ci, H, W, Co, 4, 2, 1, True, 2 * H, 2 * W, Ci * 4, 2
    B, Ci, H, W, Co, k, s, p = shape
    return B, Ci, H, W, Co, k, s, p, False, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Ci * k * k, k


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _ints(name, shape, seed, lo, hi):
    """Integers uniform in [lo, hi], float64."""
    return np.floor(synth.uniform(name, shape, seed, float(lo), float(hi) + 1.0))


def planes_I(Kmax):
    """Largest |i| of class `planes` (at least 3; thin_m then keeps the budget)."""
    for I in range(7, 2, -1):
        if 3 * Kmax * (64 * I + 1.0 / 16) + 5 < 2.0 ** 20:
            return I
    return 3


def thin_m(Cin, window, most):
    """Smallest m for which the mask (c + row + column) mod m = 0 leaves at most `most` values in a receptive field."""
    m = 1
    while Cin * window * -(-window // m) > most:
        m += 1
    return m


def _thin_mask(shape4, m):
    B, Ci, H, W = shape4
    c, r, q = np.arange(Ci)[None, :, None, None], np.arange(H)[None, None, :, None], np.arange(W)[None, None, None, :]
    return (c + r + q) % m == 0


def make_case(cls, shape, seed=0):
    """{"x", "w", "bias" [Cout], "shift" [B, Cout], "resid" [B, Cout, Ho, Wo], "g", "b" [Cout] (the LayerNorm's)} of class `cls`,
    float32; w is [Cout, Cin, k, k], or [Cin, Cout, 4, 4] for the transposed form."""
    B, Ci, H, W, Co, k, s, p, T, Ho, Wo, Kmax, win = geometry(shape)
    xs, ws, rs = (B, Ci, H, W), ((Ci, Co, 4, 4) if T else (Co, Ci, k, k)), (B, Co, Ho, Wo)
    tag = f"conv_edge_{cls}"
    nx = lambda: synth.normal(tag + "_x", xs, seed).astype(np.float64)
    nw = lambda: synth.normal(tag + "_w", ws, seed).astype(np.float64) / np.sqrt(Kmax)
    scale = 1.0
    if cls in ("planes", "wsmall"):
        tag = "conv_edge_planes"
        I = planes_I(Kmax)
        sign = np.where(synth.uniform(tag + "_s", xs, seed) < 0.5, -1.0, 1.0)
        x = (sign * 64.0 * _ints(tag + "_i", xs, seed, 3, I) + _ints(tag + "_j", xs, seed, -1, 1) / 16.0) * _thin_mask(xs, thin_m(Ci, win, 1819))
        w = _ints(tag + "_w", ws, seed, -3, 3)
        w.reshape(-1)[0] = 3.0
    elif cls == "wplanes":
        x = _ints(tag + "_x", xs, seed, -1, 1) * _thin_mask(xs, thin_m(Ci, win, 1365))
        w = _ints(tag + "_i", ws, seed, -3, 3) + _ints(tag + "_j", ws, seed, -1, 1) * 2.0 ** -12
        w.reshape(-1)[0] = 3.0
    elif cls == "lround":
        r, q = np.arange(H)[:, None], np.arange(W)[None, :]
        chan = (r // win + 5 * (q // win)) % Ci                                   # the one channel of a kept pixel
        keep = ((r % win == 0) & (q % win == 0))[None, None] & (np.arange(Ci)[None, :, None, None] == chan[None, None])
        x = np.where(keep, nx() + np.sign(nx()) * 0.25, 0.0)
        w = _ints(tag + "_w", ws, seed, -2, 2)
        w.reshape(-1)[0] = 2.0
    elif cls == "normal":
        x, w = nx(), nw()
    elif cls == "tiny":
        x, w, scale = 1e-6 * nx(), nw(), 1e-6
    elif cls == "top":
        mag = np.exp(synth.uniform(tag + "_m", xs, seed, 0.0, float(np.log(65504.0))))
        x = np.minimum(mag, 65504.0) * np.where(synth.uniform(tag + "_s", xs, seed) < 0.5, -1.0, 1.0)
        flat = x.reshape(-1)
        flat[::97] = np.where(flat[::97] < 0, -65504.0, 65504.0)
        w = nw()
    elif cls == "wide_w":
        e = _ints(tag + "_e", (Co,), seed, -20, 0)
        e[0] = 0.0
        x, w, scale = nx(), nw() * (2.0 ** e).reshape((1, Co, 1, 1) if T else (Co, 1, 1, 1)), 2.0 ** e
    else:
        raise ValueError(cls)
    if cls in ("planes", "wplanes", "wsmall"):
        bias, shift, resid = (_ints(tag + "_b", (Co,), seed, -32, 32) / 16.0, _ints(tag + "_sh", (B, Co), seed, -16, 16) / 16.0,
                              _ints(tag + "_r", rs, seed, -16, 16) / 16.0)
        if cls == "wsmall":
            sc = np.where(np.arange(Co) % 4 == 1, 2.0 ** -18, 1.0)
            w = w * sc.reshape((1, Co, 1, 1) if T else (Co, 1, 1, 1))
            bias, shift, resid = bias * sc, shift * sc[None, :], resid * sc[None, :, None, None]
    elif cls == "lround":
        bias, shift, resid = np.zeros(Co), np.zeros((B, Co)), np.zeros(rs)
    else:
        scale = np.broadcast_to(scale, (Co,))                    # (per output channel in `wide_w`)
        bias, shift, resid = (scale * synth.normal(tag + "_b", (Co,), seed, 0.1), scale[None, :] * synth.normal(tag + "_sh", (B, Co), seed, 0.3),
                              scale[None, :, None, None] * synth.normal(tag + "_r", rs, seed))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    case = {"x": f32(x), "w": f32(w), "bias": f32(bias), "shift": f32(shift), "resid": f32(resid),
            "g": synth.normal(tag + "_g", (Co,), seed, 0.2, 1.0), "b": synth.normal(tag + "_bb", (Co,), seed, 0.2)}
    for v in case.values():
        v.setflags(write=False)
    return case


# ---- the arithmetics' operands ------------------------------------------------------------------------------------------------------
def weight_scale(w):
    """s of csrc/cdc_weights.hip: 14 - e with max |w| = m 2^e, m in [0.5, 1), over the whole tensor, clamped to +-100."""
    wmax = float(np.abs(np.asarray(w, np.float32)).max())
    s = 14 - int(np.frexp(np.float32(wmax))[1]) if wmax > 0 and np.isfinite(wmax) else 0
    return max(-100, min(100, s))


def _fp16_toward_zero(v):
    r = np.asarray(v, np.float32).astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def act_planes(a, truncate_l=False):
    """(h, l') float16 of float32 activations (split2h)."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    v = (a - h.astype(np.float32)) * np.float32(2048)
    return h, (_fp16_toward_zero(v) if truncate_l else v.astype(np.float16))


def weight_planes(w, s):
    """(WH, WL, WH2) float16 of float32 weights at the scale 2^s."""
    v = np.asarray(w, np.float32) * np.float32(2.0 ** s)
    WH = v.astype(np.float16)
    WL = (v - WH.astype(np.float32)).astype(np.float16)
    WH2 = (WH.astype(np.float32) * np.float32(1.0 / 2048.0)).astype(np.float16)
    return WH, WL, WH2


def split3(a):
    """(a1, a2, a3) float32 with a == a1 + a2 + a3 exactly, each of at most 8 significant bits (truncation)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    mask = np.uint32(0xFFFF0000)
    a1 = (a.view(np.uint32) & mask).view(np.float32)
    r = a - a1
    a2 = (r.view(np.uint32) & mask).view(np.float32)
    return a1, a2, r - a2


def lround_input(x):
    """xq = h + l' 2^-11, float64: what the two planes of f16x2 carry of x."""
    h, l = act_planes(x)
    return h.astype(np.float64) + l.astype(np.float64) * 2.0 ** -11


def _flush16(p):
    return np.where(np.abs(p.astype(np.float32)) < np.float32(2.0 ** -14), np.float16(0), p)


# ---- float64 statement --------------------------------------------------------------------------------------------------------------
def _conv(x, w, shape):
    B, Ci, H, W, Co, k, s, p, T = geometry(shape)[:9]
    x, w = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    return (F.conv_transpose2d(x, w, stride=2, padding=1) if T else F.conv2d(x, w, stride=s, padding=p)).numpy()


def conv_f64(case, shape, x=None):
    """{"conv" (no bias), "S", "X1", "W1", "K"}: float64, each broadcastable to [B, Cout, Ho, Wo].  x: another input than the case's
    (lround_input)."""
    x = case["x"] if x is None else x
    w = case["w"]
    one_w = np.ones((w.shape[0], 1) + w.shape[2:]) if len(shape) == 5 else np.ones((1,) + w.shape[1:])
    one_x = np.ones((1,) + x.shape[1:])
    out = {"conv": _conv(x, w, shape), "S": _conv(np.abs(x), np.abs(w), shape), "X1": _conv(np.abs(x), one_w, shape),
           "W1": _conv(one_x, np.abs(w), shape), "K": _conv(one_x, one_w, shape)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _ln_view(a):
    return np.asarray(a).reshape(a.shape[0], a.shape[1], 1, -1)


def statement(ref, case, ep):
    """y (float64) of the epilogue `ep` over the reference `ref` of conv_f64."""
    B, Co = case["shift"].shape
    v = ref["conv"] + case["bias"].astype(np.float64).reshape(1, Co, 1, 1)
    if ep == "bias":
        return v
    if ep == "sr":
        return v + case["shift"].astype(np.float64).reshape(B, Co, 1, 1) + case["resid"]
    if ep == "r":
        return v + case["resid"]
    if ep == "ln":
        return ln_ref.ln_f64(_ln_view(v)[None], case["g"], case["b"], True, case["shift"], _ln_view(case["resid"]))["y"].reshape(v.shape)
    raise ValueError(ep)


def representation_terms(arith, K):
    """(per-product relative part, additions per product) of E."""
    return {"f16x2": (12.0, 3.0), "bf16x3": (8.04, 6.0), "f32": (1.0, 1.0)}[arith]


def bound(ref, case, ep, arith):
    """The element-wise bound of the module docstring for `statement(ref, case, ep)`; ep "ln" is for the exact classes only."""
    B, Co = case["shift"].shape
    v = ref["conv"] + case["bias"].astype(np.float64).reshape(1, Co, 1, 1)
    if ep == "ln":
        return ln_ref.ln_bound(_ln_view(v)[None], case["g"], case["b"], True, case["shift"], _ln_view(case["resid"]))["y"].reshape(v.shape)
    rep, adds = representation_terms(arith, ref["K"])
    E = (rep + adds * ref["K"]) * U * ref["S"]
    if arith == "f16x2":
        E = E + 2.0 ** -36 * ref["W1"] + 2.0 ** -24 * 2.0 ** -weight_scale(case["w"]) * ref["X1"]
    E = E + U * np.abs(v)
    if ep == "sr":
        v = v + case["shift"].astype(np.float64).reshape(B, Co, 1, 1)
        E = E + U * np.abs(v)
    if ep in ("sr", "r"):
        v = v + case["resid"]
        E = E + U * np.abs(v)
    return 1.05 * E + TINY


def budget(ref, case):
    """Largest S + |bias| + |shift| + |resid| over the output (the exact classes' budgets: < 2^20 planes, < 2^12 wplanes)."""
    B, Co = case["shift"].shape
    return float((ref["S"] + np.abs(case["bias"]).reshape(1, Co, 1, 1) + np.abs(case["shift"]).reshape(B, Co, 1, 1)
                  + np.abs(case["resid"])).max())


# ---- rows: sampled output elements as dot products ----------------------------------------------------------------------------------
def sample_rows(case, shape, n=1024, seed=0, every=None):
    """n output elements (seeded; `every`: all of them when the output has at most that many) as rows of a dot product:
    {"a", "w" [n, taps Cin] float32 (k = tap Cin + channel; out-of-bounds products are zeros), "bias", "shift", "resid" [n], "idx"}."""
    B, Ci, H, W, Co, k, s, p, T, Ho, Wo, Kmax, win = geometry(shape)
    total = B * Co * Ho * Wo
    if every is not None and total <= every:
        flat = np.arange(total)
    else:
        flat = np.floor(synth.uniform("conv_edge_rows", (n,), seed) * total).astype(np.int64)
    b, co, oy, ox = np.unravel_index(flat, (B, Co, Ho, Wo))
    x, w = case["x"], case["w"]
    a = np.zeros((len(flat), k * k, Ci), np.float32)
    wr = np.zeros((len(flat), k * k, Ci), np.float32)
    for ky in range(k):
        for kx in range(k):
            if T:                                       # oy = 2 iy - 1 + ky
                ny, nx_ = oy + 1 - ky, ox + 1 - kx
                ok = (ny % 2 == 0) & (nx_ % 2 == 0)
                iy, ix = ny // 2, nx_ // 2
                wt = w[:, co, ky, kx].T
            else:
                iy, ix = oy * s - p + ky, ox * s - p + kx
                ok = np.ones(len(flat), bool)
                wt = w[co, :, ky, kx]
            ok = ok & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            t = ky * k + kx
            a[ok, t] = x[b[ok], :, iy[ok], ix[ok]]
            wr[ok, t] = wt[ok]
    return {"a": a.reshape(len(flat), -1), "w": wr.reshape(len(flat), -1), "bias": case["bias"][co], "shift": case["shift"][b, co],
            "resid": case["resid"][b, co, oy, ox], "idx": (b, co, oy, ox), "Cin": Ci}


def rows_f64(rows, ep="bias", a=None):
    """(y, S) float64 of the rows' statement."""
    a = rows["a"] if a is None else a
    y = (a.astype(np.float64) * rows["w"].astype(np.float64)).sum(1) + rows["bias"]
    if ep == "sr":
        y = y + rows["shift"].astype(np.float64)
    if ep in ("sr", "r"):
        y = y + rows["resid"]
    return y, (np.abs(a).astype(np.float64) * np.abs(rows["w"]).astype(np.float64)).sum(1)


def rows_bound(rows, ep, arith, s):
    a64, w64 = np.abs(rows["a"]).astype(np.float64), np.abs(rows["w"]).astype(np.float64)
    live = (rows["a"] != 0) | (rows["w"] != 0)
    ref = {"conv": (rows["a"].astype(np.float64) * rows["w"].astype(np.float64)).sum(1), "S": (a64 * w64).sum(1), "X1": a64.sum(1),
           "W1": w64.sum(1), "K": live.sum(1).astype(np.float64)}
    rep, adds = representation_terms(arith, ref["K"])
    E = (rep + adds * ref["K"]) * U * ref["S"]
    if arith == "f16x2":
        E = E + 2.0 ** -36 * ref["W1"] + 2.0 ** -24 * 2.0 ** -s * ref["X1"]
    v = ref["conv"] + rows["bias"]
    E = E + U * np.abs(v)
    if ep == "sr":
        v = v + rows["shift"]
        E = E + U * np.abs(v)
    if ep in ("sr", "r"):
        v = v + rows["resid"]
        E = E + U * np.abs(v)
    return 1.05 * E + TINY


# ---- float32 restatements -----------------------------------------------------------------------------------------------------------
def _terms(rows, arith, s, mutant=None):
    """[n, K, P] float64: the P exact products per k, in the order an accumulator receives them."""
    a, w = rows["a"], rows["w"]
    if arith == "f32":
        return (a.astype(np.float64) * w.astype(np.float64))[..., None]
    if arith == "bf16x3":
        a1, a2, a3 = (t.astype(np.float64) for t in split3(a))
        w1, w2, w3 = (t.astype(np.float64) for t in split3(w))
        return np.stack([a1 * w1, a1 * w2, a2 * w1, a1 * w3, a2 * w2, a3 * w1], -1)
    h, l = act_planes(a, truncate_l=mutant == "lp_trunc")
    WH, WL, WH2 = weight_planes(w, s)
    Ci = rows["Cin"]
    if mutant == "ftz":
        h, l = _flush16(h), _flush16(l)
    if mutant == "wh2_flush":
        WH2 = _flush16(WH2)
    h, l, WH, WL, WH2 = (t.astype(np.float64) for t in (h, l, WH, WL, WH2))
    if mutant == "lp_zero_chunk":                       # tap 1 (or the only one), channels 16 ... 31
        k0 = (Ci if a.shape[1] > Ci else 0) + 16
        l[:, k0:k0 + 16] = 0.0
    t3 = l * WH2
    if mutant == "acc2_unscaled":                       # tap 0, channels 32 ... 63
        t3[:, 32:64] = (l * WH)[:, 32:64]
    t2 = np.zeros_like(t3) if mutant == "drop_hWL" else h * WL
    return np.stack([h * WH, t2, t3], -1)


def emulate(rows, arith, order="serial", ep="bias", mutant=None, block=16):
    """Float32 restatement of the rows in the arithmetic `arith`: products exact, every accumulation rounded to float32.
    order "serial": one product after the other; "blocks": `block`-deep sums (exact inside, as a matrix instruction adds them) added
    to one accumulator per plane in turn; "split8": the blocks dealt to 8 accumulators, which are added at the end.  Then 2^-s, + bias,
    (+ shift, + resid).  mutant: one of MUTANTS (f16x2 only)."""
    s = weight_scale_of(rows) if arith == "f16x2" else 0
    T = _terms(rows, arith, s, mutant)
    n, K, P = T.shape
    f32 = np.float32
    if order == "serial":
        acc = np.zeros(n, f32)
        flat = T.reshape(n, K * P)
        for i in range(K * P):
            acc = (acc.astype(np.float64) + flat[:, i]).astype(f32)
    else:
        nacc = 8 if order == "split8" else 1
        accs = [np.zeros(n, f32) for _ in range(nacc)]
        for bi, k0 in enumerate(range(0, K, block)):
            for pl in range(P):
                j = bi % nacc
                accs[j] = (accs[j].astype(np.float64) + T[:, k0:k0 + block, pl].sum(1)).astype(f32)
        acc = accs[0]
        for j in range(1, nacc):
            acc = acc + accs[j]
    y = acc * f32(2.0 ** -s) + rows["bias"]
    if ep == "sr":
        y = y + rows["shift"]
    if ep in ("sr", "r"):
        y = y + rows["resid"]
    return y.astype(f32)


def weight_scale_of(rows):
    return rows.get("s", weight_scale(rows["w"]))


def with_scale(rows, case):
    """The rows with the weight scale of the WHOLE tensor (a sample need not hold the largest weight)."""
    out = dict(rows)
    out["s"] = weight_scale(case["w"])
    return out


def rms_ratio(got, want, S):
    """rms of err / S over the elements with S > 0."""
    live = S > 0
    e = (np.asarray(got, np.float64) - want)[live] / S[live]
    return float(np.sqrt(np.mean(e * e))) if e.size else 0.0


def serial_figure(case, shape, arith, ep="bias", n=1024):
    """rms of err / S of the serial-order restatement over n sampled output elements: half of the kernels' limit."""
    rows = with_scale(sample_rows(case, shape, n), case)
    want, S = rows_f64(rows, ep)
    return rms_ratio(emulate(rows, arith, "serial", ep), want, S)


# ---- measures -----------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def worst(got, want, bnd, S=None):
    """(largest |got - want| / bnd, its index, a line that names the worst element: error, bound, S, binade)."""
    got = np.asarray(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(np.float64) - want)
        r = err / bnd
    r = np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    line = f"worst element {tuple(int(v) for v in i)}: got {got[i]!r} want {want[i]:.9g} error {err[i]:.3g} bound {np.broadcast_to(bnd, r.shape)[i]:.3g}"
    if S is not None:
        line += f" S {np.broadcast_to(S, r.shape)[i]:.3g}"
    line += f" binade 2^{int(np.floor(np.log2(abs(want[i])))) if want[i] != 0 else 0}"
    return float(r.max()), i, line
