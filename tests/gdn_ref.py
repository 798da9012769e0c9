"""Input classes, expectations and measures of the GDN1 edge tests, shared by tests/test_gdn_ref_host.py (no GPU: the preconditions)
and tests/test_gpu_gdn_edges.py (the kernel).  The float64 evaluation is simple_ref.gdn1_np over the float32-reparametrised parameters.

Tolerance (as tests/test_gpu_simple.py): element-wise relative error <= (C + 2) 2^-24.  Derived, not measured: the C + 1 terms of the
norm are non-negative (no cancellation), each accumulation rounds once (relative 2^-24 of a partial sum that is at most the norm), and
the quotient / product rounds once more.  Wherever float64 gives exactly 0 the kernel must too, with the same sign.

Classes (every draw through cdc_compression_amd.synth, so a case is a pure function of its arguments):
  normal  synth.gdn_input / synth.gdn_layer_params: gamma = sqrt(0.1) I + N(0, 0.05^2), gamma' 0.1 on the diagonal, ~0.0025 or 0 off it.
  dense   gamma ~ U(0, 0.3), not symmetric, no zero in gamma'; beta = 1 + N(0, 0.1^2), beta[0] = 0 (the clamp acts).
  wide    dense parameters, x = +-10^U(-15, 15): thirty decades inside one sum.
  perm    raw gamma zero except gamma[i][(3 i + 5) mod C] = 1, so gamma' is exactly that 0/1 matrix: output i reads exactly one other
          channel, and a wrong row, column or k-slice index is an O(1) error at every element.  The map has no fixed point (2 i = -5
          has no solution modulo an even C) and is not its own inverse; it is a permutation where 3 does not divide C, and three-to-one
          onto a third of the channels where it does (C = 48, 96, 144, 192, 240) -- the closed form below holds either way.
  below   every raw gamma <= 2^-18, negative entries and the bound itself included: gamma' = 0 and the norm is beta' exactly."""
import numpy as np

from cdc_compression_amd import synth
from simple_ref import gdn1_np, gdn_reparam_np

CLASSES = ("normal", "dense", "wide", "perm", "below")
TOLERANCE_CLASSES = ("normal", "dense", "wide", "perm", "below")     # every class is held to the float64 bound
TILE = 64                                                            # pixels of a gdn_kernel tile


WIDTHS = tuple(range(16, 257, 16))                                   # the sixteen instantiations of gdn_kernel
PIXEL_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)            # around an MFMA column block (16), a tile (64) and two tiles
WALK_SHAPES = ((3, 16, 64 * 7 + 9), (1, 256, 64 * 3 + 1))           # (B, C, HW): 8 tiles (trips 3/3/2 at 3 workgroups); 4 tiles, 1024 threads
HOSTILE_SHAPE = (2, 48, 70)                                          # (B, C, HW) of the non-finite and overflow cases: a whole tile and a tail of 6


def tolerance_cases(cus=256):
    """(cls, B, C, HW) of every case that tests/test_gpu_gdn_edges.py holds to the float64 bound."""
    cases = [(cls, 2, C, 70) for C in WIDTHS for cls in ("dense", "perm")]
    cases += [(cls, 2, C, 70) for C in (16, 48, 256) for cls in ("wide", "below")]
    cases += [("normal", 2, C, HW) for C in (48, 256) for HW in PIXEL_EDGES]
    cases += [(cls, B, C, HW) for B, C, HW in WALK_SHAPES for cls in ("dense", "perm")]
    cases += [("dense", -(-4 * cus // 3), 16, 64 * 7 + 9), ("normal",) + HOSTILE_SHAPE, ("dense",) + HOSTILE_SHAPE]
    return cases


def bound(C):
    return (C + 2) * 2.0 ** -24


def perm_of(C):
    return (3 * np.arange(C) + 5) % C


def gdn_params(cls, C, seed=0):
    """(beta [C], gamma [C, C]), raw float32 parameters of class `cls`."""
    if cls == "normal":
        return synth.gdn_layer_params(C, seed=seed)
    beta = synth.normal(f"gdn_edge_beta_{cls}", (C,), seed, 0.1, 1.0)
    beta[0] = 0.0
    if cls in ("dense", "wide"):
        gamma = synth.uniform("gdn_edge_gamma_dense", (C, C), seed, 0.0, 0.3).astype(np.float32)
    elif cls == "perm":
        gamma = np.zeros((C, C), np.float32)
        gamma[np.arange(C), perm_of(C)] = 1.0
    elif cls == "below":
        gamma = np.minimum(synth.normal("gdn_edge_gamma_below", (C, C), seed, 0.05), np.float32(2.0 ** -18))
        gamma.reshape(-1)[0::5] = np.float32(2.0 ** -19)             # ... and positive entries under the bound
    else:
        raise ValueError(cls)
    return beta, gamma


def gdn_x(cls, B, C, HW, seed=0):
    """x [B, C, 1, HW] float32 of class `cls`."""
    shape = (B, C, 1, HW)
    if cls == "wide":
        mag = 10.0 ** synth.uniform("gdn_edge_x_wide_mag", shape, seed, -15.0, 15.0)
        sign = np.where(synth.uniform("gdn_edge_x_wide_sign", shape, seed) < 0.5, -1.0, 1.0)
        return (sign * mag).astype(np.float32)
    if cls == "normal":
        return synth.gdn_input(shape, seed=seed)
    x = synth.gdn_input(shape, seed=seed, name=f"gdn_edge_x_{cls}")
    if x.size > 1:
        x.reshape(-1)[1] = -0.0                                       # a negative zero beside gdn_input's positive ones
    return x


def gdn_edge_case(cls, B, C, HW, seed=0):
    """(x, beta, gamma) of one case."""
    beta, gamma = gdn_params(cls, C, seed)
    return gdn_x(cls, B, C, HW, seed), beta, gamma


def with_nonfinite(x):
    """(x with +inf at [0, 5, 3] and NaN at [1, 7, 66] (the tail tile of HW = 70), mask [B, 1, 1, HW] of the two hostile pixels)."""
    x = x.copy()
    x[0, 5, 0, 3] = np.inf
    x[1, 7, 0, 66] = np.nan
    m = np.zeros((x.shape[0], 1, 1, x.shape[3]), bool)
    m[0, 0, 0, 3] = m[1, 0, 0, 66] = True
    return x, np.broadcast_to(m, x.shape)


def with_overflow(x):
    """(x with a finite 1e30 at [0, 5, 3]: the inverse of that pixel leaves float32, mask of the pixel)."""
    x = x.copy()
    x[0, 5, 0, 3] = 1e30
    m = np.zeros((x.shape[0], 1, 1, x.shape[3]), bool)
    m[0, 0, 0, 3] = True
    return x, np.broadcast_to(m, x.shape)


def gdn_f64(x, beta, gamma, inverse):
    """The float64 evaluation of the float32-reparametrised parameters (non-finite inputs pass through as IEEE has them)."""
    with np.errstate(all="ignore"):
        return gdn1_np(x, *gdn_reparam_np(beta, gamma), inverse)


def gdn_f32_chain(x, beta, gamma, inverse):
    """float32 restatement: beta' + sum_j gamma'[i][j] |x_j| accumulated in j order, one rounding per accumulation (a fused
    multiply-add: the product of two float32 is exact in float64; the sum is rounded to 53 bits and then to 24, a double rounding
    that differs from the single one in a vanishing share of the cases and by one ulp of one step), then the rounded quotient / product."""
    br, gr = gdn_reparam_np(beta, gamma)
    B, C = x.shape[:2]
    ax = np.abs(x.reshape(B, C, -1)).astype(np.float64)
    acc = np.broadcast_to(br[None, :, None], ax.shape).astype(np.float32)
    with np.errstate(all="ignore"):
        for j in range(C):
            acc = (acc.astype(np.float64) + gr[None, :, j, None].astype(np.float64) * ax[:, j, None, :]).astype(np.float32)
        acc = acc.reshape(x.shape)
        return (x * acc if inverse else x / acc).astype(np.float32)


def perm_closed_form(x, beta, inverse):
    """The `perm` class in float32: x_i / fl(beta'_i + |x_pi(i)|), inverse x_i * fl(...): every other term of the sum is an exact 0."""
    C = x.shape[1]
    br, _ = gdn_reparam_np(beta, np.zeros((C, C), np.float32))
    norm = (br[None, :, None, None] + np.abs(x[:, perm_of(C)])).astype(np.float32)
    return (x * norm if inverse else x / norm).astype(np.float32)


def below_closed_form(x, beta, inverse):
    """The `below` class in float32: x / beta'[c], inverse x * beta'[c]."""
    C = x.shape[1]
    br, _ = gdn_reparam_np(beta, np.zeros((C, C), np.float32))
    br = br[None, :, None, None]
    return (x * br if inverse else x / br).astype(np.float32)


def worst_fraction(got, want, C):
    """Largest element-wise relative error of `got` against the float64 `want`, as a fraction of (C + 2) 2^-24, over the elements
    where `want` is finite and not 0.  Zeros are not measured here: zeros_agree."""
    m = np.isfinite(want) & (want != 0)
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        e = np.abs(got.astype(np.float64)[m] - want[m]) / np.abs(want[m])
    e = np.where(np.isnan(e), np.inf, e)                              # a NaN or inf where float64 is finite is a miss, not a skip
    return float(e.max()) / bound(C)


def zeros_agree(got, want):
    """Where float64 is exactly 0, `got` is 0 with the same sign."""
    z = want == 0
    return bool((got[z] == 0).all() and (np.signbit(got[z]) == np.signbit(want[z])).all())


def nonfinite_agree(got, want):
    """NaN mask and signed-inf mask of `got` equal those of the float32 cast of the float64 `want`."""
    with np.errstate(all="ignore"):
        w = want.astype(np.float32)
    return bool((np.isnan(got) == np.isnan(w)).all() and (np.isposinf(got) == np.isposinf(w)).all()
                and (np.isneginf(got) == np.isneginf(w)).all())


def ulp_distance(a, b):
    """Largest distance in float32 steps between two finite float32 arrays (0: bit-equal up to the sign of a zero)."""
    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b))).max())


def old_workgroups(HW, B, cus):
    """gdn_launch's grid rule as it stood before it became gdn_workgroups: max(1, min(tiles, ceil(4 CUs / B)))."""
    tiles = -(-HW // TILE)
    return max(1, min(tiles, -(-4 * cus // B))), tiles
