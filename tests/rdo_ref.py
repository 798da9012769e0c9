"""References and input builders of the rate-distortion optimised quantiser (tests/test_rdo_host.py pins them on the CPU,
tests/test_gpu_rdo.py runs the kernels against them).  No GPU here.

The decision of include/cdc_hip.h (cdc_set_rdo), restated twice on the same float32 operands (y, m, s):
    terms64   the float64 restatement the kernels are held to,
    terms32   the float32 method, operation by operation with torch on the CPU; it exists only to measure what the method itself
              loses against float64 in mu * dR - dD, which sizes the band inside which a float32 decision may differ.
The discrete part is common to both and exact: d = y - m in float32 and k0 = rint(d) are today's symbol, as latent_symbols_kernel
computes it; k1 = k0 - sign(k0); the candidates are priced at the float32 values k + m the decoder reconstructs.
"""
import numpy as np

from oracle import model as om

BAND_FACTOR = 10.0            # the band is this multiple of the largest |float32 - float64| of mu dR - dD over a test's own inputs
UNDECIDED_CAP = 0.01          # at most this share of a case's symbols may lie inside the band
MUS = np.array([0.0, 0.5, 8.0], np.float32)      # the three images of the op-level cases
PER_IMAGE = (1, 63, 257, 4 * 256 + 3)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def candidates(y, m):
    """(d, k0, k1) float32: the float32 difference, today's symbol and its neighbour towards the mean (k1 = k0 where k0 = 0)."""
    y, m = _f32(y), _f32(m)
    d = y - m
    k0 = np.rint(d).astype(np.float32)
    k1 = (k0 - np.sign(k0)).astype(np.float32)
    return d, k0, k1


def price64(x, m, s):
    """Bits of the float32 value x under (m, s), float64: -log2 of oracle/model.py's clamped likelihood."""
    return -np.log2(om.normal_likelihood(_f32(x), _f32(m), _f32(s)))


def terms64(y, m, s):
    """-> dict of float64 arrays: bits0, bits1, dR, dD, and the float32 candidates d, k0, k1, x0 = k0 + m, x1 = k1 + m."""
    m, s = _f32(m), _f32(s)
    d, k0, k1 = candidates(y, m)
    x0, x1 = (k0 + m).astype(np.float32), (k1 + m).astype(np.float32)
    b0, b1 = price64(x0, m, s), price64(x1, m, s)
    b1 = np.where(k0 == 0, b0, b1)
    d64, k64 = d.astype(np.float64), k0.astype(np.float64)
    e = np.abs(d64) - np.abs(k64)
    return {"d": d, "k0": k0, "k1": k1, "x0": x0, "x1": x1, "bits0": b0, "bits1": b1, "dR": b0 - b1, "dD": 2.0 * e + 1.0}


def terms32(y, m, s):
    """The same in float32, one torch operation per operation of csrc/rdo_terms.h / csrc/rate_terms.h -> (dR, dD) float32."""
    import torch
    t = lambda a: torch.from_numpy(_f32(a).copy())       # noqa: E731
    m32, s32 = t(m), t(s)
    d, k0, k1 = (t(a) for a in candidates(y, m))
    c = -(2 ** -0.5)

    def bits(k):
        a = torch.abs((k + m32) - m32)
        up = 0.5 * torch.erfc(c * ((0.5 - a) / s32))
        lo = 0.5 * torch.erfc(c * ((-0.5 - a) / s32))
        return -torch.log2((up - lo).clamp(min=1e-9))
    b0 = bits(k0)
    b1 = torch.where(k0 == 0, b0, bits(k1))
    e = torch.abs(d) - torch.abs(k0)
    return (b0 - b1).numpy(), (2.0 * e + 1.0).numpy()


def margin64(t, mu):
    """mu dR - dD in float64: > 0 moves."""
    return np.float64(np.float32(mu)) * t["dR"] - t["dD"]


def decide64(t, mu):
    """The float64 decision -> bool array `move`."""
    return (t["k0"] != 0) & (margin64(t, mu) > 0)


def method_band(y, m, s, mus):
    """BAND_FACTOR x the largest |float32 - float64| of mu dR - dD over these inputs and these mu (the CPU-side measurement)."""
    t = terms64(y, m, s)
    dR32, dD32 = terms32(y, m, s)
    worst = 0.0
    for mu in np.asarray(mus, np.float32).reshape(-1):
        m32 = (np.float32(mu) * dR32 - dD32).astype(np.float64)       # float32 product and difference
        worst = max(worst, float(np.max(np.abs(m32 - margin64(t, mu)))))
    return BAND_FACTOR * worst, worst


def quantise64(y, m, s, mu):
    """-> (q float32 = k + m of the float64 decision, moved bool)."""
    t = terms64(y, m, s)
    mv = decide64(t, mu)
    return np.where(mv, t["x1"], t["x0"]).astype(np.float32), mv


def sweep64(y, m, s, mus):
    """The sums of cdc_entropy_rate_sweep's latent part for one image in float64 -> (bits [L], sse [L], moved [L])."""
    t = terms64(y, m, s)
    y64 = _f32(y).astype(np.float64)
    bits, sse, moved = [], [], []
    for mu in np.asarray(mus, np.float32).reshape(-1):
        mv = decide64(t, mu)
        q = np.where(mv, t["x1"], t["x0"]).astype(np.float64)
        bits.append(float(np.where(mv, t["bits1"], t["bits0"]).sum()))
        sse.append(float(((y64 - q) ** 2).sum()))
        moved.append(int(mv.sum()))
    return np.array(bits), np.array(sse), np.array(moved, np.int64)


# ---- inputs of the op-level cases ----------------------------------------------------------------------------------------------------

def _edges(b):
    """Hand-made (d, s, m) triples of image b, the classes in this order so that a short image holds the first of each: the rintf ties
    d = +-0.5 (k0 = 0) and +-1.5 (k0 = +-2, dD = 0; +-2.5 with dD = 2 in image 0, whose mu = 0 leaves a dD = 0 symbol on the decision's
    edge by construction), k0 = +-1 (a move lands on 0), k0 = 0, tails where both prices sit on the 1e-9 clamp, |m| up to 1e4 (the
    rounding of k + m), the scale points 0.1 and 2048."""
    rows = []
    for d in (0.5, -0.5, 1.5, -1.5):
        for s in (0.3, 1.0, 3.0):
            rows.append((d if abs(d) < 1 or b else d + np.sign(d), s, 0.0))
    for d in (1.0, -1.0, 0.75, -0.75, 1.25, -1.25, 1.45, -1.45, 0.51, -0.51):                   # k0 = +-1
        rows.append((d, (0.1, 0.25, 0.6, 2.0, 64.0)[len(rows) % 5], 0.25))
    for d in (0.0, 0.25, -0.25, 0.49, -0.49):                                                   # k0 = 0
        rows.append((d, (0.1, 1.0, 2048.0)[len(rows) % 3], -1.75))
    for d in (30.0, -30.0, 40.3, -41.7, 200.0, -7.0):                                            # both prices on the clamp
        rows.append((d, (0.1, 0.5, 1.0)[len(rows) % 3], 3.0))
    for m in (1.0e4, -1.0e4, 9999.37, -8191.99, 4096.5, 1234.567):                               # k + m rounds
        for d in (1.3, -2.6):
            rows.append((d, (0.1, 1.5, 20.0)[len(rows) % 3], m))
    for d in (2.5, -2.5, 1.0, -3.25):                                                            # the scale points
        for s in (0.1, 2048.0):
            rows.append((d, s, 0.5))
    a = np.array(rows, np.float64)
    return a[:, 0], a[:, 1], a[:, 2]


def op_case(per_image, seed=0):
    """(latent, mean, scale) float32 [3, per_image]: the hand-made edges of each image first (as many as fit), then scales log-uniform
    in [0.1, 64] with d = 1.5 s N(0, 1) and means 2 N(0, 1).  per_image = 1: one k0 = -1 symbol an image."""
    B = MUS.size
    rng = np.random.default_rng([seed, per_image])
    s = np.exp(rng.uniform(np.log(0.1), np.log(64.0), (B, per_image)))
    d = 1.5 * s * rng.standard_normal((B, per_image))
    m = 2.0 * rng.standard_normal((B, per_image))
    for b in range(B):
        ed, es, em = _edges(b)
        if per_image == 1:
            ed, es, em = np.array([-1.25]), np.array([0.6]), np.array([0.25])
        n = min(per_image, ed.size)
        d[b, :n], s[b, :n], m[b, :n] = ed[:n], es[:n], em[:n]
    mean = m.astype(np.float32)
    scale = s.astype(np.float32)
    latent = (mean.astype(np.float64) + d).astype(np.float32)
    return latent, mean, scale


def undecided(t, mu, band):
    """Symbols whose float64 margin lies inside the band (a symbol with k0 = 0 cannot move: always decided)."""
    return (t["k0"] != 0) & (np.abs(margin64(t, mu)) < band)
