"""References and input builders of region-of-interest coding (tests/test_price_map_host.py pins them on the CPU,
tests/test_gpu_price_map.py runs the kernels against them).  No GPU here.

The decision of include/cdc_hip.h (cdc_set_rdo_map) on the references of tests/rdo_ref.py, which stay as they are: the price of a bit
of element i of an image [C][P] is the FLOAT32 product eff = fl32(mu * g[i mod P]); the float64 margin is float64(eff) dR - dD.  A
symbol whose effective price is exactly 0 never moves in any arithmetic (0 * dR > dD is false for dD >= 0): it is decided, and
checked exactly.  The band and the cap are the project's (R.BAND_FACTOR, R.UNDECIDED_CAP).

The cell mean of cdc_price_cells, restated in float64 in the order the header states: pixel e of the cell's part of the window
(row-major) to lane e mod 64 in ascending order, an xor butterfly over the 64 lanes, the division by the count, one cast to float32;
a cell beyond the window takes the value of the cell its clamped indices name.
"""
import numpy as np

import rdo_ref as R

MUS = np.array([0.0, 0.5, 2.0], np.float32)                # the three images of the op-level cases: effective prices stay <= 8
CASES = ((1, 1), (3, 5), (7, 37), (5, 259), (32, 16), (32, 96))        # (C, P)
FIXED = np.array([1.0, 0.25, 4.0, 0.125, 0.0], np.float32)            # the last positions of every map row
DYADIC = np.array([0.0, 0.125, 0.25, 1.0, 4.0], np.float32)           # pixel values whose float64 sums are exact in any order


def op_case(C, P):
    """(latent, mean, scale) float32 [3, C, P]: R.op_case(C * P), reshaped."""
    return tuple(np.ascontiguousarray(a.reshape(3, C, P)) for a in R.op_case(C * P))


def map_case(n, P, seed=0):
    """A price map float32 [n, P]: log-uniform in [2^-3, 2^2], the values FIXED (as many as fit, from its first) at the last positions
    of each row."""
    rng = np.random.default_rng([seed, n, P])
    g = np.exp2(rng.uniform(-3.0, 2.0, (n, P))).astype(np.float32)
    k = min(P, FIXED.size)
    g[:, P - k:] = FIXED[:k]
    return g


def effective(mu, g, C):
    """fl32(mu_b * g[b][p]) per element -> float32 [B, C, P]; g [n, P] with n = 1 or B."""
    mu = np.asarray(mu, np.float32).reshape(-1, 1)
    g = np.asarray(g, np.float32)
    eff = (mu * np.broadcast_to(g, (mu.shape[0], g.shape[1]))).astype(np.float32)       # one float32 product
    return np.ascontiguousarray(np.broadcast_to(eff[:, None, :], (eff.shape[0], C, eff.shape[1])))


def margin64(t, eff):
    """float64(eff) dR - dD: > 0 moves."""
    return eff.astype(np.float64) * t["dR"] - t["dD"]


def decide64(t, eff):
    return (t["k0"] != 0) & (margin64(t, eff) > 0)


def margin32(y, m, s, eff):
    """The float32 method: (eff * dR) - dD with every operation rounded to float32 (R.terms32's dR and dD)."""
    dR32, dD32 = R.terms32(y, m, s)
    return ((eff * dR32).astype(np.float32) - dD32).astype(np.float32)


def method_band(y, m, s, eff):
    """R.BAND_FACTOR x the largest |float32 - float64| of the margin over these inputs -> (band, worst)."""
    t = R.terms64(y, m, s)
    worst = float(np.max(np.abs(margin32(y, m, s, eff).astype(np.float64) - margin64(t, eff))))
    return R.BAND_FACTOR * worst, worst


def undecided(t, eff, band):
    """Symbols whose float64 margin lies inside the band.  k0 = 0 cannot move and eff = 0 never moves: both are decided."""
    return (t["k0"] != 0) & (eff != 0) & (np.abs(margin64(t, eff)) < band)


def quantise64(y, m, s, eff):
    """-> (q float32 = k + m of the float64 decision, moved bool)."""
    t = R.terms64(y, m, s)
    mv = decide64(t, eff)
    return np.where(mv, t["x1"], t["x0"]).astype(np.float32), mv


# ---- the cell mean ------------------------------------------------------------------------------------------------------------------

def _wave_sum(values):
    """float64 values (row-major pixels of one cell) -> the sum in the kernel's order: lane e mod 64 ascending, then the xor butterfly."""
    lanes = np.zeros(64, np.float64)
    for e0 in range(0, values.size, 64):
        chunk = values[e0:e0 + 64]
        lanes[:chunk.size] = lanes[:chunk.size] + chunk
    idx = np.arange(64)
    for mask in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[idx ^ mask]
    return lanes[0]


def cells_ref(pixel_map, H, W, cell, gh, gw):
    """pixel_map float32 [n, Hf, Wf] (only its top-left H x W window is read) -> cells float32 [n, gh, gw]."""
    pm = np.asarray(pixel_map, np.float32)
    n = pm.shape[0]
    out = np.empty((n, gh, gw), np.float32)
    for i in range(n):
        for gy in range(gh):
            cy = min(gy, (H - 1) // cell)
            for gx in range(gw):
                cx = min(gx, (W - 1) // cell)
                part = pm[i, cy * cell:min((cy + 1) * cell, H), cx * cell:min((cx + 1) * cell, W)].astype(np.float64).reshape(-1)
                out[i, gy, gx] = np.float32(_wave_sum(part) / float(part.size))
    return out


def dyadic_map(n, H, W, seed=0, Hf=None, Wf=None, poison=np.nan):
    """A pixel map float32 [n, Hf, Wf] of DYADIC values in blocks of 1 to 7 pixels over the H x W window; everything outside the
    window is `poison`."""
    Hf, Wf = Hf or H, Wf or W
    rng = np.random.default_rng([seed, n, H, W])
    pm = np.full((n, Hf, Wf), poison, np.float32)
    coarse = DYADIC[rng.integers(0, DYADIC.size, (n, -(-H // 5), -(-W // 3)))]
    fine = DYADIC[rng.integers(0, DYADIC.size, (n, H, W))]
    block = np.repeat(np.repeat(coarse, 5, axis=1), 3, axis=2)[:, :H, :W]
    pm[:, :H, :W] = np.where(rng.random((n, H, W)) < 0.2, fine, block)
    return pm
