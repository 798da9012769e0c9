"""Inputs and float64 references of the rate / error map tests (tests/test_rd_maps_host.py asserts their conditions on the CPU,
tests/test_gpu_rd_maps.py runs cdc_rate_map and cdc_distortion_map against them).  No GPU here.  The per-symbol prices come from
tests/rate_ref.py (rate_terms_f64 the reference, rate_terms_f32 the float32 method whose own loss sets the tolerance); this file
only sums them along the axes the maps sum along, and builds the moved-symbol batch of the geometry test."""
import functools

import numpy as np

import rate_ref as R

U = R.UP
MAPS = ("latent", "hyper", "cell", "latent_channels", "hyper_channels")

GEOMETRY_HW = (2, 3)                                                   # hyper latent 2 x 3, latent 8 x 12
LATENT_MOVES = (((0, 0), 0), ((0, 11), 127), ((7, 0), 64), ((7, 11), 5), ((3, 5), 77))      # ((y, x), channel)
HYPER_MOVES = (((0, 0), 3), ((1, 2), 127), ((0, 1), 60))               # ((yh, xh), channel)
LATENT_MOVE, HYPER_MOVE = 1.0, 3.0                                     # the moved symbol's distance from its mean / median

TYPICAL_HW = (5, 4)                                                    # latent 20 x 16 = 320 positions: more than one workgroup's
TYPICAL_B = 3


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def sums(h, c):
    """Per-symbol terms (hyper [B, CH, hh, wh], latent [B, CL, U hh, U wh], float64) -> the five maps' sums, float64."""
    latent, hyper = c.sum(axis=1), h.sum(axis=1)
    cell = latent + np.repeat(np.repeat(hyper, U, axis=1), U, axis=2) / float(U * U)
    return {"latent": latent, "hyper": hyper, "cell": cell, "latent_channels": c.sum(axis=(2, 3)), "hyper_channels": h.sum(axis=(2, 3))}


def references(qh, ql, mu, sc):
    """(ref, own): per map the float64 value of every entry and what the float32 method itself loses on the entry's terms
    (sum of |r32 - r64|): the two figures of the tolerance rule of tests/test_gpu_rate_edges.py, per entry."""
    sd = R.prior_sd()
    h64, c64 = R.rate_terms_f64(sd, qh, ql, mu, sc)
    h32, c32 = R.rate_terms_f32(sd, qh, ql, mu, sc)
    return sums(h64, c64), sums(np.abs(h32 - h64), np.abs(c32 - c64)), (h64, c64)


def tolerance(ref, own):
    """8 x the float32 method's own loss on the entry's terms + 4 float32 ulps of the entry."""
    return 8.0 * own + 4.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def class_case():
    """(a): rate_ref.class_batch(0), nine images at a 1 x 1 hyper latent."""
    names, qh, ql, mu, sc = R.class_batch(0)
    ref, own, terms = references(qh, ql, mu, sc)
    return names, _frozen(qh, ql, mu, sc), ref, own, terms


@functools.lru_cache(maxsize=None)
def geometry_case():
    """(b): image 0 is the baseline (every hyper symbol on its median, the quiet latent part); image 1 + i moves the latent symbol of
    LATENT_MOVES[i], image 1 + len(LATENT_MOVES) + j the hyper symbol of HYPER_MOVES[j]."""
    hh, wh = GEOMETRY_HW
    n = 1 + len(LATENT_MOVES) + len(HYPER_MOVES)
    qh = np.broadcast_to(R.medians()[None, :, None, None], (n, R.CH, hh, wh)).copy()
    ql, mu, sc = (np.broadcast_to(a[None], (n,) + a.shape).copy() for a in R.quiet_gauss(hh, wh))
    for i, ((y, x), c) in enumerate(LATENT_MOVES, 1):
        ql[i, c, y, x] += np.float32(LATENT_MOVE)
    for j, ((y, x), c) in enumerate(HYPER_MOVES, 1 + len(LATENT_MOVES)):
        qh[j, c, y, x] += np.float32(HYPER_MOVE)
    ref, own, terms = references(qh, ql, mu, sc)
    return _frozen(qh, ql, mu, sc), ref, own, terms


@functools.lru_cache(maxsize=None)
def typical_case():
    """(c): TYPICAL_B seeded images of the `typical` Gaussian class over the `centre` hyper class at a 5 x 4 hyper latent."""
    hh, wh = TYPICAL_HW
    parts = [R.gauss_class("typical", 100 + b, hh, wh) for b in range(TYPICAL_B)]
    qh = np.stack([R.hyper_class("centre", 100 + b, hh, wh) for b in range(TYPICAL_B)])
    ql, mu, sc = (np.stack([p[k] for p in parts]) for k in range(3))
    ref, own, terms = references(qh, ql, mu, sc)
    return _frozen(qh, ql, mu, sc), ref, own, terms


# ---- error maps -----------------------------------------------------------------------------------------------------------------------

def cell_sums(v, cell, gh, gw):
    """v [B, 3, H, W] -> [B, gh, gw]: the sum of v over the three channels and the pixels of each cell inside the window; and the
    int32 count of the summed elements."""
    B, _, H, W = v.shape
    out = np.zeros((B, gh, gw), v.dtype)
    count = np.zeros((B, gh, gw), np.int32)
    for gy in range(gh):
        for gx in range(gw):
            blk = v[:, :, gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell]
            out[:, gy, gx] = blk.sum(axis=(1, 2, 3))
            count[:, gy, gx] = blk.shape[1] * blk.shape[2] * blk.shape[3]
    return out, count
