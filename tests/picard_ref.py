"""One Picard sweep of cdc_op_window_update (include/cdc_hip.h: THE SWEEP) stated in NumPy over tests/sampler_ref.py's DDIM update: the
recurrence in float64 with its elementwise bound, the same recurrence operation by operation in float32, and the residuals of a set
of returned values.  Test infrastructure without a GPU.

Layout: fx [B][p][C][H][W] (row m: the model output of state y_{w+m}); y [B][p + 1][C][H][W] (the guesses of y_w .. y_{w+p}); row m is the
update of sample index steps - 1 - (w + m); noise[m]: the draws of that row [B][C][H][W], or None.

The bound of row m (the new guess of y_{w+m+1}), element by element:
    sum over l <= m of sampler_ref's bound of row l's update     (<= (m + 1) times the largest of them)
    + 2 (m + 1) 2^-24 ymax                                       one add and one subtract per row, each rounded once
ymax: the largest magnitude among every value the recurrence forms -- updates, new guesses, old guesses and carries -- so that it
bounds each rounded result.  Every row's update is evaluated on the GIVEN float32 guess (the one the U-Net saw), so no error passes
through an update: the carry is the only path from row to row."""
import numpy as np

import sampler_ref as R

U = R.U


def live_rows(w, p, steps):
    return min(p, steps - w)


def sweep_f64(s, w, fx, y, noise, eta, pred, clip):
    """-> (new [B][live][...] float64, bound [B][live][...]).  s: the SampleSchedule."""
    B, p = fx.shape[:2]
    live = live_rows(w, p, s.steps)
    c = np.zeros(fx[:, 0].shape, np.float64)
    acc = np.zeros_like(c)
    new, ymax, bounds = [], 0.0, []
    for m in range(live):
        i = s.steps - 1 - (w + m)
        phi, b = R.ddim_update_f64(s, i, fx[:, m], y[:, m], None if noise is None else noise[m], eta, pred, clip)
        yn = phi + c
        old = y[:, m + 1].astype(np.float64)
        c = yn - old
        acc = acc + b
        ymax = max(ymax, float(np.abs(phi).max()), float(np.abs(yn).max()), float(np.abs(old).max()), float(np.abs(c).max()))
        new.append(yn)
        bounds.append(acc.copy())
    new, bounds = np.stack(new, 1), np.stack(bounds, 1)
    for m in range(live):
        bounds[:, m] += 2 * (m + 1) * U * ymax
    return new, bounds


def sweep_f32(s, w, fx, y, noise, eta, pred, clip, c_eps=None):
    """The same recurrence in float32, every operation rounded on its own -> new [B][live][...] float32."""
    B, p = fx.shape[:2]
    live = live_rows(w, p, s.steps)
    c = np.zeros(fx[:, 0].shape, np.float32)
    new = []
    for m in range(live):
        i = s.steps - 1 - (w + m)
        ce = None if c_eps is None else R.step_scalars(s, i, eta, pred)["c_eps"][c_eps]
        yn = R.ddim_update_f32(s, i, fx[:, m].copy(), y[:, m].copy(), None if noise is None else noise[m], eta, pred, clip, c_eps=ce) + c
        c = yn - y[:, m + 1]
        assert yn.dtype == np.float32 and c.dtype == np.float32
        new.append(yn)
    return np.stack(new, 1)


def residuals(new, y):
    """r [B][live]: float64 sums over the image of the float32 squares of the float32 differences new - old."""
    live = new.shape[1]
    d = new.astype(np.float32) - y[:, 1:live + 1]
    sq = d * d
    assert sq.dtype == np.float32
    return sq.astype(np.float64).reshape(new.shape[0], live, -1).sum(axis=2)


def inputs(B, p, shape, seed=5):
    """fx [B][p][...], y [B][p + 1][...]: float32.  The guesses of neighbouring states lie close to each other, as a window's do."""
    from cdc_compression_amd import synth
    fx = synth.normal("fx", (B, p) + tuple(shape), seed=seed, std=1.2)
    base = synth.normal("y", (B, 1) + tuple(shape), seed=seed + 1, std=0.8)
    y = (base + synth.normal("dy", (B, p + 1) + tuple(shape), seed=seed + 2, std=0.05)).astype(np.float32)
    return fx, y
