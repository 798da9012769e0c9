"""Parallel-in-time decode (include/cdc_hip.h: cdc_decode_parallel): the stride rule, the window bookkeeping and the
argument rules, in plain Python so that they can be read and tested without a device.

The library's host loop (csrc/cdc_decode.hip: window_stride, window_row_steps) is the code that decides; `stride` and `row_steps` here
restate it, and tests/test_picard_host.py runs the same hand-made tables through both (cdc_parallel_stride, cdc_parallel_row_steps), so
the two cannot drift apart unnoticed.  `solve` is the sweep loop over any chain of maps, which the tests run on a float64 toy chain.
A sampler chain y_{j+1} = Phi_j(y_j), j = 0 .. N-1, is solved by sweeps over a window of p steps at base w (Shih et al., "Parallel Sampling of Diffusion Models", 2023):

    c_0 = 0;   y'_{w+m+1} = Phi_{w+m}(y_{w+m}) + c_m;   c_{m+1} = y'_{w+m+1} - y_{w+m+1};   r_m = sum (y'_{w+m+1} - y_{w+m+1})^2

which in exact arithmetic is the prefix sum y'_{w+m+1} = y_w + sum_{l <= m} (Phi_{w+l}(y_{w+l}) - y_{w+l}).  Row 0 is always final."""
import math

DEFAULT_WINDOW = 16
# In the image's [-1, 1] units: a quarter of the half-step of the uint8 rounding of as_uint8 (1 / 255 = 3.9e-3).  A starting value, not
# a measured optimum: nobody has measured sweep counts or the accumulated deviation on trained weights.
DEFAULT_TOL = 1e-3
MAX_WINDOW = 256            # the update kernel's rows
MAX_ROWS = 65535            # B * window: what cdc_decode_samples accepts as rows


def live_rows(w, p, steps):
    """The rows of the window at base w that lie inside the schedule; the other p - live are dead."""
    return max(0, min(p, steps - w))


def row_steps(w, p, steps):
    """The sample index i = steps - 1 - j of the state in every slot of the ring at window base w: slot (j mod p) holds y_j,
    j = w .. w + p - 1.  A dead row's index is clamped to 0: it is evaluated, and nobody reads the result."""
    out = [0] * p
    for k in range(p):
        out[(w + k) % p] = max(0, steps - 1 - (w + k))
    return out


def stride(residuals, numel, tol, live):
    """The stride of a sweep.  residuals: [B][p] sums of squared changes per image and row; numel: the elements of an image.  The number
    of leading live rows that EVERY image accepts, sqrt(r / numel) <= tol, and at least 1 (a NaN accepts nothing)."""
    s = 0
    while s < live and all(math.sqrt(r[s] / numel) <= tol for r in residuals):
        s += 1
    return max(1, s)


def sweep(phis, ys, w, p):
    """One sweep in the recurrence form over the states ys (list, ys[j] the guess of y_j, len >= w + p + 1 or up to the chain's end):
    -> (new guesses of y_{w+1} .. y_{w+live}, residuals r_0 .. r_{live-1}).  ys is not changed."""
    N = len(phis)
    live = live_rows(w, p, N)
    new, res, c = [], [], 0.0
    for m in range(live):
        y = phis[w + m](ys[w + m]) + c
        c = y - ys[w + m + 1]
        res.append(_sumsq(c))
        new.append(y)
    return new, res


def sweep_prefix(phis, ys, w, p):
    """The same sweep in the Picard prefix-sum form: y'_{w+m+1} = y_w + sum_{l <= m} (Phi_{w+l}(y_{w+l}) - y_{w+l})."""
    N = len(phis)
    new, acc = [], 0.0
    for m in range(live_rows(w, p, N)):
        acc = acc + (phis[w + m](ys[w + m]) - ys[w + m])
        new.append(ys[w] + acc)
    return new


def _sumsq(c):
    try:
        return float((c * c).sum())
    except AttributeError:
        return float(c * c)


def _numel(y):
    return int(getattr(y, "size", 1))


def solve(phis, y0, p, tol):
    """The sweep loop over a chain of maps: -> (y_N, strides).  Every state starts as y_0 (the constant guess); new window positions
    start as the last state computed."""
    N = len(phis)
    ys = [y0] * (N + 1)
    w, strides = 0, []
    while w < N:
        new, res = sweep(phis, ys, w, p)
        live = len(new)
        ys[w + 1:w + 1 + live] = new
        s = stride([res], _numel(y0), tol, live)
        for j in range(w + live + 1, min(N, w + p + s) + 1):       # the positions the slide uncovers
            ys[j] = new[-1]
        strides.append(s)
        w += s
    return ys[N], strides


def check_args(parallel, parallel_tol, steps, B, sampler="ddim", eta=0, seed=None, tile=None, samples=None, trajectory=None):
    """The argument rules of `parallel=`, checked before anything runs: -> (window, tol), or None when parallel is None / False.
    parallel=True is a window of 16; a window above `steps` is the whole schedule."""
    if parallel is None or parallel is False:
        if parallel_tol is not None:
            raise ValueError("parallel_tol belongs to parallel=")
        return None
    p = DEFAULT_WINDOW if parallel is True else int(parallel)
    tol = DEFAULT_TOL if parallel_tol is None else float(parallel_tol)
    if sampler != "ddim":
        raise ValueError(f'parallel: sampler "{sampler}" carries a history, which makes a step a map of two states; only "ddim" is supported')
    if tile is not None:
        raise ValueError("parallel excludes tile=: a tiled decode fills its batch rows with tiles")
    if samples is not None:
        raise ValueError("parallel excludes samples=: K samples fill the batch rows a window would use")
    if trajectory is not None:
        raise ValueError("parallel excludes trajectory=: a sweep has no single x0 per step to record")
    if eta != 0 and seed is None:
        raise ValueError("parallel with eta != 0 needs a seed: a noise tensor is not supported, the draws must be a function of (seed, step)")
    if p < 2:
        raise ValueError(f"parallel={p}: the window must hold at least 2 steps")
    if steps is not None:
        if steps < 2:
            raise ValueError(f"parallel needs a schedule of at least 2 steps, got {steps}")
        p = min(p, int(steps))
    if p > MAX_WINDOW:
        raise ValueError(f"parallel={p}: the window may hold at most {MAX_WINDOW} steps")
    if B is not None and B * p > MAX_ROWS:
        raise ValueError(f"parallel: B * window = {B * p} rows, beyond {MAX_ROWS}")
    if not tol >= 0:
        raise ValueError(f"parallel_tol={tol}: must be >= 0")
    return p, tol
