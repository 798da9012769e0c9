"""Float64 restatement of Residual(PreNorm(LinearAttention)) (xparam / epsilonparam network_components.py:10-16, 56-77, 117-139) and the
input cases that put the operator's softmax at its edges.  Plain numpy, no dependency on oracle/: what the GPU kernels are compared with
(tests/test_gpu_attention_edges.py), pinned to the real reference's float64 run by tests/golden/attention_edges.npz
(tests/golden/make_golden_attention.py, tests/test_attention_host.py).

Every builder is a pure function of (seed, shape) made of exact operations only (synth.normal, IEEE + - * / sqrt, correctly rounded
sums), so every host regenerates the same bits; the fixture stores a checksum of them.  A builder returns
(x, norm_g, norm_b, w_qkv, w_out, b_out), the arguments of Ops.linear_attention.  From a batch of 5 on, the images repeat the first
four."""
import hashlib
import math

import numpy as np

from cdc_compression_amd import synth

SEED = 24              # the seed of the operator tests in tests/test_gpu_parity.py, whose inputs the `normal` case is
SEED_BACKGROUND = 30   # ... but `background`: the first seed at which its window condition holds at every shape of PATHS (24 channels included)
SEED_OFFSET = 26       # ... and `offset`: the first seed at which max |ref| stays below 1000 (the fp16 range of the planes) at every shape
DISTINCT = 4           # distinct images of a large batch


# ---- the operator ------------------------------------------------------------------------------------------------------------------------

def softmax_weights(x, norm_g, norm_b, w_qkv):
    """(k [B, C, N], softmax of k over the pixels [B, C, N]) in float64."""
    x, g, b, wq = (np.asarray(a, np.float64) for a in (x, norm_g, norm_b, w_qkv))
    B, C, H, W = x.shape
    k = np.matmul(wq.reshape(3 * C, C)[C:2 * C], _layernorm(x, g, b).reshape(B, C, H * W))
    p = np.exp(k - k.max(-1, keepdims=True))
    return k, p / p.sum(-1, keepdims=True)


def _layernorm(x, g, b, eps=1e-5):
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)            # biased, as torch.var(unbiased=False)
    return (x - mean) / np.sqrt(var + eps) * g.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)


def linear_attention(x, norm_g, norm_b, w_qkv, w_out, b_out, parts=False):
    """y = to_out(ctx^T (q C^-1/2)) + x with q, k, v = to_qkv(LayerNorm(x)), ctx = softmax_N(k) v^T; float64 [B, C, H, W].
    parts: (y, ctx [B, C, C], v [B, C, N]) instead."""
    x, g, b, wq, wo, bo = (np.asarray(a, np.float64) for a in (x, norm_g, norm_b, w_qkv, w_out, b_out))
    B, C, H, W = x.shape
    qkv = np.matmul(wq.reshape(3 * C, C), _layernorm(x, g, b).reshape(B, C, H * W))
    q, k, v = qkv[:, :C] * C ** -0.5, qkv[:, C:2 * C], qkv[:, 2 * C:]
    p = np.exp(k - k.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ctx = np.matmul(p, v.transpose(0, 2, 1))                                  # [B, d, e]
    out = np.matmul(ctx.transpose(0, 2, 1), q)                                # [B, e, N]
    y = (np.matmul(wo.reshape(C, C), out) + bo.reshape(1, C, 1)).reshape(B, C, H, W) + x
    return (y, ctx, v) if parts else y


def reference(args, fn=None):
    """linear_attention(*args) (or fn(args)) where a large batch repeats its first DISTINCT images (the builders' rule): computed once
    per image."""
    fn = fn or (lambda a: linear_attention(*a))
    B = args[0].shape[0]
    if B <= DISTINCT:
        return fn(args)
    assert np.array_equal(args[0], args[0][np.arange(B) % DISTINCT])
    return fn((args[0][:DISTINCT], *args[1:]))[np.arange(B) % DISTINCT]


def relerr(got, ref):
    """max |got - ref| / max(1, max |ref|): the project's error measure (tests/test_gpu_parity.py)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def checksum(args):
    """sha256 over the bytes of the six float32 arguments: a host on which a builder gives other bits fails loudly."""
    h = hashlib.sha256()
    for a in args:
        a = np.ascontiguousarray(a)
        assert a.dtype == np.float32
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def _params(seed, C, b_mean=0.0):
    return [synth.normal("ag", (1, C, 1, 1), seed, 0.2, 1.0), synth.normal("ab", (1, C, 1, 1), seed, 0.2, b_mean),
            synth.normal("aq", (3 * C, C, 1, 1), seed, 2.0 / np.sqrt(C)), synth.normal("ao", (C, C, 1, 1), seed, 1.0 / np.sqrt(C)),
            synth.normal("aob", (C,), seed, 0.1)]


def _batch(shape):
    return (min(shape[0], DISTINCT),) + tuple(shape[1:])


def _repeat(x, B):
    return x if x.shape[0] == B else np.ascontiguousarray(x[np.arange(B) % x.shape[0]])


def _scale_k(p, f):
    C = p[2].shape[1]
    p[2] = p[2].copy()
    p[2][C:2 * C] *= np.float32(f)
    return p


def case_normal(seed, shape):
    """x ~ N(0, 1), to_qkv of std 2 / sqrt(C): every softmax row a mild bump (the inputs of the older operator tests)."""
    return (_repeat(synth.normal("ax", _batch(shape), seed), shape[0]), *_params(seed, shape[1]))


def case_flat(seed, shape):
    """k = 0: a uniform softmax, ctx[d][e] = mean_n v[e][n] for every d."""
    x, *p = case_normal(seed, shape)
    return (x, *_scale_k(p, 0.0))


def case_sharp(seed, shape, factor):
    """k rows x factor: near one-hot rows, most weights underflow, k differences of hundreds."""
    x, *p = case_normal(seed, shape)
    return (x, *_scale_k(p, factor))


def case_offset(seed, shape):
    """norm_b = 5 + 0.2 N: every k row sits on a constant of order 10 to 100."""
    return (_repeat(synth.normal("ax", _batch(shape), seed), shape[0]), *_params(seed, shape[1], b_mean=5.0))


def _fsum_dot(a, b):
    return math.fsum((a * b).tolist())                 # products rounded once each, their sum correctly rounded: the same on every host


def _unit_pair(seed, C):
    """Two zero-mean orthonormal vectors (float64) from two normal draws: Gram-Schmidt on correctly rounded sums."""
    a = synth.normal("ae1", (C,), seed).astype(np.float64)
    b = synth.normal("ae2", (C,), seed).astype(np.float64)
    a = a - math.fsum(a.tolist()) / C
    b = b - math.fsum(b.tolist()) / C
    a = a / math.sqrt(_fsum_dot(a, a))
    b = b - _fsum_dot(a, b) * a
    b = b - math.fsum(b.tolist()) / C
    b = b / math.sqrt(_fsum_dot(b, b))
    return a, b


def _cos_sin(t):
    """cos and sin on [0, pi/2] as Taylor polynomials in Horner form: + and * only (libm's may differ by an ulp between hosts)."""
    t2 = t * t
    c = np.zeros_like(t)
    s = np.zeros_like(t)
    for n in range(26, 0, -2):                         # t^26 / 26! < 1e-21 on the interval
        c = (c + (1.0 if n % 4 == 0 else -1.0) / math.factorial(n)) * t2
        s = (s + (1.0 if n % 4 == 0 else -1.0) / math.factorial(n + 1)) * t2
    return c + 1.0, (s + 1.0) * t


def case_ramp(seed, shape, sign):
    """x[:, n] = cos(t_n) e1 + sin(t_n) e2 + 0.01 N, t_n = (pi / 2) n / N, k rows x (40 sign): k moves along the pixel axis in one sweep.
    In every 32-row block some row's running maximum rises in nearly every 32-pixel tile, so the online softmax takes its rescale
    branch tile after tile, while other rows never rise after their first tile; sign = -1 (`ramp_down`) negates k exactly: the rows
    that rise in `ramp_up` fall, and the other way round."""
    B, C, H, W = shape
    N = H * W
    e1, e2 = _unit_pair(seed, C)
    c, s = _cos_sin((math.pi / 2) * np.arange(N, dtype=np.float64) / N)
    x = (e1[:, None] * c[None, :] + e2[:, None] * s[None, :])[None] + synth.normal("axn", _batch(shape), seed, 0.01).reshape(-1, C, N).astype(np.float64)
    x = x.astype(np.float32).reshape(_batch(shape))
    return (_repeat(x, B), *_scale_k(_params(seed, C), 40.0 * sign))


def case_background(seed, shape, at=None):
    """x[:, n] = e2 + 0.01 N at every pixel but n = `at` (N // 3 unless given), where it is e1 + 0.01 N; k rows x 4: one feature on a
    flat background.  In the rows where the feature carries the maximum, thousands of pixels share one small weight (and nearly one
    v): the coherent tail that a weight format with an ABSOLUTE error bound gets wrong.  `background@n` puts the feature at pixel n:
    first in a split of the fused kernels, every later pixel of that split is weighed against it by the running maximum."""
    B, C, H, W = shape
    N = H * W
    at = N // 3 if at is None else at
    e1, e2 = synth.normal("ae1", (C,), seed), synth.normal("ae2", (C,), seed)
    x = synth.normal("axn", _batch(shape), seed, 0.01).reshape(-1, C, N).astype(np.float64) + e2.astype(np.float64)[None, :, None]
    x[:, :, at] += (e1.astype(np.float64) - e2.astype(np.float64))[None, :]
    x = x.astype(np.float32).reshape(_batch(shape))
    return (_repeat(x, B), *_scale_k(_params(seed, C), 4.0))


def case_peak(seed, shape, n):
    """`sharp8` with every image rolled along its flattened pixel axis so that the arg-max of k row 0 sits at pixel n."""
    x, *p = case_sharp(seed, shape, 8.0)
    B, C, H, W = shape
    xd = x[:min(B, DISTINCT)].reshape(-1, C, H * W)
    k, _ = softmax_weights(xd.reshape(-1, C, H, W), p[0], p[1], p[2])
    xr = np.stack([np.roll(xd[b], n - int(np.argmax(k[b, 0])), axis=1) for b in range(xd.shape[0])])
    return (_repeat(np.ascontiguousarray(xr).reshape(-1, C, H, W), B), *p)


def build(case, shape, seed=None):
    """The inputs of a named case: normal, flat, sharp8, sharp32, offset, ramp_up, ramp_down, background, background@<n>, peak@<n>."""
    shape = tuple(int(v) for v in shape)
    if seed is None:
        seed = {"background": SEED_BACKGROUND, "offset": SEED_OFFSET}.get(case.split("@")[0], SEED)
    if case.startswith("background@"):
        return case_background(seed, shape, int(case[11:]))
    if case.startswith("peak@"):
        return case_peak(seed, shape, int(case[5:]))
    if case.startswith("sharp"):
        return case_sharp(seed, shape, float(case[5:]))
    if case.startswith("ramp_"):
        return case_ramp(seed, shape, {"up": 1.0, "down": -1.0}[case[5:]])
    return {"normal": case_normal, "flat": case_flat, "offset": case_offset, "background": case_background}[case](seed, shape)


def flat_closed_form(args):
    """The operator on a `flat` case without a softmax: every row of ctx is mean_n v, so out[e][n] = (mean_n v[e]) sum_d q[d][n]."""
    x, g, b, wq, wo, bo = (np.asarray(a, np.float64) for a in args)
    B, C, H, W = x.shape
    qkv = np.matmul(wq.reshape(3 * C, C), _layernorm(x, g, b).reshape(B, C, H * W))
    q, v = qkv[:, :C] * C ** -0.5, qkv[:, 2 * C:]
    out = v.mean(-1)[:, :, None] * q.sum(1)[:, None, :]
    return (np.matmul(wo.reshape(C, C), out) + bo.reshape(1, C, 1)).reshape(B, C, H, W) + x


def background_window_rows(args):
    """Per image: the number of k rows in which more than half of the pixels carry a softmax weight in (1e-8, 6.1e-5) x the row's
    largest -- the window in which a weight relative to a largest weight of 1 is an fp16 subnormal."""
    _, p = softmax_weights(*args[:4])
    r = p / p.max(-1, keepdims=True)
    return (((r > 1e-8) & (r < 6.1e-5)).mean(-1) > 0.5).sum(-1)


# ---- which cases run where ---------------------------------------------------------------------------------------------------------------

BASE_CASES = ("normal", "flat", "sharp8", "sharp32", "offset", "ramp_up", "ramp_down", "background")

# (path, shape (B, C, H, W), environment switches, kernel kinds the planner's labels must show, nsplit the labels must show)
# -- the smallest shapes at which Builder::attention (csrc/cdc_planner.hip) chooses each path
PATHS = (
    ("kvctx16-1tile", (1, 64, 32, 64), {}, ("kvctx", "ctxf"), 64),
    ("kvctx16-1tile", (1, 128, 32, 64), {}, ("kvctx", "ctxf"), 64),
    ("kvctx16-2tiles", (32, 64, 32, 64), {}, ("kvctx", "ctxf"), 32),
    ("kvctx16-4tiles", (2, 64, 128, 128), {}, ("kvctx", "ctxf"), 128),
    ("kvctx16-16tiles", (32, 64, 128, 128), {}, ("kvctx", "ctxf"), 32),    # splits shrink in number with the batch: 512 pixels each here
    ("kvctx-exact", (1, 64, 32, 64), {"CDC_ARITH": "0"}, ("kvctx", "ctxf"), 64),
    ("kvctx-exact", (2, 64, 128, 128), {"CDC_ARITH": "0"}, ("kvctx", "ctxf"), 128),
    ("folded", (1, 192, 64, 64), {}, ("kstats", "ctxp", "ctxf"), 64),
    ("ctx1", (2, 128, 16, 16), {}, ("ctx1",), 1),
    ("ctx1", (1, 384, 8, 8), {}, ("ctx1",), 1),
    ("chain", (2, 128, 16, 16), {"CDC_NO_CTX_ONE": "1"}, ("kstats", "ctxp", "ctxr"), 4),
    ("ragged-C", (1, 24, 12, 20), {}, ("kstats", "ctxp", "ctxr"), 3),     # 24 of a tile's 64 channels, 240 = 3 x 64 + 48 pixels
    ("generic", (1, 24, 9, 13), {}, ("kstats", "ctxp", "ctxr"), 1),       # N % 4 != 0: ctx_partial_generic_kernel
)
PEAK_PATHS = ("kvctx16-2tiles", "kvctx16-4tiles", "folded")
LONG_SPLIT_PATHS = ("kvctx16-16tiles",)          # `background@n` with the feature first in a split


def peak_pixels(shape, nsplit):
    """First and last lane of a 32-pixel tile, a tile seam, a split seam, the end."""
    N = shape[2] * shape[3]
    return (0, 31, 32, N // nsplit - 1, N // nsplit, N - 1)


def first_of_a_split(shape, nsplit):
    """The first pixel of the split that follows pixel N // 3 (where plain `background` has its feature, inside a split)."""
    per = shape[2] * shape[3] // nsplit
    return (shape[2] * shape[3] // 3 // per + 1) * per


def cases_of(path, shape, nsplit):
    return (BASE_CASES + (tuple(f"peak@{n}" for n in peak_pixels(shape, nsplit)) if path in PEAK_PATHS else ())
            + ((f"background@{first_of_a_split(shape, nsplit)}",) if path in LONG_SPLIT_PATHS else ()))


def fixture_entries():
    """Every distinct (case, shape) of PATHS, in a fixed order: the entries of tests/golden/attention_edges.npz."""
    seen, out = set(), []
    for path, shape, _, _, nsplit in PATHS:
        for case in cases_of(path, shape, nsplit):
            if (case, shape) not in seen:
                seen.add((case, shape))
                out.append((case, shape))
    return out


def sample_idx(nsample, size, seed=11):
    """The sampled flat indices of a digest (as tests/helpers.py: digest_idx)."""
    return (synth._splitmix64(np.arange(nsample, dtype=np.uint64) + np.uint64(seed * 1000)) % np.uint64(size)).astype(np.int64)


def entry_key(case, shape):
    return f"{case}|{'x'.join(str(v) for v in shape)}"
