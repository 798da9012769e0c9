"""References and input builders of the rate-side edge suite (tests/test_rate_ref_host.py pins them on the CPU,
tests/test_gpu_rate_edges.py runs the kernels against them).  No GPU here.

Two statements of the two likelihood terms of Compressor.bpp (compress_modules.py:76-90), per element:
    rate_terms_f64  the float64 restatement of oracle/model.py (the reference the kernels are held to),
    rate_terms_f32  the reference's own float32 method, operation by operation with torch on the CPU; it exists only to
                    measure what that method loses against float64, which is what a float32 kernel is granted.
Input classes as functions of a seed (CLASSES): where the Gaussian term and the FlexiblePrior term are evaluated -- the
centre, the tails, the 1e-9 floor, the widest and the narrowest scale.  Builders of exact rounding ties and of scales on
and beside the 128 bin edges of the entropy coder (csrc/entropy.hip), with the zero-weight hyper_dec whose output is its
last bias, so that mean and scale inside cdc_entropy_encode can be put on any float32 value."""
import numpy as np

from cdc_compression_amd import synth
from oracle import entropy as oe
from oracle import model as om

PD = (1, 3, 3, 3, 1)
FLOOR_BITS = 29.89            # -log2(1e-9) = 29.897...: an element priced above this sits on the likelihood floor

# the tiny 128 / 128-channel model of the suite: reversed_hyper_dims = [128, 128, 128, 256]
MODEL_KW = dict(dim=32, dim_mults=(1, 2, 3, 4), reverse_dim_mults=(4, 3, 2, 1), hyper_dims_mults=(4, 4, 4), channels=3, out_channels=32)
CH = CL = 128
UP = 4                        # latent positions per hyper position and side


# ---- parameters ------------------------------------------------------------------------------------------------------

def prior_sd(C=CH, seed=11):
    """FlexiblePrior parameters under the reference keys.  Affine weights 0.5 N(0, 1) - 0.5: softplus of them stays near
    0.5, so the logits move slowly with x and neither the centre nor N(0, 6) symbols reach the 1e-9 floor (the weights x 2
    of the golden rate fixtures put most elements there, where an error of the chain is clamped away).  Biases and `a`
    as in _prior_sd of tests/test_entropy.py."""
    sd = {}
    for i in range(4):
        sd[f"prior.affine.{i}.weight"] = (0.5 * synth.normal(f"pw{i}", (C, 1, 1, PD[i], PD[i + 1]), seed, 1.0) - 0.5).astype(np.float32)
        sd[f"prior.affine.{i}.bias"] = synth.normal(f"pb{i}", (C, 1, 1, 1, PD[i + 1]), seed, 0.1)
        if i < 3:
            sd[f"prior.a.{i}"] = synth.normal(f"pa{i}", (C, 1, 1, 1, PD[i + 1]), seed, 0.5)
    return sd


def medians(C=CH):
    """Per-channel medians on a dyadic grid: median + k + 0.5 is then exact in float32 for every small integer k."""
    grid = np.array([0.0, 0.25, -1.75, 3.0, -0.5, 1.5], np.float32)
    return grid[np.arange(C) % grid.size].copy()


def hyper_manifest(dims=(CH, 128, 128, 2 * CL)):
    return om.hyper_dec_manifest(list(dims))


def zero_weight_hyper_sd(mean_bias, scale_bias, dims=(CH, 128, 128, 2 * CL), seed=7):
    """hyper_dec with every weight zero: its output is the last layer's bias at every position, whatever the hyper latent,
    so mean[c] = mean_bias[c] and scale[c] = max(scale_bias[c], 0.1).  The biases of the inner layers stay synthetic."""
    man = hyper_manifest(dims)
    sd = synth.unet_state_dict(man, seed=seed)
    for k, _ in man:
        if k.endswith(".weight"):
            sd[k] = np.zeros_like(sd[k])
    last = f"hyper_dec.{len(dims) - 2}.0.bias"
    sd[last] = np.concatenate([np.asarray(mean_bias, np.float32), np.asarray(scale_bias, np.float32)])
    assert sd[last].shape == (dims[-1],)
    return sd


def expected_mean_scale(mean_bias, scale_bias, B, hh, wh):
    """What hyper_decode must return for zero_weight_hyper_sd, bit for bit."""
    shape = (B, len(mean_bias), UP * hh, UP * wh)
    mean = np.broadcast_to(np.asarray(mean_bias, np.float32)[None, :, None, None], shape).copy()
    scale = np.broadcast_to(np.maximum(np.asarray(scale_bias, np.float32), np.float32(0.1))[None, :, None, None], shape).copy()
    return mean, scale


# ---- the two references -----------------------------------------------------------------------------------------------

def rate_terms_f64(sd, q_hyper, q_latent, mean, scale):
    """(hyper_rate, cond_rate) per element in float64: -log2 of oracle/model.py's two likelihoods."""
    return -np.log2(om.flexible_prior_likelihood(sd, q_hyper)), -np.log2(om.normal_likelihood(q_latent, mean, scale))


def rate_terms_f32(sd, q_hyper, q_latent, mean, scale):
    """The same two formulas as the reference evaluates them: float32, one torch operation per reference operation
    (FlexiblePrior.likelihood network_components.py:342-378, NormalDistribution.likelihood utils.py:147-159)."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))       # noqa: E731
    x = t(q_hyper)
    C = x.shape[1]

    def logits(v):
        h = v.permute(1, 0, 2, 3).unsqueeze(-1)                      # [C, B, H, W, 1]
        for i in range(4):
            w = t(sd[f"prior.affine.{i}.weight"]).reshape(C, 1, 1, PD[i], PD[i + 1])
            b = t(sd[f"prior.affine.{i}.bias"]).reshape(C, 1, 1, 1, PD[i + 1])
            h = torch.matmul(h, F.softplus(w)) + b
            if i < 3:
                a = t(sd[f"prior.a.{i}"]).reshape(C, 1, 1, 1, PD[i + 1])
                h = h + torch.tanh(a) * torch.tanh(h)
        return h.squeeze(-1).permute(1, 0, 2, 3)

    lower, upper = logits(x - 0.5), logits(x + 0.5)
    sign = -torch.sign(lower + upper)
    like = torch.abs(torch.sigmoid(upper * sign) - torch.sigmoid(lower * sign)).clamp(min=1e-9)
    hyper_rate = -torch.log2(like)
    d = torch.abs(t(q_latent) - t(mean))
    s = t(scale)
    c = -(2 ** -0.5)
    up = 0.5 * torch.erfc(c * ((0.5 - d) / s))
    lo = 0.5 * torch.erfc(c * ((-0.5 - d) / s))
    cond_rate = -torch.log2((up - lo).clamp(min=1e-9))
    return hyper_rate.numpy().astype(np.float64), cond_rate.numpy().astype(np.float64)


def floor_share(rate64):
    return float(np.count_nonzero(np.asarray(rate64) > FLOOR_BITS)) / float(np.asarray(rate64).size)


# ---- input classes ----------------------------------------------------------------------------------------------------
# every builder returns float32 arrays of one image: a Gaussian class (q_latent, mean, scale) of shape [CL, 4 hh, 4 wh], a
# hyper class q_hyper of shape [CH, hh, wh]

GAUSS_CLASSES = ("centre", "typical", "tail", "floor", "wide", "smin")
HYPER_CLASSES = ("centre", "spread", "far")


def gauss_class(name, seed, hh=1, wh=1, C=CL):
    shape = (C, UP * hh, UP * wh)
    rng = np.random.default_rng([seed, GAUSS_CLASSES.index(name), 1])
    mean = synth.normal(f"rate_mean_{name}", shape, seed, 2.0)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    if name == "centre":
        s, d = np.exp(rng.uniform(np.log(0.1), np.log(2048.0), shape)), np.zeros(shape)
    elif name == "typical":
        s, d = np.full(shape, 3.0), np.rint(rng.standard_normal(shape) * 3.0)
    elif name == "tail":                                             # |d| / s in [4, 6], d an integer
        s = np.exp(rng.uniform(np.log(1.0), np.log(5.0), shape))
        s32 = s.astype(np.float32).astype(np.float64)
        d = np.clip(np.rint(rng.uniform(4.0, 6.0, shape) * s32), np.ceil(4.0 * s32), np.floor(6.0 * s32)) * sign
        s = s32
    elif name == "floor":
        s, d = np.full(shape, 0.5), np.full(shape, 30.0) * sign
    elif name == "wide":
        s = np.exp(rng.uniform(np.log(256.0), np.log(2048.0), shape))      # |d| up to 4000, within 5.2 s: beyond, phi(z) / s < 1e-9
        d = np.rint(rng.uniform(-1.0, 1.0, shape) * np.minimum(4000.0, 5.2 * s))
    elif name == "smin":
        s, d = np.full(shape, np.float32(0.1), np.float64), (rng.random(shape) < 0.5).astype(np.float64) * sign
    else:
        raise KeyError(name)
    scale = s.astype(np.float32)
    if name == "smin":
        mean = np.rint(mean * 4.0).astype(np.float32) / np.float32(4.0)          # (d = 1 stays exactly 1 in float32)
    q_latent = (mean.astype(np.float64) + d).astype(np.float32)
    return q_latent, mean, scale


def quiet_gauss(hh=1, wh=1, C=CL):
    """A latent part that costs next to nothing (d = 0 at s = 0.1: 8e-7 bits an element): the image's rate is its hyper term."""
    shape = (C, UP * hh, UP * wh)
    mean = np.zeros(shape, np.float32)
    return mean.copy(), mean, np.full(shape, 0.1, np.float32)


def hyper_class(name, seed, hh=1, wh=1, C=CH):
    shape = (C, hh, wh)
    rng = np.random.default_rng([seed, HYPER_CLASSES.index(name), 2])
    if name == "centre":
        k = np.rint(rng.standard_normal(shape))
    elif name == "spread":
        k = np.rint(rng.standard_normal(shape) * 6.0)
    elif name == "far":
        k = rng.integers(100, 401, shape) * np.where(rng.random(shape) < 0.5, -1, 1)
    else:
        raise KeyError(name)
    q = medians(C).astype(np.float64)[:, None, None] + k
    q32 = q.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q)                 # median + integer is exact
    return q32


def class_batch(seed=0):
    """The batch of test (a): one image per class at hh x wh = 1 x 1.  A Gaussian class comes with the `centre` hyper class, a
    hyper class with the quiet latent part, so each image's rate is that of its class.  Returns (names, q_hyper, q_latent, mean, scale)."""
    names, qh, ql, mu, sc = [], [], [], [], []
    for g in GAUSS_CLASSES:
        a, b, c = gauss_class(g, seed)
        names.append("gauss/" + g); qh.append(hyper_class("centre", seed)); ql.append(a); mu.append(b); sc.append(c)
    for h in HYPER_CLASSES:
        a, b, c = quiet_gauss()
        names.append("hyper/" + h); qh.append(hyper_class(h, seed)); ql.append(a); mu.append(b); sc.append(c)
    return names, np.stack(qh), np.stack(ql), np.stack(mu), np.stack(sc)


# ---- rounding ties ----------------------------------------------------------------------------------------------------

MEAN_GRID = np.array([0.0, 0.25, -1.75, 3.0, -0.5, 100.5], np.float32)
TIE_K = np.array([0, 1, -1, -2, 2, 3, -3, -4, 6, 7, -7, -8, 12, 13, -13, -14, 37], np.int64)      # 17 values: coprime to 6 and to 16


def tie_offsets(C):
    return MEAN_GRID[np.arange(C) % MEAN_GRID.size].copy()


def tie_set(offset, start=0):
    """x = offset + k + 0.5 elementwise, k running through TIE_K from `start`: exact ties in float32 (asserted).
    Returns (x float32, k int64) of offset's shape."""
    offset = np.asarray(offset, np.float32)
    k = TIE_K[(np.arange(offset.size) + start) % TIE_K.size].reshape(offset.shape)
    x = offset.astype(np.float64) + k + 0.5
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x), "a tie is not representable in float32"
    assert np.array_equal((x32 - offset).astype(np.float64), k + 0.5), "float32 subtraction does not give the tie back"
    return x32, k


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


# ---- scales on and beside the bin edges ----------------------------------------------------------------------------------

def edge_scale_sets():
    """[(name, scale bias [128], expected bin [128])]: every edge e_i itself, its float32 neighbours on both sides for all 128 i
    (0 and 127 included), and the values beyond the table: 4096, 2048 + 1 ulp, biases below 0.1 that the clamp takes to e_0."""
    e = oe.edges()
    i = np.arange(128)
    up = np.nextafter(e, np.float32(np.inf))
    down = np.nextafter(e, np.float32(-np.inf))
    beyond = e.copy()
    want = i.copy()
    for c, (v, b) in enumerate([(4096.0, 127), (0.05, 0), (-1.0, 0), (0.0, 0), (np.float32(0.1), 0), (up[127], 127), (1.0e6, 127), (down[0], 0)]):
        beyond[8 * c + 3] = v
        want[8 * c + 3] = b
    assert np.all(np.maximum(down, np.float32(0.1)) > np.concatenate([[np.float32(0)], e[:-1]])), "an edge's lower neighbour left its bin"
    return [("edges", e.copy(), i.copy()),
            ("above", up.astype(np.float32), np.minimum(i + 1, 127)),
            ("below", down.astype(np.float32), i.copy()),          # (below e_0 = 0.1f the clamp gives e_0 back: bin 0)
            ("beyond", beyond.astype(np.float32), want)]


def spec_bins(scale):
    """Table index by the specification: the smallest i with s <= e_i, 127 beyond."""
    return np.minimum(np.searchsorted(oe.edges(), np.asarray(scale, np.float32), side="left"), 127)


def spec_K(i):
    """Support half-width of scale table i by the specification: min(1023, ceil(8 e_i) + 1)."""
    from math import ceil
    return min(1023, int(ceil(8.0 * float(oe.edges()[i]))) + 1)
