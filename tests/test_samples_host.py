"""K samples per image, the host side: the seed rule, the chunk rule, the argument rules (all raise before any library call) and the
float32 Welford restatement of tests/samples_ref.py against float64."""
import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import samples
from cdc_compression_amd.parallel import expand_seeds, sample_seeds
from samples_ref import mean_var32, mean_var64, welford32


# ---- parallel.sample_seeds ---------------------------------------------------------------------------------------------------------
def test_sample_seeds_of_an_int_seed():
    s = sample_seeds(7, 3, 4)
    assert s == [[7 + b + (k << 32) for k in range(4)] for b in range(3)]
    assert [row[0] for row in s] == expand_seeds(7, 3)                       # sample 0 is today's seeded decode
    flat = [v for row in s for v in row]
    assert len(set(flat)) == 12                                              # no two rows share a key
    assert all(isinstance(v, int) for v in flat)


def test_sample_seeds_of_per_image_seeds_and_of_a_2d_array():
    per = [5, (1 << 50) + 7]
    s = sample_seeds(per, 2, 3)
    assert s == [[v + (k << 32) for k in range(3)] for v in per]
    assert [row[0] for row in s] == expand_seeds(per, 2)
    given = [[1, 2, 3], [2 ** 64 - 1, 0, 9]]
    assert sample_seeds(given, 2, 3) == given
    assert sample_seeds(np.asarray(given, dtype=np.uint64), 2, 3) == given
    assert sample_seeds(np.asarray(per, dtype=np.uint64), 2, 3) == s


def test_sample_seeds_wrap_at_2_to_the_64():
    top = 2 ** 64 - 1
    s = sample_seeds(top, 2, 3)
    assert s[0] == [top, (top + (1 << 32)) % 2 ** 64, (top + (2 << 32)) % 2 ** 64]
    assert s[1] == [0, 1 << 32, 2 << 32]
    assert s[0][1] == (1 << 32) - 1
    hi = sample_seeds([(2 ** 32 - 1) << 32], 1, 2)
    assert hi == [[(2 ** 32 - 1) << 32, 0]]
    assert all(0 <= v < 2 ** 64 for row in s + hi for v in row)


@pytest.mark.parametrize("seed,B,K", [([1, 2], 3, 2), ([[1, 2], [3, 4]], 3, 2), ([[1, 2], [3, 4]], 2, 3), ([[1, 2], [3]], 2, 2),
                                      (1.5, 2, 2), ([1.0, 2.0], 2, 2), ([[1, 2.5]], 1, 2), (True, 1, 2), ("ab", 2, 2), (None, 1, 2),
                                      (-1, 1, 2), (2 ** 64, 1, 2), ([[1, 2 ** 64]], 1, 2), (3, 2, 0), (3, 2, 1.5), (3, 2, True)])
def test_sample_seeds_refuses_bad_shapes_and_non_ints(seed, B, K):
    with pytest.raises(ValueError):
        sample_seeds(seed, B, K)


# ---- the chunk rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,want", [(1, 8, 8), (4, 8, 8), (5, 8, 4), (32, 6, 1), (1, 7, 7), (3, 100, 10), (40, 6, 1)])
def test_default_chunk_is_the_largest_divisor_within_32_rows(B, K, want):
    assert samples.default_chunk(B, K) == want
    plan = samples.chunks(B, K)
    assert plan == [(k0, want) for k0 in range(0, K, want)]


def test_an_explicit_chunk_runs_in_order_and_may_leave_a_short_tail():
    assert samples.chunks(2, 5, 2) == [(0, 2), (2, 2), (4, 1)]
    assert samples.chunks(2, 4, 1) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    assert samples.chunks(2, 4, 9) == [(0, 4)]
    sd = sample_seeds(7, 2, 4)
    np.testing.assert_array_equal(samples.chunk_seeds(sd, 2, 2), np.asarray([sd[0][2], sd[0][3], sd[1][2], sd[1][3]], dtype=np.uint64))


# ---- argument rules: each raises before any library call ----------------------------------------------------------------------------
class _NoLibrary:
    """A denoise_fn / context whose every use is an error: the argument rules must fire first."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached (.{name})")


def _diffs():
    return [cdc.GaussianDiffusionX(_NoLibrary(), None, None, num_timesteps=100, pred_mode="x", var_schedule="cosine"),
            cdc.GaussianDiffusionEps(_NoLibrary(), None, num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")]


@pytest.mark.parametrize("kw", [dict(samples=4, gamma=None, eta=0.5),                                   # no seed
                                dict(samples=4, seed=1, eta=0.5, init=np.zeros((1, 3, 8, 8), np.float32)),   # init
                                dict(samples=4, seed=1, gamma=0.8, init=np.zeros((1, 3, 8, 8), np.float32)),
                                dict(samples=4, seed=1),                                                # nothing stochastic
                                dict(samples=4, seed=1, gamma=0.0, eta=0),
                                dict(samples=1, seed=1, gamma=0.8, reduce="mean_var"),
                                dict(samples=4, seed=1, gamma=0.8, reduce="median"),
                                dict(samples=4, seed=1, gamma=0.8, reduce="mean_var", as_uint8=True),
                                dict(samples=0, seed=1, gamma=0.8),
                                dict(samples=2.5, seed=1, gamma=0.8),
                                dict(samples=4, seed=1, gamma=0.8, sample_chunk=0),
                                dict(seed=1, gamma=0.8, reduce="mean"),                                 # reduce without samples
                                dict(seed=1, gamma=0.8, sample_chunk=2)])
def test_decompress_argument_rules_raise_before_any_library_call(kw):
    for diff in _diffs():
        with pytest.raises(ValueError):
            diff.decompress(_NoLibrary(), **kw)


@pytest.mark.parametrize("kw", [dict(samples=4, gamma=0.8),                                             # no seed
                                dict(samples=4, seed=1),                                                # nothing stochastic
                                dict(samples=4, seed=1, gamma=0.8, metric="mse"),
                                dict(samples=0, seed=1, gamma=0.8),
                                dict(samples=4, seed=1, eta=0.5, sampler="dpmpp_2m", gamma=0.8),
                                dict(samples=4, seed=1, gamma=0.8, sample_chunk=-1)])
def test_compress_best_of_argument_rules_raise_before_any_library_call(kw):
    for diff in _diffs():
        with pytest.raises(ValueError):
            diff.compress_best_of(np.zeros((1, 3, 8, 8), np.float32), **kw)


def test_lpips_without_its_network_and_ms_ssim_below_its_minimum_side_are_refused():
    img = np.zeros((1, 3, 64, 64), np.float32)
    for diff in _diffs():
        assert diff.loss_fn_vgg is None
        with pytest.raises(ValueError, match="lpips"):
            diff.compress_best_of(img, 4, metric="lpips", seed=1, gamma=0.8)
        with pytest.raises(ValueError, match="160"):
            diff.compress_best_of(img, 4, metric="ms_ssim", seed=1, gamma=0.8)


def test_the_selection_rule():
    nan = float("nan")
    assert samples.argbest([1.0, 3.0, 3.0, 2.0], True) == 1                  # a tie goes to the lowest k
    assert samples.argbest([1.0, 3.0, 3.0, 0.5, 0.5], False) == 3
    assert samples.argbest([nan, 2.0, nan, 2.0], True) == 1                  # a NaN never beats a number
    assert samples.argbest([nan, 2.0, nan, 1.0], False) == 3
    assert samples.argbest([nan, nan, nan], True) == 0                       # all NaN: sample 0
    assert samples.argbest([nan, float("-inf")], True) == 1
    assert samples.argbest([float("inf"), float("inf")], True) == 0


# ---- the float32 restatement against float64 -------------------------------------------------------------------------------------------
def _family(name, K, n, rng):
    if name == "normal":
        return rng.standard_normal((K, n))
    if name == "offset":
        return 1.0 + 1e-3 * rng.standard_normal((K, n))
    if name == "clipped":
        return np.clip(rng.standard_normal((K, n)), -1.0, 1.0)
    if name == "identical":
        return np.repeat(rng.standard_normal((1, n)), K, axis=0)
    if name == "mixed":
        return np.where(rng.random((K, n)) < 0.5, 100.0, 1e-3) * rng.standard_normal((K, n))
    assert name == "coin"
    return np.where(rng.random((K, n)) < 0.5, 1.0, -1.0)


@pytest.mark.parametrize("K", [2, 3, 5, 8, 32, 100])
@pytest.mark.parametrize("family", ["normal", "offset", "clipped", "identical", "mixed", "coin"])
def test_welford32_against_float64(family, K):
    """|mean32 - mean64| <= (K + 2) 2^-24 max|x| and |var32 - var64| <= (K + 6) 2^-24 max|x|^2, max|x| per element over the K samples:
    each of the K updates of the mean adds at most about one rounding of a value bounded by max|x|, and the two products and sums
    of the m2 update a few more per sample in units of max|x|^2 / K after the division.  Measured: below 12 and 10.2 of those units
    at K = 100, below 7.3 and 6.1 at K <= 32."""
    rng = np.random.default_rng(1000 * K + len(family))
    x = _family(family, K, 4096, rng).astype(np.float32)
    m32, v32 = mean_var32(x)
    m64, v64 = mean_var64(x)
    amax = np.abs(x.astype(np.float64)).max(axis=0)
    u = 2.0 ** -24
    em = np.abs(m32.astype(np.float64) - m64) / np.maximum(amax, 1e-300)
    ev = np.abs(v32.astype(np.float64) - v64) / np.maximum(amax ** 2, 1e-300)
    print(f"{family} K={K}: mean {em.max() / u:.2f} u (bound {K + 2}), var {ev.max() / u:.2f} u (bound {K + 6})")
    assert (em <= (K + 2) * u).all(), em.max() / u
    assert (ev <= (K + 6) * u).all(), ev.max() / u
    if family == "identical":
        mean, m2 = welford32(x)
        np.testing.assert_array_equal(mean, x[0])
        assert not m2.any()


def test_welford32_does_not_depend_on_the_chunking():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 513)).astype(np.float32)
    whole = welford32(x)
    for cuts in ((3, 4), (1, 1, 1, 1, 1, 1, 1), (6, 1)):
        mean = m2 = None
        k0 = 0
        for c in cuts:
            mean, m2 = welford32(x[k0:k0 + c], k0, mean, m2)
            k0 += c
        np.testing.assert_array_equal(mean, whole[0])
        np.testing.assert_array_equal(m2, whole[1])
