"""The counter-based normal generator of the seeded stochastic decode (csrc/rng.h; format in include/cdc_hip.h), checked without a
GPU through the library's host exports cdc_philox4x32_10 / cdc_randn_host, plus the Python argument rules of `seed=` / `gamma=`.

The float64 restatement below is written from the format statement alone (Philox4x32-10 from the paper, the uniform and the
Box-Muller step as the header states them) and shares no code with the library."""
import ctypes

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, parallel

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox_ref(c, k):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: c = [c0, c1, c2, c3] (arrays), k = (k0, k1) (ints)."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in c)
    k0, k1 = int(k[0]), int(k[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def randn_ref(seed, per_image, draw, dtype=np.float64):
    """z(seed, draw, e) for e < per_image in `dtype` arithmetic, from the format statement."""
    nq = (per_image + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    zero = np.zeros(nq, dtype=np.uint64)
    w = philox_ref([q, zero + np.uint64(draw), zero, zero], (seed & 0xFFFFFFFF, seed >> 32))
    u = [((x >> np.uint64(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23) for x in w]
    z = np.empty((nq, 4), dtype)
    for p in range(2):
        r = np.sqrt(dtype(-2.0) * np.log(u[2 * p]))
        ang = dtype(2.0 * np.pi) * u[2 * p + 1]
        z[:, 2 * p], z[:, 2 * p + 1] = r * np.cos(ang), r * np.sin(ang)
    return z.reshape(-1)[:per_image]


def randn_host(seeds, per_image, draw=0, scale=1.0):
    sd = np.asarray(seeds, dtype=np.uint64)
    out = np.empty((len(sd), per_image), np.float32)
    rc = _lib.lib().cdc_randn_host(sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(sd), per_image, draw, scale, out.ctypes.data)
    assert rc == 0
    return out


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    """The Random123 known-answer vectors, through the library and through the restatement the other tests lean on."""
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    assert _lib.lib().cdc_philox4x32_10(c, k, o) == 0
    assert tuple(o) == want
    assert tuple(int(v[0]) for v in philox_ref([[x] for x in ctr], key)) == want


@pytest.mark.parametrize("seeds,draw,per_image", [([0], 0, 4096), ([1234, 1235, 99], 1, 1 << 16), ([(7 << 32) + 5, 2 ** 64 - 1], 500, 30001),
                                                  ([2 ** 63 + 12345], 17, 3 * 37 * 41), ([1234], 3, 1 << 20)])
def test_randn_host_against_float64_restatement(seeds, draw, per_image):
    """The words and hence the uniforms are equal; what differs is float32 rounding of 2 pi u (<= 2 pi 2^-24 in the angle, times
    r <= 5.77: 2.2e-6) and a few ulp of logf / sqrtf / sincosf at |z| <= 5.77 (about 1e-6).  1e-5 is about 4 x the sum."""
    got = randn_host(seeds, per_image, draw)
    worst = 0.0
    for b, s in enumerate(seeds):
        ref = randn_ref(s, per_image, draw)
        assert np.abs(ref).max() <= 5.77
        worst = max(worst, float(np.abs(got[b].astype(np.float64) - ref).max()))
    print(f"max |z32 - z64| = {worst:.3e}")
    assert worst <= 1e-5, worst
    # the scale is one float32 multiplication of the same normal
    np.testing.assert_array_equal(randn_host(seeds, per_image, draw, 0.8), got * np.float32(0.8))


def _corr_z(a, b):
    """z-score of the sample correlation of two standard-normal samples (standard error 1 / sqrt(N))."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.mean(a * b) * np.sqrt(a.size))


def test_randn_distribution_and_independence():
    """2^22 values of seed 1234: moments and the correlations the counter layout could spoil, as z-scores under the null
    (all < 5 in magnitude; the inputs are fixed, so this is deterministic)."""
    N, seed = 1 << 22, 1234
    z = randn_host([seed], N, 0)[0].astype(np.float64)
    scores = {"mean": z.mean() * np.sqrt(N), "variance": (z.var() - 1.0) / np.sqrt(2.0 / N), "fourth moment": (np.mean(z ** 4) - 3.0) / np.sqrt(96.0 / N)}
    quads = z.reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            scores[f"lanes {i},{j}"] = _corr_z(quads[:, i], quads[:, j])
    scores["neighbouring counters"] = _corr_z(quads[:-1].reshape(-1), quads[1:].reshape(-1))
    scores["draws 0,1"] = _corr_z(z, randn_host([seed], N, 1)[0])
    scores["seeds s,s+1"] = _corr_z(z, randn_host([seed + 1], N, 0)[0])
    print({k: round(float(v), 2) for k, v in scores.items()})
    for k, v in scores.items():
        assert abs(v) < 5.0, (k, v)


def test_randn_is_independent_of_the_batch_layout():
    seeds = [1234, (9 << 40) + 3, 77]
    per = 3 * 20 * 24 + 2
    for draw in (0, 5):
        got = randn_host(seeds, per, draw)
        for b, s in enumerate(seeds):
            np.testing.assert_array_equal(got[b], randn_host([s], per, draw)[0])
    assert not np.array_equal(got[0], got[1])


def test_randn_host_refuses_bad_arguments():
    L = _lib.lib()
    sd = np.zeros(1, np.uint64)
    out = np.zeros(4, np.float32)
    p = sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.cdc_randn_host(None, 1, 4, 0, 1.0, out.ctypes.data) == -1
    assert L.cdc_randn_host(p, 0, 4, 0, 1.0, out.ctypes.data) == -1
    assert L.cdc_randn_host(p, 1, 0, 0, 1.0, out.ctypes.data) == -1
    assert L.cdc_randn_host(p, 1, 4, 0, 1.0, None) == -1
    assert L.cdc_philox4x32_10(None, None, None) == -1


def test_expand_and_shard_seeds():
    assert parallel.expand_seeds(5, 3) == [5, 6, 7]
    assert parallel.expand_seeds(2 ** 64 - 1, 3) == [2 ** 64 - 1, 0, 1]                     # (s + b) mod 2^64
    assert parallel.expand_seeds(np.int64(9), 2) == [9, 10]
    assert parallel.expand_seeds(np.array([3, 2 ** 63], dtype=np.uint64), 2) == [3, 2 ** 63]
    for bad in (-1, 2 ** 64, [1, 2], [1, 2, 3, 4], [1, -2, 3], [1, 2 ** 64, 3], [1, 2.5, 3], "abc", 1.5, None, True):
        with pytest.raises(ValueError):
            parallel.expand_seeds(bad, 3)
    for seed in (41, list(range(100, 111))):
        for world in (1, 2, 3, 4, 8, 16):                   # ragged worlds, ranks with an empty shard included
            got = [s for r in range(world) for s in parallel.shard_seeds(seed, 11, world, r)]
            assert got == parallel.expand_seeds(seed, 11)
            for r in range(world):
                lo, hi = parallel.shard_bounds(11, world, r)
                assert len(parallel.shard_seeds(seed, 11, world, r)) == hi - lo


@pytest.mark.parametrize("tree", ["x", "eps"])
def test_seed_and_gamma_argument_rules(tree):
    """Checked before anything reaches the device, so they hold on a machine without one."""
    kw = dict(dim=32, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    un = cdc.Unet(**kw)
    if tree == "x":
        diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    else:
        diff = cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear")
    B, H, W = 2, 32, 32
    ctx = [np.zeros((B, 8, H, W), np.float32), np.zeros((B, 16, H // 2, W // 2), np.float32)]
    init = np.zeros((B, 3, H, W), np.float32)
    images = np.zeros((B, 3, H, W), np.float32)
    for kwargs in (dict(gamma=0.8), dict(gamma=0.8, seed=1, init=init), dict(seed=[1]), dict(seed=[1, 2, 3]), dict(seed=-1),
                   dict(seed=2 ** 64), dict(seed=[1, 2 ** 64]), dict(seed=[1, -1]), dict(seed=1.5)):
        with pytest.raises(ValueError):
            diff.decompress(ctx, (B, 3, H, W), sample_steps=2, **kwargs)
        with pytest.raises(ValueError):
            diff.compress(images, sample_steps=2, **kwargs)


def test_decode_seeded_refuses_bad_arguments_before_it_needs_a_device():
    un = cdc.Unet(dim=32, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    L, h = _lib.lib(), un._handle()
    sd = np.zeros(2, np.uint64)
    p = sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    tail = (None, 0, None, 2, 32, 32, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL, _lib.CDC_MEM_HOST, None)
    assert L.cdc_decode_seeded(h, None, 0.8, None, 0.5, *tail) == -1 and b"null seeds" in L.cdc_last_error(h)
    assert L.cdc_decode_seeded(h, None, 0.8, p, float("nan"), *tail) == -1 and b"not finite" in L.cdc_last_error(h)
    assert L.cdc_decode_seeded(h, None, float("inf"), p, 0.5, *tail) == -1
    assert L.cdc_decode_seeded(None, None, 0.8, p, 0.5, *tail) == -1
    assert L.cdc_randn(None, p, 2, 16, 0, 1.0, None, 0, None) == -1
