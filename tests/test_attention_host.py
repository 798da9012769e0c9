"""The float64 restatement of the attention operator (tests/attention_ref.py) without a GPU: against the real reference's float64 run
(tests/golden/attention_edges.npz, written by tests/golden/make_golden_attention.py) on every case and shape that
tests/test_gpu_attention_edges.py runs, and the conditions under which those cases test what they say."""
import functools
import os

import numpy as np
import pytest

import attention_ref as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_edges.npz")
SHAPES = sorted({shape for _, shape, _, _, _ in A.PATHS})


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def _shape_id(shape):
    return "x".join(str(v) for v in shape)


def test_the_fixture_holds_every_case_of_every_path_and_nothing_else():
    g = _golden()
    want = {A.entry_key(c, s) for c, s in A.fixture_entries()}
    assert {k.rsplit("/", 1)[0] for k in g if "|" in k} == want
    assert len(want) == 99 and int(g["nsample"]) == 1024
    for path, shape, _, _, nsplit in A.PATHS:                          # the pixels that `peak` visits sit where the docstrings say
        N, per = shape[2] * shape[3], shape[2] * shape[3] // nsplit
        assert N % nsplit == 0 or path in ("ragged-C", "generic")
        if path in A.PEAK_PATHS:
            assert per % 32 == 0 and per >= 64 and A.peak_pixels(shape, nsplit) == (0, 31, 32, per - 1, per, N - 1)
        if path in A.LONG_SPLIT_PATHS:                                   # many tiles per split, the feature first in one of them
            n = A.first_of_a_split(shape, nsplit)
            assert per >= 512 and n % per == 0 and (N // 3) % per != 0 and f"background@{n}" in A.cases_of(path, shape, nsplit)
    assert os.path.getsize(GOLDEN) < 1000000


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_restatement_equals_the_reference_in_float64(shape):
    """1e-12 relative on every stored digest; the inputs are regenerated and their checksum compared first."""
    g = _golden()
    idx = g[f"idx/{_shape_id(shape)}"].astype(np.int64)
    assert np.array_equal(idx, A.sample_idx(int(g["nsample"]), int(np.prod(shape))))
    for case in [c for c, s in A.fixture_entries() if s == shape]:
        key = A.entry_key(case, shape)
        args = A.build(case, shape)
        assert np.array_equal(A.checksum(args), g[f"{key}/sha"]), f"{key}: the builder gives other inputs on this host"
        y = A.reference(args)
        amax = float(g[f"{key}/amax"])
        assert y.shape == shape and y.dtype == np.float64
        assert np.abs(y.reshape(-1)[idx] - g[f"{key}/val"]).max() <= 1e-12 * max(1.0, amax), key
        assert abs(float(np.abs(y).max()) - amax) <= 1e-12 * max(1.0, amax), key
        assert abs(float(y.sum(dtype=np.float64)) - float(g[f"{key}/sum"])) <= 1e-12 * max(1.0, amax) * y.size, key
        assert amax < 1000.0, key                                       # no case leaves the fp16 range of the plane operands


def test_float32_evaluation_of_the_reference_stays_below_1e_5():
    """e32, the reference's own float32 run against its float64 run: the GPU test grants the kernels max(5e-6, 3 e32), so every
    bound stays at or below 3e-5, inside the project's 1e-4."""
    g = _golden()
    e32 = {k[:-4]: float(g[k]) for k in g if k.endswith("/e32")}
    assert len(e32) == 99 and max(e32.values()) <= 1e-5, max(e32.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_flat_case_is_the_mean_of_v(shape):
    args = A.build("flat", shape)
    y, ctx, v = A.linear_attention(*args, parts=True)
    assert np.abs(ctx - v.mean(-1)[:, None, :]).max() <= 1e-13 * np.abs(v).max()
    assert A.relerr(A.flat_closed_form(args), y) <= 1e-13


BACKGROUNDS = sorted({(c, s) for c, s in A.fixture_entries() if c.startswith("background")})


@pytest.mark.parametrize("case,shape", BACKGROUNDS, ids=lambda v: v if isinstance(v, str) else _shape_id(v))
def test_background_case_fills_the_fp16_subnormal_window(case, shape):
    """At least 8 rows of every image have more than half of their pixels at a softmax weight in (1e-8, 6.1e-5) x the row's largest."""
    args = A.build(case, shape)
    rows = A.background_window_rows([a[:A.DISTINCT] if i == 0 else a for i, a in enumerate(args)])
    assert rows.shape == (min(shape[0], A.DISTINCT),) and rows.min() >= 8, rows


def test_cases_are_what_their_names_say():
    shape = (2, 64, 32, 64)
    N = shape[2] * shape[3]
    x, g, b, wq, wo, bo = A.build("normal", shape)
    pmax = A.softmax_weights(x, g, b, wq)[1].max(-1)
    assert 0.003 < pmax.min() and pmax.max() < 0.9                      # mild bumps
    assert np.median(A.softmax_weights(*A.build("sharp32", shape)[:4])[1].max(-1)) > 0.9          # near one-hot
    k = A.softmax_weights(*A.build("sharp8", shape)[:4])[0]
    assert (k.max(-1) - k.min(-1)).max() > 100.0
    k = A.softmax_weights(*A.build("offset", shape)[:4])[0]
    assert np.abs(k.mean(-1)).max() > 10.0 and np.median(np.abs(k.mean(-1))) > 3.0
    # the ramps: k sweeps hundreds of units along the pixel axis, so in every 32-row block some row's running maximum rises in (nearly)
    # every 32-pixel tile -- the rescale branch of the online softmax -- while other rows never rise after their first tile;
    # ramp_down is the exact mirror image (the rows that rise in one fall in the other)
    def raised(case):
        k = A.softmax_weights(*A.build(case, shape)[:4])[0]
        tm = k.reshape(2, 2, 32, N // 32, 32).max(-1)
        return k, tm[..., 1:] > np.maximum.accumulate(tm, axis=-1)[..., :-1]
    k_up, r_up = raised("ramp_up")
    k_down, r_down = raised("ramp_down")
    assert np.array_equal(k_down, -k_up) and k_up.max() - k_up.min() > 300.0
    for r in (r_up, r_down):
        assert r.any(2).mean() >= 0.8 and (~r.any(-1)).sum() >= 8
    for n in (0, 31, 32, 63, 64, N - 1):
        args = A.build(f"peak@{n}", shape)
        assert (A.softmax_weights(*args[:4])[0][:, 0].argmax(-1) == n).all()
    a5, a32 = A.build("background", (5, 64, 32, 64)), A.build("background", (32, 64, 32, 64))
    assert np.array_equal(a5[0][4], a5[0][0]) and np.array_equal(a32[0][:4], a5[0][:4]) and not np.array_equal(a5[0][0], a5[0][1])
