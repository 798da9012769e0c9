"""The rate side on the GPU at the places where one discrete decision or one clamped term hides an error: bpp_kernel and
dequantize_kernel (csrc/aux_kernels.hip), latent_symbols_kernel, hyper_symbols_kernel and scale_bin (csrc/entropy.hip) against the
float64 / integer references of tests/rate_ref.py, whose input conditions tests/test_rate_ref_host.py asserts on the CPU.

The model is the 128 / 128-channel ResnetCompressor of rate_ref.MODEL_KW at hh x wh = 1 x 1 (2 x 3 where the channel stride matters).
For the coder tests every hyper_dec weight is zero, so mean and scale inside cdc_entropy_encode are the last layer's bias: exact
rounding ties against the mean, scales on every one of the 128 bin edges and one float32 step beside them.  Each such test first
asserts that hyper_decode returns those biases bit for bit."""
import functools

import numpy as np
import pytest

import cdc_compression_amd as cdc
import rate_ref as R
from cdc_compression_amd import _lib, synth
from oracle import entropy as oe
from oracle import model as om

pytestmark = pytest.mark.gpu

IMG = (64, 64)               # 4096 pixels: the kernel's 1 / (H W) is a power of two, rate() * H * W gives its float32 sum back exactly


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # (a copy: the shared references are read-only)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _rate_model():
    m = cdc.ResnetCompressor(**R.MODEL_KW)
    assert m.reversed_hyper_dims[0] == R.CH and m.reversed_hyper_dims[-1] // 2 == R.CL
    m.load_hyper_state_dict({**synth.unet_state_dict(R.hyper_manifest(), seed=7), **R.prior_sd()})
    return m


@functools.lru_cache(maxsize=None)
def _class_refs():
    """Inputs of test (a) with both references, computed once and frozen."""
    names, qh, ql, mu, sc = R.class_batch(0)
    sd = R.prior_sd()
    h64, c64 = R.rate_terms_f64(sd, qh, ql, mu, sc)
    h32, c32 = R.rate_terms_f32(sd, qh, ql, mu, sc)
    return (names,) + _frozen(qh, ql, mu, sc, h64, c64, h32, c32)


def _check_rates(what, got_bits, h64, c64, h32, c32):
    """got_bits[b] against the float64 sum of image b.  Tolerance from the references alone: 8 x what the float32 method itself
    loses on this image (sum of |r32 - r64| over its elements) + 4 float32 ulps of the sum (the kernel returns a float32)."""
    worst = []
    for b in range(len(got_bits)):
        ref = float(h64[b].sum() + c64[b].sum())
        own = float(np.abs(h32[b] - h64[b]).sum() + np.abs(c32[b] - c64[b]).sum())
        tol = 8.0 * own + 4.0 * float(np.spacing(np.float32(ref)))
        err = abs(float(got_bits[b]) - ref)
        print(f"[rate] {what[b]}: sum {ref:.6f} bits, error {err:.3g}, float32 method's own loss {own:.3g}, ratio {err / own if own else 0.0:.3g}, "
              f"tolerance {tol:.3g}")
        worst.append((err <= tol, what[b], err, tol))
    assert all(w[0] for w in worst), [w[1:] for w in worst if not w[0]]


def test_bpp_of_every_class_against_float64():
    """(a) cdc_bpp, one image per input class (rate_ref.class_batch) in one batch, against the float64 sum.

    Measured on an MI355X, error / sum |r32 - r64| per class (8 is granted; every run prints the figures):
        gauss/centre 0.12   gauss/typical 0.52   gauss/tail 0.33   gauss/floor 1.0   gauss/wide 0.014   gauss/smin 4.5
        hyper/centre 0.92   hyper/spread 0.45    hyper/far 1.2
    `smin` is the worst because its elements are all alike (s = 0.1, d = 0 or 1), so one element's error adds up a thousand times
    with one sign: an element at d = 1 costs 21.734 bits, the kernel's figure is off by about 1.6e-6 = 0.9 float32 ulp of that, the
    CPU's float32 one happens to land within 3.0e-7.  In `floor` and `far` both sides price the floor and the error is that of
    log2(1e-9f) alone."""
    names, qh, ql, mu, sc, h64, c64, h32, c32 = _class_refs()
    got = _rate_model().rate(qh, ql, mu, sc, IMG)
    assert got.shape == (len(names),) and got.dtype == np.float32
    _check_rates(names, got.astype(np.float64) * (IMG[0] * IMG[1]), h64, c64, h32, c32)


def test_prior_of_a_hyper_element_is_its_channels():
    """(b) hh x wh = 2 x 3: element i of the hyper latent is priced by the prior of channel i / 6.  Every position holds its
    channel's median; image b > 0 moves one whole channel three steps away.  A wrong channel index prices the move -- and the
    medians themselves -- under other priors (rate_ref_host: one symbol's cost differs by bits from channel to channel)."""
    hh, wh = 2, 3
    moved = (0, 1, 21, 42, 63, 64, 85, 126, 127)
    med = R.medians()
    qh = np.broadcast_to(med[None, :, None, None], (1 + len(moved), R.CH, hh, wh)).copy()
    for b, c in enumerate(moved, 1):
        qh[b, c] += np.float32(3.0 if b % 2 else -4.0)
    ql, mu, sc = (np.broadcast_to(a[None], (qh.shape[0],) + a.shape).copy() for a in R.quiet_gauss(hh, wh))
    sd = R.prior_sd()
    h64, c64 = R.rate_terms_f64(sd, qh, ql, mu, sc)
    h32, c32 = R.rate_terms_f32(sd, qh, ql, mu, sc)
    got = _rate_model().rate(qh, ql, mu, sc, IMG).astype(np.float64) * (IMG[0] * IMG[1])
    names = ["medians"] + [f"channel {c} moved" for c in moved]
    _check_rates(names, got, h64, c64, h32, c32)
    # the price of each move on its own: the differences to the first image
    for b, c in enumerate(moved, 1):
        want = float(h64[b].sum() - h64[0].sum())
        own = float(np.abs(h32[b] - h64[b]).sum() + np.abs(h32[0] - h64[0]).sum() + np.abs(c32[b] - c64[b]).sum() + np.abs(c32[0] - c64[0]).sum())
        tol = 8.0 * own + 8.0 * float(np.spacing(np.float32(h64[0].sum())))
        assert abs((got[b] - got[0]) - want) <= tol, (c, got[b] - got[0], want, tol)


def test_batch_rows_of_bpp_are_independent():
    """(c) the batch call of (a) gives the bits of the single-image calls, from host and from device memory."""
    names, qh, ql, mu, sc = _class_refs()[:5]
    m = _rate_model()
    batch = m.rate(qh, ql, mu, sc, IMG)
    batch_dev = m.rate(_dev(qh), _dev(ql), _dev(mu), _dev(sc), IMG).cpu().numpy()
    np.testing.assert_array_equal(_bits(batch), _bits(batch_dev))
    for b, name in enumerate(names):
        one = m.rate(qh[b:b + 1], ql[b:b + 1], mu[b:b + 1], sc[b:b + 1], IMG)
        one_dev = m.rate(_dev(qh[b:b + 1]), _dev(ql[b:b + 1]), _dev(mu[b:b + 1]), _dev(sc[b:b + 1]), IMG).cpu().numpy()
        assert _bits(one)[0] == _bits(batch)[b] and _bits(one_dev)[0] == _bits(batch)[b], name


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1027])
def test_dequantize_rounds_ties_to_even(n):
    """(d) cdc_dequantize on exact ties equals round-half-to-even (torch.round, np.rint) bit for bit, from host and device memory."""
    off = R.tie_offsets(n).reshape(1, n, 1, 1)
    x, _ = R.tie_set(off)
    want = om.dequantize(x, off)
    assert n < 255 or np.count_nonzero(want != (R.round_half_away(x - off) + off).astype(np.float32)) >= n // 4
    m = _rate_model()
    np.testing.assert_array_equal(_bits(m.dequantize(x, off)), _bits(want))
    np.testing.assert_array_equal(_bits(m.dequantize(_dev(x), _dev(off)).cpu().numpy()), _bits(want))


# ---- the coder with mean and scale placed by the biases ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_model(which):
    name, scale_bias, bins = next(s for s in R.edge_scale_sets() if s[0] == which)
    mean_bias = R.tie_offsets(R.CL)
    sd = {**R.zero_weight_hyper_sd(mean_bias, scale_bias), **R.prior_sd(), "prior._medians": R.medians()}
    m = cdc.ResnetCompressor(**R.MODEL_KW)
    m.load_hyper_state_dict(sd)
    return m, oe.raw_prior(sd, R.CH), mean_bias, scale_bias, bins


def _placed(which, B, hh, wh, q_hyper):
    """The model of one scale set with its precondition: hyper_decode gives the biases back bit for bit, whatever q_hyper."""
    m, prior, mean_bias, scale_bias, bins = _edge_model(which)
    mean_e, scale_e = R.expected_mean_scale(mean_bias, scale_bias, B, hh, wh)
    mean, scale = m.hyper_decode(q_hyper)
    np.testing.assert_array_equal(_bits(mean), _bits(mean_e), err_msg="hyper_dec with zero weights does not return its bias (mean)")
    np.testing.assert_array_equal(_bits(scale), _bits(scale_e), err_msg="hyper_dec with zero weights does not return its bias (scale)")
    np.testing.assert_array_equal(R.spec_bins(scale_e[0, :, 0, 0]), bins)
    return m, prior, mean_e, scale_e


def _oracle_stream(prior, med, hh, wh, sym_h, sym_l, scale):
    return oe.stream(1, hh, wh, oe.encode_hyper(sym_h, prior, med), oe.encode_latent(sym_l, scale), oe.model_hash(prior, med),
                     oe.symbol_hash(sym_h, sym_l))


def _encode_and_check(m, prior, latent, hyper, mean_e, scale_e):
    """Streams of the batch == the oracle's on np.rint symbols, byte for byte; decoding returns np.rint(x - off) + off bit for bit."""
    B, _, hh, wh = hyper.shape
    med = R.medians()
    streams = m.latents_to_bytes(latent, hyper)
    assert len(streams) == B
    for b in range(B):
        assert streams[b][:4] == b"CDC\x03" and streams[b][4] == 1, "the encoder left the F16X2 arithmetic"
        sym_h = np.rint(hyper[b] - med[:, None, None]).astype(np.int32)
        sym_l = np.rint(latent[b] - mean_e[b]).astype(np.int32)
        ref = _oracle_stream(prior, med, hh, wh, sym_h, sym_l, scale_e[b])
        assert streams[b] == ref, (b, len(streams[b]), len(ref))
    ql, qh = m.decompress_from_bytes(streams, return_hyper=True)
    np.testing.assert_array_equal(_bits(ql), _bits(om.dequantize(latent, mean_e)))
    np.testing.assert_array_equal(_bits(qh), _bits(om.dequantize(hyper, np.broadcast_to(med[None, :, None, None], hyper.shape))))
    return streams


@pytest.mark.parametrize("which,hh,wh", [("edges", 1, 1), ("edges", 2, 3), ("above", 1, 1), ("below", 1, 1), ("beyond", 1, 1), ("beyond", 2, 3)])
def test_entropy_encode_at_ties_and_bin_edges(which, hh, wh):
    """(e) cdc_entropy_encode on latent ties mean + k + 0.5, hyper ties median + k + 0.5 and the scales of one edge set: the streams are
    the oracle coder's on round-half-to-even symbols and the specification's bins ("smallest i with s <= e_i, 127 beyond")."""
    B = 3
    med = R.medians()
    hyper, _ = R.tie_set(np.broadcast_to(med[None, :, None, None], (B, R.CH, hh, wh)), start=5)
    q_hyper = om.dequantize(hyper, np.broadcast_to(med[None, :, None, None], hyper.shape))
    m, prior, mean_e, scale_e = _placed(which, B, hh, wh, q_hyper)
    latent, k = R.tie_set(mean_e, start=2)
    d = latent - mean_e
    assert np.count_nonzero(np.rint(d) != R.round_half_away(d)) >= d.size // 4
    _encode_and_check(m, prior, latent, hyper, mean_e, scale_e)


def test_escapes_at_the_table_boundaries():
    """(f) symbols +-K, +-(K + 1), +-(K + 2) in the scale tables 0, 17, 64, 100 and 127 (K = min(1023, ceil(8 e_i) + 1): the last in-table
    symbol, the first escape -- payload 0 -- and the second)."""
    med = R.medians()
    hyper = np.broadcast_to(med[None, :, None, None], (2, R.CH, 1, 1)).copy()
    m, prior, mean_e, scale_e = _placed("edges", 2, 1, 1, hyper)
    sym = np.zeros(mean_e.shape, np.int64)
    for c in (0, 17, 64, 100, 127):
        K = R.spec_K(c)
        assert K == oe.gauss_table(c)[0]
        row = np.array([K, -K, K + 1, -(K + 1), K + 2, -(K + 2)])
        sym[0, c].reshape(-1)[:6] = row
        sym[1, c].reshape(-1)[5:11] = -row                         # (the same boundary in other lanes, signs swapped)
    latent = (mean_e.astype(np.float64) + sym).astype(np.float32)
    assert np.array_equal((latent - mean_e).astype(np.int64), sym)
    streams = _encode_and_check(m, prior, latent, hyper, mean_e, scale_e)
    n_esc = [int.from_bytes(s[30:34], "little") for s in streams]
    assert n_esc == [20, 20], n_esc                               # 4 of the 6 symbols of each of the 5 tables


def test_acceptance_limit_of_the_symbol_range():
    """(f) |symbol| < 2.0e9 is coded -- 1999999872, the largest float32 below, round-trips and equals the oracle's stream (its escape
    payload fits the u32 the container holds) -- and 2.0e9, NaN and inf are refused with CdcError, in the latent and in the hyper
    latent, leaving the handle usable."""
    med = R.medians()
    hyper = np.broadcast_to(med[None, :, None, None], (1, R.CH, 1, 1)).copy()
    m, prior, mean_e, scale_e = _placed("edges", 1, 1, 1, hyper)
    assert mean_e[0, 0, 0, 0] == 0.0
    big = np.float32(1999999872.0)
    assert big == np.nextafter(np.float32(2.0e9), np.float32(0)) and float(big) == 1999999872.0
    for v in (big, -big):
        latent = mean_e.copy()
        latent[0, 0, 0, 0] = v
        good = _encode_and_check(m, prior, latent, hyper, mean_e, scale_e)
    for where, v in (("latent", 2.0e9), ("latent", -2.0e9), ("latent", np.nan), ("latent", np.inf), ("hyper", np.inf), ("hyper", -np.inf),
                     ("hyper", 2.0e9)):
        latent, hyp = mean_e.copy(), hyper.copy()
        (latent if where == "latent" else hyp)[0, 0, 0, 0] = np.float32(v)
        with pytest.raises(_lib.CdcError):
            m.latents_to_bytes(latent, hyp)
        latent = mean_e.copy()
        latent[0, 0, 0, 0] = -big
        assert m.latents_to_bytes(latent, hyper) == good, (where, v)      # the handle still codes, and codes the same bytes
