"""Rate and error maps on the GPU: cdc_rate_map against the float64 sums of the per-symbol terms of tests/rate_ref.py (entry by entry,
with the tolerance rule of tests/test_gpu_rate_edges.py applied per entry), cdc_distortion_map against NumPy's integer sums and the
float64 metric helper restricted to each cell, and both through the model (forward, the streams, evaluate).  The inputs and their
conditions are tests/rd_maps_ref.py, asserted on the CPU by tests/test_rd_maps_host.py."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
import metrics_ref as M
import rate_ref as R
import rd_maps_ref as D
from cdc_compression_amd import _lib, metrics, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IMG = (64, 64)                        # as tests/test_gpu_rate_edges.py: 1 / (H W) is a power of two, rate() * H * W is the kernel's float32 sum
MSE_REL = 10.0 ** 1e-4 - 1.0          # tests/test_gpu_metrics.py grants the float32-operand PSNR 1e-3 dB: this relative error of the MSE
PSNR_DB = 1e-3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                        # (a copy: the shared references are read-only)


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _rate_model():
    m = cdc.ResnetCompressor(**R.MODEL_KW)
    assert m.reversed_hyper_dims[0] == R.CH and m.reversed_hyper_dims[-1] // 2 == R.CL and m.hyper_upsampling == R.UP
    m.load_hyper_state_dict({**synth.unet_state_dict(R.hyper_manifest(), seed=7), **R.prior_sd()})
    return m


def _check_maps(tag, got, ref, own, names=D.MAPS):
    """Every entry of every map against its float64 sum: |error| <= 8 x the float32 method's own loss on the entry's terms + 4 float32
    ulps of the entry.  Prints the worst ratio error / own loss per output."""
    bad = []
    for n in names:
        g = np.asarray(got[n])
        assert g.dtype == np.float32 and g.shape == ref[n].shape, (n, g.dtype, g.shape, ref[n].shape)
        err = np.abs(g.astype(np.float64) - ref[n])
        tol = D.tolerance(ref[n], own[n])
        ratio = np.where(own[n] > 0, err / np.where(own[n] > 0, own[n], 1.0), 0.0)
        k = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        print(f"[rd-maps] {tag} {n}: {g.size} entries, worst error / own loss {float(ratio.max()):.3g} (8 granted), closest to its bound at {k}: "
              f"error {err[k]:.3g}, tolerance {tol[k]:.3g}, entry {ref[n][k]:.6f} bits")
        if not np.all(err <= tol):
            bad.append((n, k, float(err[k]), float(tol[k])))
    assert not bad, bad


# ---- rate maps ------------------------------------------------------------------------------------------------------------------------

def test_maps_of_every_input_class_against_float64():
    """(a) one image per input class at a 1 x 1 hyper latent (fewer positions than a wave): all five outputs, entry by entry.
    The worst ratios error / own loss are printed by every run (8 is granted, plus 4 ulps of the entry, which carry the entries whose
    own loss is next to nothing).  Measured on an MI355X: latent 7.4, hyper 2.0, cell 6.95, latent_channels 8.47, hyper_channels 172;
    the entry closest to its bound is a `latent` entry of a quiet image, off by 4.2e-6 bits of 3.4e-5 granted."""
    names, (qh, ql, mu, sc), ref, own, _ = D.class_case()
    got = _rate_model().rate_map(qh, ql, mu, sc, what=D.MAPS)
    assert sorted(got) == sorted(D.MAPS) and got["latent"].shape == (9, 4, 4) and got["hyper"].shape == (9, 1, 1)
    _check_maps("classes", got, ref, own)


def test_a_moved_symbol_shows_in_its_own_entries_only():
    """(b) 2 x 3 hyper latent, latent 8 x 12: one symbol moved per image.  A latent move raises exactly its entry of `latent` and `cell`
    and its channel of the profile; a hyper move shows in `hyper` at its position, in `cell` on the 4 x 4 block beneath with 1 / 16 of
    the difference each, and leaves `latent` alone.  Everything else keeps the baseline's bits: a transposed or mis-strided index fails."""
    (qh, ql, mu, sc), ref, own, _ = D.geometry_case()
    got = _rate_model().rate_map(qh, ql, mu, sc, what=D.MAPS)
    _check_maps("geometry", got, ref, own)
    base = {n: _bits(got[n][0]) for n in D.MAPS}

    def changed(n, b):
        return np.argwhere(_bits(got[n][b]) != base[n]).tolist()

    def rise(n, b, k, scale=1.0):
        want = (ref[n][(b,) + k] - ref[n][(0,) + k])
        tol = 8.0 * (own[n][(b,) + k] + own[n][(0,) + k]) + 4.0 * (np.spacing(np.float32(ref[n][(b,) + k])) + np.spacing(np.float32(ref[n][(0,) + k])))
        d = float(got[n][(b,) + k]) - float(got[n][(0,) + k])
        assert abs(d - want) <= tol and want >= 1.0 * scale, (n, b, k, d, want, tol)

    for b, ((y, x), c) in enumerate(D.LATENT_MOVES, 1):
        assert changed("latent", b) == [[y, x]] and changed("cell", b) == [[y, x]], (b, changed("latent", b), changed("cell", b))
        assert changed("latent_channels", b) == [[c]] and changed("hyper", b) == [] and changed("hyper_channels", b) == []
        rise("latent", b, (y, x)); rise("cell", b, (y, x)); rise("latent_channels", b, (c,))
    for b, ((y, x), c) in enumerate(D.HYPER_MOVES, 1 + len(D.LATENT_MOVES)):
        block = [[4 * y + i, 4 * x + j] for i in range(4) for j in range(4)]
        assert changed("hyper", b) == [[y, x]] and changed("cell", b) == block, (b, changed("hyper", b), changed("cell", b))
        assert changed("hyper_channels", b) == [[c]] and changed("latent", b) == [] and changed("latent_channels", b) == []
        rise("hyper", b, (y, x)); rise("hyper_channels", b, (c,))
        for k in block:
            rise("cell", b, tuple(k), scale=1.0 / 16.0)


def test_more_positions_than_one_workgroup_against_float64():
    """(c) 5 x 4 hyper latent, latent 20 x 16 = 320 positions, seeded `typical` symbols off the likelihood floor: all five outputs."""
    (qh, ql, mu, sc), ref, own, _ = D.typical_case()
    got = _rate_model().rate_map(qh, ql, mu, sc, what=D.MAPS)
    _check_maps("typical", got, ref, own)
    got_dev = _host(_rate_model().rate_map(_dev(qh), _dev(ql), _dev(mu), _dev(sc), what=D.MAPS))
    for n in D.MAPS:
        assert np.array_equal(_bits(got[n]), _bits(got_dev[n])), n


def test_a_result_depends_on_nothing_but_its_image():
    """(d) image 2 of (c) alone, as row 0 and as row 2 of a batch of three; each output alone and with the others; two runs."""
    (qh, ql, mu, sc), _, _, _ = D.typical_case()
    m = _rate_model()
    full = m.rate_map(qh, ql, mu, sc, what=D.MAPS)
    again = m.rate_map(qh, ql, mu, sc, what=D.MAPS)
    alone = m.rate_map(qh[2:], ql[2:], mu[2:], sc[2:], what=D.MAPS)
    order = [2, 0, 1]
    front = m.rate_map(qh[order], ql[order], mu[order], sc[order], what=D.MAPS)
    for n in D.MAPS:
        assert np.array_equal(_bits(full[n]), _bits(again[n])), n
        assert np.array_equal(_bits(full[n][2]), _bits(alone[n][0])) and np.array_equal(_bits(full[n][2]), _bits(front[n][0])), n
        assert np.array_equal(_bits(full[n][0]), _bits(front[n][1])), n
        one = m.rate_map(qh, ql, mu, sc, what=(n,))
        assert list(one) == [n] and np.array_equal(_bits(one[n]), _bits(full[n])), n
        one_dev = _host(m.rate_map(_dev(qh), _dev(ql), _dev(mu), _dev(sc), what=n))
        assert np.array_equal(_bits(one_dev[n]), _bits(full[n])), n


@pytest.mark.parametrize("case", ["classes", "typical"])
def test_cell_bits_add_up_to_bpp(case):
    """(e) the sum of cell_bits, accumulated in float64, is rate() * H * W within the rule of (a) applied to the whole image; so are the
    sums of the two channel profiles."""
    if case == "classes":
        names, (qh, ql, mu, sc), ref, own, _ = D.class_case()
    else:
        (qh, ql, mu, sc), ref, own, _ = D.typical_case()
        names = [f"typical {b}" for b in range(D.TYPICAL_B)]
    m = _rate_model()
    got = m.rate_map(qh, ql, mu, sc, what=("cell", "latent_channels", "hyper_channels"))
    bits = m.rate(qh, ql, mu, sc, IMG).astype(np.float64) * (IMG[0] * IMG[1])
    total = got["cell"].astype(np.float64).sum(axis=(1, 2))
    profile = got["latent_channels"].astype(np.float64).sum(axis=1) + got["hyper_channels"].astype(np.float64).sum(axis=1)
    for b, name in enumerate(names):
        r = float(ref["cell"][b].sum())
        tol = 8.0 * float(own["cell"][b].sum()) + 4.0 * float(np.spacing(np.float32(r)))
        print(f"[rd-maps] {name}: {r:.6f} bits, cdc_bpp off by {abs(bits[b] - r):.3g}, sum of cell_bits off cdc_bpp by {abs(total[b] - bits[b]):.3g}, "
              f"sum of the profiles by {abs(profile[b] - bits[b]):.3g}, tolerance {tol:.3g}")
        assert abs(total[b] - bits[b]) <= tol and abs(profile[b] - bits[b]) <= tol, (name, total[b], profile[b], bits[b], tol)


def test_rate_map_refusals_touch_nothing():
    """(f) all outputs NULL, B = 0, a missing input, a handle without the prior tensors, and a latent shape that does not belong to the
    hyper latent: the stated error with a message, inputs and output buffers untouched."""
    (qh, ql, mu, sc), _, _, _ = D.geometry_case()
    qh, ql, mu, sc = (np.array(a[:2]) for a in (qh, ql, mu, sc))
    keep = [a.copy() for a in (qh, ql, mu, sc)]
    m, L = _rate_model(), _lib.lib()
    h = m._hyper_handle()
    SENT = np.float32(-12345.0)
    outs = [np.full(s, SENT, np.float32) for s in ((2, 8, 12), (2, 2, 3), (2, 8, 12), (2, R.CL), (2, R.CH))]
    ptr = lambda a: a.ctypes.data      # noqa: E731

    def call(handle, ins=(qh, ql, mu, sc), which=(0, 1, 2, 3, 4), B=2, hh=2, wh=3):
        o = [ptr(outs[i]) if i in which else None for i in range(5)]
        rc = L.cdc_rate_map(handle, *[None if a is None else ptr(a) for a in ins], *o, B, hh, wh, 0, None)
        return rc, (L.cdc_last_error(handle) or b"").decode()

    for kw in (dict(which=()), dict(B=0), dict(B=-1), dict(hh=0), dict(wh=0), dict(ins=(None, ql, mu, sc)), dict(ins=(qh, ql, mu, None))):
        rc, msg = call(h, **kw)
        assert rc == -1 and msg, (kw, rc, msg)
    bare = cdc.ResnetCompressor(**R.MODEL_KW)
    bare.load_hyper_state_dict(synth.unet_state_dict(R.hyper_manifest(), seed=7))          # no prior.* tensors
    rc, msg = call(bare._hyper_handle())
    bpp = np.full(2, SENT, np.float32)
    rc_bpp = L.cdc_bpp(bare._hyper_handle(), ptr(qh), ptr(ql), ptr(mu), ptr(sc), ptr(bpp), 2, 2, 3, 64, 64, 0, None)
    assert rc == -2 and rc == rc_bpp and "prior" in msg and msg == (L.cdc_last_error(bare._hyper_handle()) or b"").decode(), (rc, rc_bpp, msg)
    with pytest.raises(_lib.CdcError):
        bare.rate_map(qh, ql, mu, sc)
    with pytest.raises(_lib.CdcError):
        m.rate_map(qh, ql[:, :, :, :8], mu[:, :, :, :8], sc[:, :, :, :8])
    with pytest.raises(_lib.CdcError):
        m.rate_map(qh, ql, mu, sc[:, :64])
    assert all(np.all(o == SENT) for o in outs) and np.all(bpp == SENT)
    assert all(np.array_equal(_bits(a), _bits(k)) for a, k in zip((qh, ql, mu, sc), keep))
    rc, msg = call(h)                                                                    # and the same buffers are filled by a good call
    assert rc == 0 and not any(np.any(o == SENT) for o in outs)


# ---- error maps -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _unet():
    return cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))


@functools.lru_cache(maxsize=None)
def _byte_case():
    rng = np.random.default_rng(70100)
    a = rng.integers(0, 256, (2, 3, 70, 100), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    d = a.astype(np.int64) - b.astype(np.int64)
    s, n = D.cell_sums(d * d, 16, 5, 7)
    return a, b, s.astype(np.float64) / 65025.0, n


def _framed(win, Hf, Wf, fill):
    f = np.full(win.shape[:2] + (Hf, Wf), fill, win.dtype)
    f[:, :, :win.shape[2], :win.shape[3]] = win
    return f


@pytest.mark.parametrize("where", ["host", "device"])
def test_sse_of_bytes_is_exact(where):
    """(g) two uint8 batches, 70 x 100, cells of 16 on a 5 x 7 grid (partial cells 6 rows high at the bottom, 4 columns wide at the right):
    NumPy's int64 sums / 65025.0 bit for bit; the same bits from float32 operands under as_saved in a 128 x 128 frame of NaN."""
    to = _dev if where == "device" else (lambda t: t)
    a, b, want, count = _byte_case()
    assert count[0, 4, 6] == 3 * 6 * 4 and count[0, 0, 0] == 768 and count.sum() == 2 * 3 * 70 * 100
    m = _unet()
    sse, n = metrics.sse_map(m, to(a), to(b), 16)
    assert sse.dtype == np.float64 and n.dtype == np.int32 and sse.shape == (2, 5, 7) and n.shape == (2, 5, 7)
    assert np.array_equal(_bits(sse), _bits(want)) and np.array_equal(n, count)
    fa, fb = ((v.astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32) for v in (a, b))
    assert np.array_equal(M.saved_u8(fa), a) and np.array_equal(M.saved_u8(fb), b)
    sse_f, n_f = metrics.sse_map(m, to(_framed(fa, 128, 128, np.nan)), to(_framed(fb, 128, 128, np.nan)), 16, size=(70, 100), as_saved=True)
    assert np.array_equal(_bits(sse_f), _bits(want)) and np.array_equal(n_f, count)
    sse_m, _ = metrics.sse_map(m, to(_framed(fa, 128, 128, np.inf)), to(_framed(b, 71, 103, 9)), 16, size=(70, 100), as_saved=(True, False))
    assert np.array_equal(_bits(sse_m), _bits(want))


def test_sse_of_float_operands_against_float64():
    """(h) float32 operands (and a float32 against a uint8 one) per cell against the float64 helper of tests/metrics_ref.py restricted to
    the cell.  The bound is the one tests/test_gpu_metrics.py grants the whole-image float32-operand MSE (1e-3 dB of PSNR, i.e. a
    relative 2.3e-4), applied per cell; sum(sse) / sum(count) gives metrics.psnr within that file's 1e-3 dB.  Measured on an MI355X:
    the worst cell is off by a relative 9.3e-8 (float32 / float32), 1.7e-7 (float32 / uint8), 1.4e-7 (uint8 / float32)."""
    rng = np.random.default_rng(70101)
    a = rng.uniform(-1.3, 1.3, (2, 3, 70, 100)).astype(np.float32)
    b = (a + rng.normal(0, 0.1, a.shape)).astype(np.float32)
    u = M.as_u8(np.clip(M.to_unit(a) + rng.normal(0, 0.05, a.shape), 0, 1))
    m = _unet()
    worst = 0.0
    for x, y in ((a, b), (a, u), (u, b)):
        d = M.to_unit(x) - M.to_unit(y)
        want, count = D.cell_sums(d * d, 16, 5, 7)
        assert np.all(10.0 * np.log10(count / want) <= 45.0)            # every cell in the range that bound is granted for
        sse, n = metrics.sse_map(m, _framed(x, 70, 101, 255 if x.dtype == np.uint8 else np.nan), y, 16, size=(70, 100))
        rel = np.abs(sse - want) / want
        worst = max(worst, float(rel.max()))
        print(f"[rd-maps] sse float {x.dtype} / {y.dtype}: worst cell off by a relative {float(rel.max()):.3g} ({MSE_REL:.3g} granted)")
        assert np.all(rel <= MSE_REL) and np.array_equal(n, count)
        ps = 10.0 * np.log10(n.sum(axis=(1, 2)) / sse.sum(axis=(1, 2)))
        assert np.all(np.abs(ps - metrics.psnr(m, x, y)) <= PSNR_DB) and np.all(np.abs(ps - M.psnr(x, y)) <= PSNR_DB)
        dev = metrics.sse_map(m, _dev(x), _dev(y), 16)
        again = metrics.sse_map(m, x, y, 16)
        assert np.array_equal(_bits(dev[0]), _bits(again[0])) and np.array_equal(_bits(again[0]), _bits(sse))
        one = metrics.sse_map(m, x[1:], y[1:], 16)
        assert np.array_equal(_bits(one[0][0]), _bits(sse[1]))


def test_grid_rules_and_refusals():
    """(i) a grid larger than the window's has exact zero cells with count 0; cell = 1; one cell larger than the image; the refusals."""
    a, b, want, count = _byte_case()
    m = _unet()
    sse, n = metrics.sse_map(m, a, b, 16, grid=(8, 8))
    assert sse.shape == (2, 8, 8) and np.array_equal(_bits(sse[:, :5, :7]), _bits(want)) and np.array_equal(n[:, :5, :7], count)
    outside = np.ones((8, 8), bool)
    outside[:5, :7] = False
    assert np.all(_bits(sse[:, outside]) == 0) and not n[:, outside].any()
    d = a[:, :, :3, :5].astype(np.int64) - b[:, :, :3, :5].astype(np.int64)
    sse1, n1 = metrics.sse_map(m, a, b, 1, size=(3, 5))
    assert sse1.shape == (2, 3, 5) and np.all(n1 == 3) and np.array_equal(_bits(sse1), _bits((d * d).sum(axis=1).astype(np.float64) / 65025.0))
    big, nb = metrics.sse_map(m, a, b, 1000)
    dd = a.astype(np.int64) - b.astype(np.int64)
    assert big.shape == (2, 1, 1) and np.all(nb == 3 * 70 * 100) and np.array_equal(_bits(big[:, 0, 0]), _bits((dd * dd).sum(axis=(1, 2, 3)).astype(np.float64) / 65025.0))

    h, L = m._handle(), _lib.lib()
    f = np.zeros((2, 3, 70, 100), np.float32)
    SENT = -7.0
    out, cnt = np.full((2, 8, 8), SENT, np.float64), np.full((2, 8, 8), -7, np.int32)
    view = lambda t, kind=None, Hf=70, Wf=100, saved=0: _lib.ImageView(t.ctypes.data, (1 if t.dtype == np.uint8 else 0) if kind is None else kind, Hf, Wf, saved)   # noqa: E731

    def call(va, vb, B=2, H=70, W=100, cell=16, gh=5, gw=7, sse=out.ctypes.data, count=cnt.ctypes.data):
        rc = L.cdc_distortion_map(h, ctypes.byref(va), ctypes.byref(vb), B, H, W, cell, gh, gw, sse, count, 0, None)
        return rc, (L.cdc_last_error(h) or b"").decode()

    for kw in (dict(cell=0), dict(cell=-1), dict(gh=4), dict(gw=6), dict(gh=0), dict(H=71), dict(W=101), dict(B=0), dict(sse=None)):
        rc, msg = call(view(f), view(a), **kw)
        assert rc == -1 and msg, (kw, rc, msg)
    for va, vb in ((view(f, kind=2), view(a)), (view(f), view(a, kind=-1)), (view(f), view(a, saved=1)), (view(f, Hf=69), view(a)),
                   (view(f), view(a, Wf=99))):
        rc, msg = call(va, vb)
        assert rc == -1 and msg, (rc, msg)
    assert np.all(out == SENT) and np.all(cnt == -7)
    assert call(view(f), view(a), count=None)[0] == 0 and np.all(cnt == -7)                 # ([2][5][7]: the first 70 doubles of `out`)
    assert not np.any(out.ravel()[:70] == SENT) and np.all(out.ravel()[70:] == SENT)


# ---- through the model ----------------------------------------------------------------------------------------------------------------

def _small(tag):
    """The small models of tests/test_gpu_anysize.py (tests/golden/manifest_anysize_small.json)."""
    meta = json.load(open(os.path.join(GOLDEN, "manifest_anysize_small.json")))[tag]
    un = cdc.Unet(**dict(meta["unet_kwargs"]))
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in meta["unet_manifest"]], seed=0, final_gain=1.0 if tag == "x" else 0.2))
    man = [(k, tuple(v)) for k, v in meta["comp_manifest"]]
    sd = synth.unet_state_dict(man, seed=meta["seed"])
    if tag == "x":
        comp = cdc.ResnetCompressor(**meta["comp_kwargs"])
        comp.load_state_dict(sd)
        return cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine"), {}, sd
    comp = cdc.BigCompressor(**meta["comp_kwargs"])
    comp.load_state_dict(sd)
    return cdc.GaussianDiffusionEps(un, comp, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear"), {"sample_mode": "ddim"}, sd


def _images():
    return M.as_u8(M.picture(2, 70, 100))


def _check_forward_map(comp, sd, images, cond=None):
    """forward(..., return_rate_map=True): shape, its float64 sum against bpp * H * W within the rule of (e), the bits of rate_map() of
    the returned latents, and the same bits from the streams alone."""
    B, _, H, W = images.shape
    kw = {} if cond is None else {"cond": cond}
    out = comp.forward(images, return_rate_map=True, **kw)
    plain = comp.forward(images, **kw)
    assert sorted(plain) == ["bpp", "output", "q_hyper_latent", "q_latent"] and sorted(out) == sorted(list(plain) + ["rate_map"])
    rm = np.asarray(out["rate_map"])
    c = comp.rate_map_cell
    Hp, Wp = comp.padded_size(H, W)
    assert c * comp.hyper_upsampling == comp.frame_multiple and rm.shape == (B, Hp // c, Wp // c) and rm.dtype == np.float32
    mean, scale = comp.hyper_decode(out["q_hyper_latent"], **kw)
    direct = comp.rate_map(out["q_hyper_latent"], out["q_latent"], mean, scale)
    assert list(direct) == ["cell"] and np.array_equal(_bits(direct["cell"]), _bits(rm))
    psd = {k: v for k, v in sd.items() if k.startswith("prior.affine.") or k.startswith("prior.a.")}
    args = [np.asarray(t) for t in (out["q_hyper_latent"], out["q_latent"], mean, scale)]
    h64, c64 = R.rate_terms_f64(psd, *args)
    h32, c32 = R.rate_terms_f32(psd, *args)
    bits = np.asarray(out["bpp"]).astype(np.float64) * (H * W)
    for b in range(B):
        ref = float(h64[b].sum() + c64[b].sum())
        own = float(np.abs(h32[b] - h64[b]).sum() + np.abs(c32[b] - c64[b]).sum())
        tol = 8.0 * own + 4.0 * float(np.spacing(np.float32(ref)))
        total = float(rm[b].astype(np.float64).sum())
        print(f"[rd-maps] forward image {b}: {ref:.4f} bits, sum of the map off bpp * H * W by {abs(total - bits[b]):.3g}, tolerance {tol:.3g}")
        assert abs(total - bits[b]) <= tol, (b, total, bits[b], tol)
    streams = comp.compress_to_bytes(images, **({} if cond is None else {"bitrate_scale": cond}))
    q, from_streams = comp.decompress_from_bytes(streams, return_rate_map=True)
    assert np.array_equal(_bits(q), _bits(np.asarray(out["q_latent"]))) and np.array_equal(_bits(from_streams), _bits(rm))
    assert comp.decompress_from_bytes(streams).shape == q.shape
    return rm


def test_rate_map_through_forward_and_the_streams():
    """(j) the small golden compressor of tests/test_gpu_anysize.py on a 70 x 100 uint8 batch of two.  That model is shallower than
    the published ones: two levels, frame multiple 16, so its cell is 4 pixels and the map of its 80 x 112 frame is [2][20][28]; the
    [2][8][8] map of 16-pixel cells is the next test's, on a model of the published depth."""
    diff, _, sd = _small("x")
    comp = diff.context_fn
    assert comp.frame_multiple == 16 and comp.rate_map_cell == 4 and comp.padded_size(70, 100) == (80, 112)
    rm = _check_forward_map(comp, sd, _images())
    assert rm.shape == (2, 20, 28) and np.all(rm > 0)


@pytest.mark.parametrize("vbr", [False, True])
def test_rate_map_of_a_model_of_the_published_depth(vbr):
    """(j) on the small model of tests/test_gpu_vbr.py (four levels, three hyper layers: frame multiple 64, 16-pixel cells): the map of
    the 128 x 128 frame of a 70 x 100 batch is [2][8][8]; as a variable-bitrate model with two different rates in one batch."""
    meta = json.load(open(os.path.join(GOLDEN, "manifest_vbr_small.json")))
    sd = synth.compressor_state_dict([(k, tuple(v)) for k, v in meta["manifest"]], seed=meta["seed"])
    if not vbr:
        sd = {k: v for k, v in sd.items() if not synth.is_vbr_key(k)}
    comp = cdc.BigCompressor(vbr=vbr, **meta["kwargs"])
    comp.load_state_dict(sd)
    assert comp.frame_multiple == 64 and comp.rate_map_cell == 16
    rm = _check_forward_map(comp, sd, _images(), cond=np.array([0.3, 0.9], np.float32) if vbr else None)
    assert rm.shape == (2, 8, 8)


@pytest.mark.parametrize("tag", ["x", "eps"])
def test_evaluate_with_maps(tag):
    """(k) evaluate(..., maps=True): three maps of one shape, map_cell the context model's cell (4 for these two-level models, whose
    frame multiple is 16; 16 at the published depth, tests/test_rd_maps_host.py), count 0 beyond the window, sum(sse) / sum(count)
    gives the returned psnr; without maps the dict has the keys it had."""
    diff, kw, _ = _small(tag)
    images = _images()
    plain = diff.evaluate(images, sample_steps=2, **kw)
    assert sorted(plain) == ["bpp", "ms_ssim", "psnr", "reconstruction"]
    ev = diff.evaluate(images, sample_steps=2, maps=True, **kw)
    c = diff.context_fn.rate_map_cell
    assert sorted(ev) == sorted(list(plain) + ["map_cell", "rate_map", "sse_count", "sse_map"]) and ev["map_cell"] == c == 4
    Hp, Wp = diff.padded_size(70, 100)
    rm, sse, n = np.asarray(ev["rate_map"]), ev["sse_map"], ev["sse_count"]
    assert (Hp, Wp) == (80, 112) and rm.shape == sse.shape == n.shape == (2, Hp // c, Wp // c)
    assert rm.dtype == np.float32 and sse.dtype == np.float64 and n.dtype == np.int32
    _, want_n = D.cell_sums(np.ones((2, 3, 70, 100), np.int64), c, Hp // c, Wp // c)
    assert np.array_equal(n, want_n) and not n[:, 18:].any() and not n[:, :, 25:].any() and n[:, :17, :25].all() and not sse[n == 0].any()
    assert np.array_equal(_bits(ev["psnr"]), _bits(plain["psnr"])) and np.array_equal(np.asarray(ev["bpp"]), np.asarray(plain["bpp"]))
    ps = 10.0 * np.log10(n.sum(axis=(1, 2)) / sse.sum(axis=(1, 2)))
    assert np.all(np.abs(ps - ev["psnr"]) <= 1e-9), (ps, ev["psnr"])       # two byte operands (as_saved): both sides are exact integers
    bits = np.asarray(ev["bpp"]).astype(np.float64) * (70 * 100)
    # (bpp and every entry are float32 roundings of the same float64 sums, 6e-8 relative each; (j) holds the sum to the rule of (e))
    assert np.all(np.abs(rm.astype(np.float64).sum(axis=(1, 2)) - bits) <= 1e-6 * bits)
    raw = diff.evaluate(images, sample_steps=2, maps=True, as_saved=False, **kw)
    ps = 10.0 * np.log10(raw["sse_count"].sum(axis=(1, 2)) / raw["sse_map"].sum(axis=(1, 2)))
    assert np.all(np.abs(ps - raw["psnr"]) <= PSNR_DB)


def test_example_script_writes_the_maps_when_asked(tmp_path):
    """--maps_dir of the example scripts: the two maps per image as .npy, the cell size printed under bpp; the saved picture, the
    bpp line and the error map agree with each other."""
    import subprocess
    import sys
    Image = pytest.importorskip("PIL.Image")
    src = tmp_path / "in"
    src.mkdir()
    want = M.as_u8(M.picture(1, 70, 100))
    Image.fromarray(want[0].transpose(1, 2, 0)).save(src / "a.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                        "--n_denoise_step", "2", "--img_dir", str(src), "--out_dir", str(tmp_path / "out"), "--maps_dir", str(tmp_path / "maps")],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, CDC_SYNTHETIC_INIT="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[0] == "image: a.png" and lines[1].startswith("bpp:") and lines[2] == "map cell: 16", lines
    rate, sse = np.load(tmp_path / "maps" / "a.rate_map.npy"), np.load(tmp_path / "maps" / "a.sse_map.npy")
    assert rate.shape == sse.shape == (8, 8) and rate.dtype == np.float32 and sse.dtype == np.float64
    import re
    bpp = float(re.search(r"\d+\.\d+(?:[eE][-+]?\d+)?", lines[1]).group(0))            # (printed with four decimals)
    assert abs(float(rate.astype(np.float64).sum()) / (70 * 100) - bpp) <= 1e-4 + 1e-5 * bpp
    got = np.asarray(Image.open(tmp_path / "out" / "a.png").convert("RGB")).transpose(2, 0, 1)[None]
    d = got.astype(np.int64) - want.astype(np.int64)
    ref, _ = D.cell_sums(d * d, 16, 8, 8)
    assert np.array_equal(_bits(sse), _bits(ref[0].astype(np.float64) / 65025.0))
