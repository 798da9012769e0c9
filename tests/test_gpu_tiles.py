"""Tiled decode on the MI355X: the window gather and the feathered blend of csrc/tile_kernels.hip, the frame-indexed draws of
csrc/sampler_kernels.hip (the framed fill and the third instantiation of the DDIM kernels), and `decompress(tile=, region=)` against
the composition it is defined as, built here from the plain public calls.  Shapes are in units of G, the model's frame multiple; the
frame is 6 G x 5 G.  Nothing here says anything about seams on trained weights: the weights are synthetic."""
import ctypes

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, frame, synth, tiles
import tiles_ref as R
from test_gpu_anysize import _small
from test_gpu_parity import TOL_DEC, make_unet, relerr
from test_tiles_host import FRAMED_CASES

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)
SEED = (3 << 33) + 17


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def X():
    """The small x-param model with its compressor, a 6 G x 5 G image and its latent, streams and plain context."""
    diff, un, comp, _ = _small("x")
    G = diff.padded_size(1, 1)[0]
    H, W = 6 * G, 5 * G
    img = synth.normal("tiles_image", (2, 3, H, W), seed=31, std=0.5).clip(-1, 1).astype(np.float32)
    q = comp(img)["q_latent"]
    return {"diff": diff, "un": un, "comp": comp, "G": G, "H": H, "W": W, "img": img, "q": q, "cell": 1 << len(comp.rev_mults)}


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", ["latent_odd", "pixel_quads"])
def test_gather_is_numpy_slicing(where, case):
    un, *_ = make_unet("small_x")
    h = un._handle()
    if case == "latent_odd":          # the element path: tile width 3, origins at x = 1
        C, Hs, Ws, th, tw, origins = 5, 13, 11, 4, 3, [(0, 1), (2, 1), (9, 8), (5, 0)]
    else:                             # the 16-byte path
        C, Hs, Ws, th, tw, origins = 3, 24, 20, 8, 12, [(0, 0), (3, 8), (16, 4), (7, 8)]
    src = synth.normal("gather_src", (2, C, Hs, Ws), seed=2)
    want = np.stack([src[b, :, y:y + th, x:x + tw] for b in range(2) for (y, x) in origins])
    if where == "host":
        got = tiles.gather(h, src, origins, th, tw, 0)
    else:
        import torch
        got = tiles.gather(h, torch.from_numpy(src).cuda(), origins, th, tw, 0).cpu().numpy()
    assert got.shape == (8, C, th, tw)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    with pytest.raises(_lib.CdcError, match="outside"):
        tiles.gather(h, src, [(0, Ws - tw + 1)], th, tw, 0)
    with pytest.raises(_lib.CdcError, match="outside"):
        tiles.gather(h, src, [(-1, 0)], th, tw, 0)


# ---- 2. the framed fill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", [0, 5])
@pytest.mark.parametrize("case", FRAMED_CASES)
def test_framed_fill_on_the_device_is_the_crop_of_the_full_frame_fill(case, draw):
    """The same device function in both kernels: identity, not a tolerance."""
    C, fh, fw, y0, x0, th, tw = case
    un, *_ = make_unet("small_x")
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    full = diff.randn([SEED], (1, C, fh, fw), draw=draw, scale=0.8)
    got = tiles.randn_framed(un._handle(), [SEED], [(fh, fw, y0, x0)], C, th, tw, 0, draw=draw, scale=0.8)
    np.testing.assert_array_equal(_bits(got[0]), _bits(full[0, :, y0:y0 + th, x0:x0 + tw]))


def test_framed_fill_two_rows_with_their_own_frames_and_seeds_on_device_memory():
    import torch
    un, *_ = make_unet("small_x")
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    seeds, frames = [1234, 2 ** 64 - 1], [(24, 32, 4, 8), (20, 50, 7, 3)]
    got = tiles.randn_framed(un._handle(), seeds, frames, 3, 12, 16, 0, draw=5, like=torch.empty(1, device="cuda:0")).cpu().numpy()
    for b, (fh, fw, y0, x0) in enumerate(frames):
        full = diff.randn([seeds[b]], (1, 3, fh, fw), draw=5)
        np.testing.assert_array_equal(_bits(got[b]), _bits(full[0, :, y0:y0 + 12, x0:x0 + 16]))
    with pytest.raises(_lib.CdcError, match="outside its frame"):
        tiles.randn_framed(un._handle(), [1], [(24, 32, 13, 0)], 3, 12, 16, 0)


# ---- 3. the framed DDIM update at op level -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tree", [("small_x", "x"), ("small_eps", "eps")])
@pytest.mark.parametrize("frames,th,tw", [([(24, 32, 4, 8), (24, 32, 12, 16)], 12, 16),      # the four-pixel traversal
                                          ([(24, 32, 4, 3), (24, 32, 11, 16)], 12, 16),      # x0 = 3: the element traversal
                                          ([(20, 50, 2, 8), (20, 50, 8, 10)], 9, 40),        # frame_w = 50
                                          ([(20, 50, 2, 8), (20, 50, 8, 10)], 9, 13)])       # a row width that is no multiple of 4
def test_framed_ddim_update_is_the_update_fed_the_crop_of_the_full_frame_draw(name, tree, frames, th, tw):
    un, *_ = make_unet(name)
    L, h = _lib.lib(), un._handle()
    if tree == "x":
        diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    else:
        diff = cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise="none", pred_mode="noise", var_schedule="linear")
    steps, i, eta, seeds = 4, 2, 0.7, [SEED, 99]
    diff.set_sample_schedule(steps)
    pred, clip = diff._pred_flag(), diff._clip_flag(True if tree == "x" else "none")
    fx = synth.normal("fx", (2, 3, th, tw), seed=4, std=0.6)
    x = synth.normal("x", (2, 3, th, tw), seed=5, std=0.9)
    noise = np.stack([diff.randn([seeds[b]], (1, 3, fh, fw), draw=i + 1)[0, :, y0:y0 + th, x0:x0 + tw] for b, (fh, fw, y0, x0) in enumerate(frames)])
    noise = np.ascontiguousarray(noise)
    sd = np.asarray(seeds, np.uint64)

    def update(noise_arr, seed_arr):
        out = np.full_like(x, np.nan)
        _lib.check(h, L.cdc_op_ddim_update(h, fx.ctypes.data, x.ctypes.data, None if noise_arr is None else noise_arr.ctypes.data,
                                           None if seed_arr is None else seed_arr.ctypes.data_as(U64P), eta, i, out.ctypes.data, 2, 3, th, tw, pred,
                                           clip, None, None, 0, 0, _lib.CDC_MEM_HOST, None))
        return out

    want = update(noise, None)
    with tiles.noise_frames(h, frames):
        got = update(None, sd)
    plain = update(None, sd)                                        # the frames are cleared again: the row's own tensor indexes the draws
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert not np.array_equal(plain, got)
    with tiles.noise_frames(h, frames[:1]):                         # one frame row for a call of two rows
        with pytest.raises(_lib.CdcError, match="noise frames are set"):
            update(None, sd)
    with tiles.noise_frames(h, [(th, tw + 3, 1, 0)] * 2):           # a window that leaves its frame
        with pytest.raises(_lib.CdcError, match="outside its"):
            update(None, sd)


# ---- 4. blend ----------------------------------------------------------------------------------------------------------------------
def _blend_case(Hf, Wf, tile, overlap, B=2, C=3, seed=7):
    plan = tiles.Plan(Hf, Wf, tile, overlap)
    t = synth.normal("blend_tiles", (B * plan.T, C, plan.th, plan.tw), seed=seed, std=0.7)
    return plan, t


BLENDS = [(6, 5, (4, 4), (1, 1)),       # tile 4 G, overlap G: the last tile shifted back on both axes, a four-tile corner
          (6, 5, (2, 2), (1, 1)),       # tile 2 G, overlap G: five tiles on the 6 G axis (two-way cover by the plan's rule: stride = tile / 2)
          (7, 5, (4, 4), (2, 2)),       # three tiles over one point on the 7 G axis: up to 3 x 2 = 6 terms
          (7, 7, (4, 4), (2, 2))]       # ... on both axes: nine terms, the largest cover the plan allows


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("nh,nw,tile,overlap", BLENDS)
def test_blend_against_float64(where, nh, nw, tile, overlap):
    """The bound is tiles_ref.blend_bound, derived from the operation order and not measured: a pixel under n tiles is off by at most
    (2 n + 6) 2^-24 max|v| -- a weight carries 3 roundings (two divisions, one product), its product with the value a fourth, the n - 1
    additions of each sum one each, the final division one: (n + 3) + (n + 2) + 1.  14 units for the four-tile corner, 24 for the nine
    terms of a three-way cover on both axes (the plan allows no more: at most three tiles cover a point of an axis)."""
    G = 8
    plan, t = _blend_case(nh * G, nw * G, tuple(v * G for v in tile), tuple(v * G for v in overlap))
    un, *_ = make_unet("small_x")
    h = un._handle()
    if where == "host":
        got = tiles.blend(h, t, plan, 2, 0)
    else:
        import torch
        got = tiles.blend(h, torch.from_numpy(t).cuda(), plan, 2, 0).cpu().numpy()
    assert got.shape == (2, 3, plan.Hp, plan.Wp) and got.dtype == np.float32
    vmax, worst, most = float(np.abs(t).max()), 0.0, 0
    for b in range(2):
        ref, den, cnt = R.blend(t[b * plan.T:(b + 1) * plan.T], plan.ys, plan.xs, plan.Hp, plan.Wp, plan.overlap)
        assert den.min() > 0
        err = np.abs(got[b].astype(np.float64) - ref)
        bound = R.blend_bound(cnt, vmax)[None]
        worst, most = max(worst, float((err / bound).max())), max(most, int(cnt.max()))
        assert (err <= bound).all(), (float((err / bound).max()), int(cnt.max()))
    print(f"blend {nh}x{nw} tile {tile} overlap {overlap}: largest cover {most}, worst error / bound {worst:.3f}")
    assert most == {(6, 5, (4, 4)): 4, (6, 5, (2, 2)): 4, (7, 5, (4, 4)): 6, (7, 7, (4, 4)): 9}[(nh, nw, tile)]


def test_blend_one_tile_window_uint8_and_absent_tiles():
    G = 8
    un, *_ = make_unet("small_x")
    h = un._handle()
    # one tile gives the input, bit for bit (negative zeros and the like included)
    one = tiles.Plan(6 * G, 5 * G, (8 * G, 8 * G), (G, G))
    t1 = synth.normal("one_tile", (2, 3, 6 * G, 5 * G), seed=3)
    t1[0, 0, 0, :4] = [-0.0, 0.0, 1e-40, -3.0e38]
    np.testing.assert_array_equal(_bits(tiles.blend(h, t1, one, 2, 0)), _bits(t1))
    # a window is the crop of the full result, bit for bit: on the 16-byte path, and at odd origins and sizes
    plan, t = _blend_case(6 * G, 5 * G, (4 * G, 4 * G), (G, G))
    t *= 1.6                                                            # values beyond [-1, 1]: the uint8 form clamps
    full = tiles.blend(h, t, plan, 2, 0)
    for win in ((2 * G, G, 3 * G, 2 * G), (2 * G - 3, G + 1, 11, 7), (0, 0, 6 * G - 5, 5 * G - 3)):
        y0, x0, hh, ww = win
        np.testing.assert_array_equal(_bits(tiles.blend(h, t, plan, 2, 0, window=win)), _bits(full[:, :, y0:y0 + hh, x0:x0 + ww]))
        # uint8: what frame.crop(as_uint8=True) makes of the float32 blend, exactly
        u = tiles.blend(h, t, plan, 2, 0, window=win, as_uint8=True)
        assert u.dtype == np.uint8
        shifted = np.zeros_like(full)
        shifted[:, :, :hh, :ww] = full[:, :, y0:y0 + hh, x0:x0 + ww]
        np.testing.assert_array_equal(u, frame.crop(h, shifted, hh, ww, 0, as_uint8=True))
    np.testing.assert_array_equal(tiles.blend(h, t, plan, 2, 0, as_uint8=True), frame.crop(h, full, 6 * G, 5 * G, 0, as_uint8=True))
    # only the tiles a window needs: tile 0 alone serves its interior; a window under an absent tile is an error
    inner = (0, 0, G, G)
    only0 = np.ascontiguousarray(np.stack([t[0], t[plan.T]]))
    np.testing.assert_array_equal(_bits(tiles.blend(h, only0, plan, 2, 0, window=inner, present=[0])), _bits(full[:, :, :G, :G]))
    with pytest.raises(_lib.CdcError, match="is absent"):
        tiles.blend(h, only0, plan, 2, 0, window=(0, 0, G, G + 1), present=[0])
    two = np.ascontiguousarray(np.stack([t[0], t[3], t[plan.T], t[plan.T + 3]]))
    with pytest.raises(_lib.CdcError, match="is absent"):
        tiles.blend(h, two, plan, 2, 0, window=(2 * G, G, 4, 4), present=[0, 3])
    with pytest.raises(_lib.CdcError, match="outside the frame"):
        tiles.blend(h, t, plan, 2, 0, window=(0, 0, 6 * G + 1, G))


# ---- 5. one tile is the plain decode -----------------------------------------------------------------------------------------------
def test_one_tile_that_covers_the_frame_is_the_plain_decode(X):
    diff, G = X["diff"], X["G"]
    streams = diff.compress_to_bytes(X["img"])
    for kw in (dict(), dict(seed=SEED, gamma=0.8, eta=0.5)):
        plain = diff.decompress(streams, sample_steps=3, **kw)
        np.testing.assert_array_equal(_bits(diff.decompress(streams, sample_steps=3, tile=8 * G, **kw)), _bits(plain))
    # an image that is not its padded frame, as uint8, and a region of it
    odd = X["img"][:1, :, :6 * G - 3, :5 * G - 5].copy()
    s2 = diff.compress_to_bytes(odd)
    kw = dict(sample_steps=3, seed=SEED, gamma=0.8, eta=0.5)
    plain = diff.decompress(s2, **kw)
    assert plain.shape == odd.shape
    np.testing.assert_array_equal(_bits(diff.decompress(s2, tile=8 * G, tile_overlap=2 * G, **kw)), _bits(plain))
    np.testing.assert_array_equal(diff.decompress(s2, tile=8 * G, as_uint8=True, **kw), diff.decompress(s2, as_uint8=True, **kw))
    win, info = diff.decompress(s2, tile=8 * G, region=(3, 5, 17, 9), **kw)
    np.testing.assert_array_equal(_bits(win), _bits(plain[:, :, 3:20, 5:14]))
    assert info["tiles"] == 1 and info["tiles_decoded"] == 1


# ---- 6. the tiled decode is the stated composition --------------------------------------------------------------------------------
def _compose(X, plan, steps, seed, gamma, eta, rates=None, images=None):
    """Tile by tile from the plain public calls: the NumPy crop of the latent, context_fn.decode, the plain decode of the tile from
    init = gamma x the crop of the full-frame start draw (eta != 0: a cdc_ddim_step chain fed the crops of the full-frame step draws),
    blended by tiles_ref in float64 -> [B, 3, Hp, Wp] float64."""
    diff, comp, un, cell, q = X["diff"], X["comp"], X["un"], X["cell"], X["q"]
    L, h = _lib.lib(), un._handle()
    B = q.shape[0]
    out = []
    for b in (range(B) if images is None else images):
        start = diff.randn([seed + b], (1, 3, plan.Hp, plan.Wp), draw=0, scale=gamma)
        dec = []
        for (y, x) in plan.origins():
            lat = np.ascontiguousarray(q[b:b + 1, :, y // cell:(y + plan.th) // cell, x // cell:(x + plan.tw) // cell])
            ctx = comp.decode(lat) if rates is None else comp.decode(lat, rates[b:b + 1])
            init = np.ascontiguousarray(start[:, :, y:y + plan.th, x:x + plan.tw])
            if eta == 0:
                dec.append(diff.decompress(ctx, (1, 3, plan.th, plan.tw), sample_steps=steps, init=init)[0])
                continue
            diff.set_sample_schedule(steps)
            img, res = init, np.empty_like(init)
            ptrs = (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in ctx])
            for i in reversed(range(steps)):
                nz = np.ascontiguousarray(diff.randn([seed + b], (1, 3, plan.Hp, plan.Wp), draw=i + 1)[:, :, y:y + plan.th, x:x + plan.tw])
                _lib.check(h, L.cdc_ddim_step(h, img.ctypes.data, i, ptrs, len(ctx), nz.ctypes.data, eta, res.ctypes.data, 1, plan.th, plan.tw,
                                              diff._pred_flag(), diff._clip_flag(True), _lib.CDC_MEM_HOST, None))
                img = res.copy()
            dec.append(img[0])
        out.append(R.blend(np.stack(dec), plan.ys, plan.xs, plan.Hp, plan.Wp, plan.overlap)[0])
    return np.stack(out)


def test_tiled_decode_is_the_composition_of_plain_calls(X):
    """Launch plans depend on the rows of a call, so this is the project's batch-row bound TOL_DEC, not bit identity."""
    diff, G = X["diff"], X["G"]
    plan = tiles.Plan(X["H"], X["W"], (4 * G, 4 * G), (G, G))
    assert plan.T == 4
    args = dict(sample_steps=4, seed=SEED, gamma=0.8, tile=4 * G, tile_overlap=G)
    rec = diff.decompress(X["q"], **args)
    assert rec.shape == X["img"].shape and np.isfinite(rec).all()
    want = _compose(X, plan, 4, SEED, 0.8, 0)
    e = relerr(rec, want)
    print(f"tiled decode against the composition: relerr {e:.3e}")
    assert e < TOL_DEC, e
    # the tiles really differ from the whole-frame decode (the U-Net's attention is global), and the noise really went in
    assert relerr(rec, diff.decompress(X["q"], sample_steps=4, seed=SEED, gamma=0.8)) > 1e-3
    assert not np.array_equal(rec, diff.decompress(X["q"], **{**args, "seed": SEED + 1}))
    # chunks of one row and of all eight rows
    e1 = relerr(diff.decompress(X["q"], tile_chunk=1, **args), want)
    e8 = relerr(diff.decompress(X["q"], tile_chunk=8, **args), want)
    print(f"tile_chunk=1: {e1:.3e}; tile_chunk=8: {e8:.3e}")
    assert e1 < TOL_DEC and e8 < TOL_DEC, (e1, e8)
    assert relerr(diff.decompress(X["q"], tile_chunk=1, **args), diff.decompress(X["q"], tile_chunk=8, **args)) < TOL_DEC
    # the streams give the same tiles as their latent
    streams = diff.compress_to_bytes(X["img"])
    np.testing.assert_array_equal(_bits(diff.decompress(streams, **args)), _bits(rec))
    # a caller's full-frame init is gathered per tile: the same start image as gamma makes
    init = np.concatenate([diff.randn([SEED + b], (1, 3, X["H"], X["W"]), draw=0, scale=0.8) for b in range(2)])
    np.testing.assert_array_equal(_bits(diff.decompress(X["q"], sample_steps=4, init=init, tile=4 * G, tile_overlap=G)), _bits(rec))
    # the second-order sampler is allowed
    sol = diff.decompress(X["q"], sampler="dpmpp_2m", **args)
    assert np.isfinite(sol).all() and not np.array_equal(sol, rec)


def test_tiled_stochastic_decode_is_the_stepped_composition_on_two_tiles(X):
    diff, G = X["diff"], X["G"]
    plan = tiles.Plan(X["H"], X["W"], (6 * G, 4 * G), (G, G))
    assert plan.T == 2 and plan.origins() == [(0, 0), (0, G)]
    rec = diff.decompress(X["q"], sample_steps=3, seed=SEED, gamma=0.8, eta=0.5, tile=(6 * G, 4 * G), tile_overlap=G)
    want = _compose(X, plan, 3, SEED, 0.8, 0.5)
    e = relerr(rec, want)
    print(f"tiled eta = 0.5 decode against the stepped composition: relerr {e:.3e}")
    assert e < TOL_DEC, e
    assert relerr(rec, diff.decompress(X["q"], sample_steps=3, seed=SEED, gamma=0.8, tile=(6 * G, 4 * G), tile_overlap=G)) > 1e-3


# ---- 7. region ---------------------------------------------------------------------------------------------------------------------
def test_region_is_the_crop_of_the_tiled_decode_and_decodes_only_its_tiles(X):
    diff, G = X["diff"], X["G"]
    args = dict(sample_steps=3, seed=SEED, gamma=0.8, eta=0.5, tile=4 * G, tile_overlap=G)
    plan = tiles.Plan(X["H"], X["W"], (4 * G, 4 * G), (G, G))
    full = diff.decompress(X["q"], **args)
    for region, want_tiles in (((G // 2, G // 2, G // 4, G // 4), [0]),                      # inside one tile's interior
                               ((2 * G - 3, G - 2, 7, 5), [0, 1, 2, 3])):                   # across the four-tile corner
        assert plan.intersecting(region) == want_tiles
        win, info = diff.decompress(X["q"], region=region, **args)
        y0, x0, h, w = region
        assert win.shape == (2, 3, h, w) and info == {"tiles": 4, "tiles_decoded": len(want_tiles), "region": region}
        e = relerr(win, full[:, :, y0:y0 + h, x0:x0 + w])
        print(f"region {region}: {info['tiles_decoded']} of {info['tiles']} tiles, relerr {e:.3e}")
        assert e < TOL_DEC, (region, e)
        u, _ = diff.decompress(X["q"], region=region, as_uint8=True, **args)
        assert u.dtype == np.uint8 and u.shape == win.shape
    with pytest.raises(ValueError, match="reaches outside"):
        diff.decompress(X["q"], region=(0, X["W"] - 2, 4, 4), **args)
    # compress() and evaluate() pass the arguments through
    rec, bpp = diff.compress(X["img"], bpp_return_mean=False, **args)
    np.testing.assert_array_equal(_bits(rec), _bits(full))
    np.testing.assert_array_equal(bpp, X["comp"](X["img"])["bpp"])
    ev = diff.evaluate(X["img"], **args)
    np.testing.assert_array_equal(_bits(ev["reconstruction"]), _bits(full))
    assert ev["psnr"].shape == (2,) and np.isfinite(ev["psnr"]).all()
    best = diff.compress_best_of(X["img"], 2, seed=SEED, gamma=0.8, eta=0.5, sample_steps=3, tile=4 * G, tile_overlap=G)
    assert best["reconstruction"].shape == X["img"].shape and best["scores"].shape == (2, 2)
    for b in range(2):
        again = diff.decompress(X["q"][b:b + 1], **{**args, "seed": [int(best["seed"][b])]})
        assert relerr(again[0], best["reconstruction"][b]) < TOL_DEC


# ---- 8. variable-bitrate model -----------------------------------------------------------------------------------------------------
def test_vbr_tiles_carry_their_image_rate():
    diff, un, comp, _ = _small("vbr")
    G = diff.padded_size(1, 1)[0]
    H, W = 6 * G, 5 * G
    img = synth.normal("tiles_image", (2, 3, H, W), seed=31, std=0.5).clip(-1, 1).astype(np.float32)
    rates = np.array([0.1, 0.9], np.float32)
    streams = diff.compress_to_bytes(img, bitrate_scale=rates)
    q = comp(img, rates)["q_latent"]
    X = {"diff": diff, "comp": comp, "un": un, "cell": 1 << len(comp.rev_mults), "q": q}
    plan = tiles.Plan(H, W, (4 * G, 4 * G), (G, G))
    args = dict(sample_steps=3, seed=SEED, gamma=0.8, tile=4 * G, tile_overlap=G)
    rec = diff.decompress(streams, **args)                                # each stream carries its own rate
    np.testing.assert_array_equal(_bits(diff.decompress(q, bitrate_scale=rates, **args)), _bits(rec))
    for b in range(2):
        # item 6's composition on one tile per image: tile b + 1 of image b, where no other tile reaches (weight 1)
        t = b + 1
        y, x = plan.origin(t)
        cell = X["cell"]
        lat = np.ascontiguousarray(q[b:b + 1, :, y // cell:(y + plan.th) // cell, x // cell:(x + plan.tw) // cell])
        start = diff.randn([SEED + b], (1, 3, H, W), draw=0, scale=0.8)
        one = diff.decompress(comp.decode(lat, rates[b:b + 1]), (1, 3, plan.th, plan.tw), sample_steps=3,
                              init=np.ascontiguousarray(start[:, :, y:y + plan.th, x:x + plan.tw]))[0]
        ys, xs = (slice(0, G), slice(4 * G, 5 * G)) if t == 1 else (slice(5 * G, 6 * G), slice(0, G))      # corners only this tile covers
        e = relerr(rec[b, :, ys, xs], one[:, ys.start - y:ys.stop - y, xs.start - x:xs.stop - x])
        other = diff.decompress(comp.decode(lat, rates[1 - b:2 - b]), (1, 3, plan.th, plan.tw), sample_steps=3,
                                init=np.ascontiguousarray(start[:, :, y:y + plan.th, x:x + plan.tw]))[0]
        eo = relerr(rec[b, :, ys, xs], other[:, ys.start - y:ys.stop - y, xs.start - x:xs.stop - x])
        print(f"vbr image {b} tile {t}: relerr {e:.3e} at its own rate, {eo:.3e} at the other image's")
        assert e < TOL_DEC and eo > 10 * TOL_DEC, (b, e, eo)


# ---- the defaults run the code they ran --------------------------------------------------------------------------------------------
def test_a_tiled_decode_leaves_no_noise_frames_on_the_handle(X):
    """The frames are set for the sampler calls of a tiled decode only: the plain seeded decode after one equals the one before it,
    bit for bit, also when the tiled decode failed inside a sampler call."""
    import torch
    diff, G = X["diff"], X["G"]
    kw = dict(sample_steps=3, seed=SEED, eta=0.5)
    before = diff.decompress(X["q"], gamma=0.8, **kw)
    diff.decompress(X["q"], tile=4 * G, gamma=0.8, **kw)
    np.testing.assert_array_equal(_bits(diff.decompress(X["q"], gamma=0.8, **kw)), _bits(before))
    with pytest.raises(_lib.CdcError, match="same memory space"):        # a host latent with a device init: refused inside the sampler call
        diff.decompress(X["q"], tile=4 * G, init=torch.zeros(X["img"].shape, device="cuda:0"), **kw)
    np.testing.assert_array_equal(_bits(diff.decompress(X["q"], gamma=0.8, **kw)), _bits(before))
