"""Images of any size, the parts that need no GPU: the version-5 / -6 stream header through the handle-free peeks, the padding
rule restated in numpy against the fixtures (so that they are pinned without the reference), and the padded-size rule."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
L = _lib.lib()


def _header(version, rate=None, size=None, hh=3, wh=5, arith=1, tail=512):
    """'C' 'D' 'C' version | arith | 0 | hh u16 | wh u16 | six u32 | [bitrate_scale f32] | [img_h u32 | img_w u32] | sections."""
    body = struct.pack("<3sBBBHHIIIIII", b"CDC", version, arith, 0, hh, wh, 256, 256, 0x1234, 0, 0, 0)
    assert len(body) == 34
    if rate is not None:
        body += struct.pack("<f", rate)
    if size is not None:
        body += struct.pack("<II", *size)
    return body + bytes(tail)


def _peek(s):
    hh, wh, ar = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.cdc_entropy_peek(s, len(s), ctypes.byref(hh), ctypes.byref(wh), ctypes.byref(ar))
    return rc, hh.value, wh.value, ar.value


def _peek_size(s):
    has, H, W = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.cdc_entropy_peek_image_size(s, len(s), ctypes.byref(has), ctypes.byref(H), ctypes.byref(W))
    return rc, has.value, H.value, W.value


def _peek_rate(s):
    has, r = ctypes.c_int(-1), ctypes.c_float(-1)
    rc = L.cdc_entropy_peek_bitrate_scale(s, len(s), ctypes.byref(has), ctypes.byref(r))
    return rc, has.value, r.value


def test_header_round_trip_of_versions_5_and_6():
    for size in ((500, 333), (1, 1), (10, 10), (2 ** 31 - 1, 7)):
        s = _header(5, size=size)
        assert _peek(s) == (0, 3, 5, 1)
        assert _peek_size(s) == (0, 1) + size
        assert _peek_rate(s)[:2] == (0, 0)                               # a fixed-rate stream: no rate
        for rate in (0.0, 0.37, -2.5):
            s = _header(6, rate=rate, size=size)
            assert _peek(s) == (0, 3, 5, 1)
            assert _peek_size(s) == (0, 1) + size
            rc, has, r = _peek_rate(s)
            assert (rc, has) == (0, 1) and np.float32(r).view(np.uint32) == np.float32(rate).view(np.uint32)
    # versions 3 and 4 hold no size: the image is the coded extent
    assert _peek_size(_header(3))[:2] == (0, 0)
    assert _peek_size(_header(4, rate=0.5))[:2] == (0, 0)
    assert cdc.ResnetCompressor.image_size_of([_header(5, size=(500, 333)), _header(3), _header(6, 0.5, (1, 2))], 64) == \
        [(500, 333), (192, 320), (1, 2)]
    # the layout itself: 42 / 46 header bytes, the size in the last eight of them, little endian
    s = _header(6, rate=1.0, size=(0x01020304, 0x0A0B0C0D), tail=0)
    assert len(s) == 46 and s[38:46] == bytes([4, 3, 2, 1, 0x0D, 0x0C, 0x0B, 0x0A])
    assert len(_header(5, size=(1, 1), tail=0)) == 42


def test_header_refusals():
    for v, kw, n in ((5, dict(size=(9, 9)), 42), (6, dict(rate=0.5, size=(9, 9)), 46)):
        full = _header(v, tail=0, **kw)
        assert len(full) == n and _peek(full)[0] == 0 and _peek_size(full)[0] == 0
        for cut in (n - 1, n - 4, n - 8, 34, 33, 4, 0):                  # a truncated header is no stream, whatever is missing
            assert _peek(full[:cut])[0] == -1 and _peek_size(full[:cut])[0] == -1 and _peek_rate(full[:cut])[0] == -1
        assert _peek_size(b"XDC" + full[3:])[0] == -1
    for v in (0, 1, 2, 7, 8, 255):
        assert _peek(_header(v, rate=0.5, size=(9, 9)))[0] == -1
    # img_h = 0 (or img_w), or a size beyond the int range: no stream, for every peek
    for size in ((0, 9), (9, 0), (0, 0), (2 ** 31, 9), (9, 2 ** 32 - 1)):
        for s in (_header(5, size=size), _header(6, rate=0.5, size=size)):
            assert _peek(s)[0] == -1 and _peek_size(s)[0] == -1 and _peek_rate(s)[0] == -1
    with pytest.raises(_lib.CdcError, match="not a CDC bitstream"):
        cdc.ResnetCompressor.image_size_of([_header(7)], 64)


def test_hyper_decoder_handle_takes_the_image_scale():
    """The hyper-decoder handle is told the pixels per hyper-latent position (its own configuration does not hold the encoder's
    levels); the refusals of sizes that do not pad to the coded extent need a finalized handle: tests/test_gpu_anysize.py."""
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2, 3, 4], reverse_dim_mults=[4, 3, 2, 1], hyper_dims_mults=[4, 4, 4], channels=3, out_channels=8)
    assert comp.frame_multiple == 64
    h = comp._hyper_handle()
    a, b = ctypes.c_int(), ctypes.c_int()
    assert L.cdc_padded_size(h, 500, 333, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (512, 384)
    assert L.cdc_entropy_set_image_scale(h, 0) == -1 and L.cdc_entropy_set_image_scale(h, 64) == 0
    assert L.cdc_entropy_set_image_scale(comp._enc_handle(), 64) == -2              # not a hyper-decoder handle


# ---- the rule, restated in numpy, against what the reference was actually given -----------------------------------------------------

def _digest_idx(nsample, size, seed=11):
    from cdc_compression_amd import synth
    return (synth._splitmix64(np.arange(nsample, dtype=np.uint64) + np.uint64(seed * 1000)) % np.uint64(size)).astype(np.int64)


def _cases():
    out = []
    for f, tags in (("anysize_full_x.npz", ("64x100", "10x10", "256x256")), ("anysize_full_x_500x333.npz", ("500x333",)),
                    ("anysize_small.npz", ("x_10x10", "eps_33x48", "vbr_33x48"))):
        out += [(f, t) for t in tags]
    return out


@pytest.mark.parametrize("fname,tag", _cases())
def test_fixtures_follow_the_padding_rule(fname, tag):
    g = np.load(os.path.join(GOLDEN, fname))
    img = np.load(os.path.join(GOLDEN, "anysize_images.npz"))["w" + tag.split("_")[-1]]
    B, _, H, W = img.shape
    assert (H, W) == tuple(g[f"{tag}_hw"])
    Hp, Wp = (int(v) for v in g[f"{tag}_padded_hw"])
    M = 64 if fname.startswith("anysize_full") else 16
    assert (Hp, Wp) == (-(-H // M) * M, -(-W // M) * M)
    # float(v) / 255 * 2 - 1, each operation in float32, then edge replication at the bottom and the right
    x = ((img.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    xp = np.pad(x, ((0, 0), (0, 0), (0, Hp - H), (0, Wp - W)), mode="edge")
    yy, xx = np.minimum(np.arange(Hp), H - 1), np.minimum(np.arange(Wp), W - 1)
    assert np.array_equal(xp, x[:, :, yy][:, :, :, xx])                   # pixel (y, x) of the frame = pixel (min(y, H-1), min(x, W-1))
    idx = g[f"{tag}_padded_idx"]
    assert np.array_equal(idx, _digest_idx(idx.size, xp.size))
    assert np.array_equal(xp.reshape(-1)[idx].view(np.int32), g[f"{tag}_padded_val"].view(np.int32))
    assert abs(float(xp.astype(np.float64).sum()) - float(g[f"{tag}_padded_sum"])) <= 1e-9 * xp.size
    # the latents are those of the frame; bpp was rescaled to the original pixels, so it is finite and positive
    n = 4 if M == 64 else 2
    assert g[f"{tag}_q_latent"].shape[0] == B and g[f"{tag}_q_latent"].shape[2:] == (Hp >> n, Wp >> n)
    assert g[f"{tag}_bpp"].shape == (B,) and (g[f"{tag}_bpp"] > 0).all()
    assert float(g[f"{tag}_f64_bpp_rel"]) < 1e-6                          # the reference reproduces itself in float64 (no flipped symbol)


def test_saved_image_of_the_fixture_follows_the_uint8_formula():
    """clamp(-1, 1) / 2 + 0.5, * 255 + 0.5, clamp, truncate -- on the sampled pixels of the 65-step reconstruction the digest holds."""
    g = np.load(os.path.join(GOLDEN, "anysize_full_x_500x333.npz"))
    s = np.load(os.path.join(GOLDEN, "anysize_full_x_500x333_saved.npz"))
    u8 = s["500x333_u8_65"]
    assert u8.shape == (1, 3, 500, 333) and u8.dtype == np.uint8
    v = g["500x333_rec65_val"].astype(np.float32)
    t = (np.clip(v, -1, 1) / np.float32(2.0) + np.float32(0.5)).astype(np.float32)
    t = (t * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    assert np.array_equal(np.clip(t, 0, 255).astype(np.uint8), u8.reshape(-1)[g["500x333_rec65_idx"]])
    near = np.unpackbits(s["500x333_near_65"])[: u8.size]
    assert 0 < near.mean() < 0.05                                          # a thin band around the rounding boundaries


# ---- the padded-size rule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_res,n,nh", [(6, 4, 3), (3, 2, 3), (2, 4, 3), (7, 2, 2), (1, 1, 1)])
def test_padded_size_rule(n_res, n, nh):
    un = cdc.Unet(dim=8, channels=3, context_channels=3, dim_mults=tuple(range(1, n_res + 1)), context_dim_mults=(1,))
    comp = cdc.BigCompressor(dim=8, dim_mults=(1,) * n, hyper_dims_mults=(1,) * nh, channels=3, out_channels=3)
    diff = cdc.GaussianDiffusionEps(un, comp, num_timesteps=100, clip_noise="none", pred_mode="noise", var_schedule="linear")
    Mu, Mc = 2 ** (n_res - 1), 2 ** (n + nh - 1)
    M = max(Mu, Mc)                                                        # least common multiple of two powers of two
    assert comp.frame_multiple == Mc
    for H, W in ((1, 1), (10, 10), (500, 333), (64, 100), (256, 256), (M, M + 1), (2 * M - 1, 3 * M)):
        up = lambda v, m: -(-v // m) * m                                   # noqa: E731
        assert comp.padded_size(H, W) == (up(H, Mc), up(W, Mc))
        a, b = ctypes.c_int(), ctypes.c_int()
        assert L.cdc_padded_size(un._handle(), H, W, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (up(H, Mu), up(W, Mu))
        assert diff.padded_size(H, W) == (up(H, M), up(W, M))
    a, b = ctypes.c_int(), ctypes.c_int()
    assert L.cdc_padded_size(un._handle(), 0, 5, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.cdc_padded_size(un._handle(), 5, 5, None, ctypes.byref(b)) == -1


def test_published_configurations_pad_to_64():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_encoder_full_x.json")))
    comp = cdc.ResnetCompressor(**meta["kwargs"])
    un = cdc.Unet(**json.load(open(os.path.join(GOLDEN, "manifest_full_x.json")))["unet_kwargs"])
    diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    assert diff.padded_size(500, 333) == (512, 384) and diff.padded_size(10, 10) == (64, 64) and diff.padded_size(512, 768) == (512, 768)
