"""Seeded stochastic decode on the MI355X: the generator of csrc/rng.h inside the sampler kernels (cdc_decode_seeded), the fill kernel
behind cdc_randn, and the `seed=` / `gamma=` keywords of decompress / compress.

What ties the new loop to the reference: test_decode_matches_reference_golden pins the stepped cdc_ddim_step chain with recorded
noise to the real reference's ddim(); here the fused loop is that stepped chain bit for bit when the chain is fed the generator's
draws."""
import ctypes
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, synth
from helpers import load_case
from test_gpu_parity import TOL_DEC, make_unet, relerr
from test_rng import randn_host

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)


def _diff(un, tree, **kw):
    if tree == "x":
        return cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode=kw.get("pred_mode", "x"), var_schedule="cosine")
    return cdc.GaussianDiffusionEps(un, None, num_timesteps=20000, clip_noise=kw.get("clip_noise", "none"), pred_mode="noise",
                                    var_schedule="linear")


def _stepped(diff, un, ctx, init, steps, eta, seeds, pred, clip):
    """The chain the fused loop replaces: cdc_ddim_step once per step, its noise = cdc_randn(seeds, draw = i + 1)."""
    L, h = _lib.lib(), un._handle()
    diff.set_sample_schedule(steps)
    B, _, H, W = init.shape
    img = init.copy()
    out = np.empty_like(img)
    ptrs = (ctypes.c_void_p * len(ctx))(*[c.ctypes.data for c in ctx])
    for i in reversed(range(steps)):
        nz = diff.randn(seeds, init.shape, draw=i + 1)
        _lib.check(h, L.cdc_ddim_step(h, img.ctypes.data, i, ptrs, len(ctx), nz.ctypes.data, eta, out.ctypes.data, B, H, W, pred, clip,
                                      _lib.CDC_MEM_HOST, None))
        img = out.copy()
    return img


@pytest.mark.parametrize("where", ["host", "device"])
def test_randn_on_the_device_matches_the_host_evaluation(where):
    """Same header, two libms: the bound of tests/test_rng.py (1e-5) holds between them as well.  16-byte and element-store layouts."""
    un, *_ = make_unet("small_x")
    L, h = _lib.lib(), un._handle()
    worst = 0.0
    for seeds, per, draw, scale in (([1234, (5 << 32) + 1, 2 ** 64 - 1], 3 * 64 * 64, 0, 1.0), ([7], 3 * 37 * 41, 9, 0.8), ([3, 4], 1 << 18, 500, 1.0)):
        sd = np.asarray(seeds, dtype=np.uint64)
        want = randn_host(seeds, per, draw, scale)
        if where == "host":
            got = np.full((len(seeds), per), np.nan, np.float32)
            _lib.check(h, L.cdc_randn(h, sd.ctypes.data_as(U64P), len(seeds), per, draw, scale, got.ctypes.data, _lib.CDC_MEM_HOST, None))
        else:
            import torch
            t = torch.full((len(seeds), per), float("nan"), device="cuda:0")
            _lib.check(h, L.cdc_randn(h, sd.ctypes.data_as(U64P), len(seeds), per, draw, scale, t.data_ptr(), _lib.CDC_MEM_DEVICE,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            got = t.cpu().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    print(f"device against host: max |dz| = {worst:.3e}")
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("name,tree,kw", [("small_x", "x", {}), ("small_eps", "eps", {"clip_noise": "none"}), ("small_eps", "eps", {"clip_noise": "half"}),
                                          ("odd_x", "x", {}), ("small_x", "x", {"pred_mode": "v"})])
def test_fused_loop_is_the_stepped_chain_bit_for_bit(name, tree, kw):
    un, _, sd, x, time, ctx, _ = make_unet(name)
    diff = _diff(un, tree, **kw)
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    steps, eta, seed = 4, 0.5, (3 << 33) + 17
    rec = diff.decompress(ctx, x.shape, sample_steps=steps, init=init, eta=eta, seed=seed)
    assert np.isfinite(rec).all()
    clip = diff._clip_flag(True if tree == "x" else diff.clip_noise)
    want = _stepped(diff, un, ctx, init, steps, eta, seed, diff._pred_flag(), clip)
    np.testing.assert_array_equal(rec, want)
    assert not np.array_equal(rec, diff.decompress(ctx, x.shape, sample_steps=steps, init=init))       # the noise really went in


def test_fused_loop_is_the_stepped_chain_on_a_width_that_is_no_multiple_of_4():
    """odd_x's model on a 24 x 42 frame: the scalar sampler kernel, which evaluates the quad of its element and picks its lane, against the
    16-byte fill kernel's draws (the golden odd_x frame is 40 wide and takes the four-pixel kernel)."""
    kw, man, sd, *_ = load_case("odd_x")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    diff = _diff(un, "x")
    B, H, W, steps = 2, 24, 42, 3
    ctx = synth.context_pyramid([5], B, H, W, seed=3)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    seeds = [8, 2 ** 64 - 1]
    rec = diff.decompress(ctx, (B, 3, H, W), sample_steps=steps, init=init, eta=0.5, seed=seeds)
    want = _stepped(diff, un, ctx, init, steps, 0.5, seeds, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL)
    np.testing.assert_array_equal(rec, want)
    assert not np.array_equal(rec, diff.decompress(ctx, (B, 3, H, W), sample_steps=steps, init=init))


def test_fused_loop_is_the_stepped_chain_full_model_256():
    kw, man, sd, *_ = load_case("full_x")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    diff = _diff(un, "x")
    B, H, W, steps = 2, 256, 256, 4
    ctx = synth.context_pyramid([64, 64, 128, 192], B, H, W, seed=3)
    init = synth.normal("init", (B, 3, H, W), seed=1, std=0.8)
    seeds = [99, 2 ** 40 + 5]
    rec = diff.decompress(ctx, (B, 3, H, W), sample_steps=steps, init=init, eta=0.5, seed=seeds)
    want = _stepped(diff, un, ctx, init, steps, 0.5, seeds, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL)
    np.testing.assert_array_equal(rec, want)


def test_eta_zero_with_a_seed_is_the_unseeded_decode_and_gamma_is_the_filled_init():
    un, _, sd, x, time, ctx, _ = make_unet("small_x")
    diff = _diff(un, "x")
    init = synth.normal("init", x.shape, seed=1, std=0.8)
    np.testing.assert_array_equal(diff.decompress(ctx, x.shape, sample_steps=3, init=init, seed=5), diff.decompress(ctx, x.shape, sample_steps=3, init=init))
    np.testing.assert_array_equal(diff.decompress(ctx, x.shape, sample_steps=3, seed=5), diff.decompress(ctx, x.shape, sample_steps=3))
    start = diff.randn(5, x.shape, draw=0, scale=0.8)
    assert 0.7 < float(start.std()) < 0.9
    np.testing.assert_array_equal(diff.decompress(ctx, x.shape, sample_steps=3, seed=5, gamma=0.8), diff.decompress(ctx, x.shape, sample_steps=3, init=start))
    # gamma and eta together: the stepped chain from the filled start image
    rec = diff.decompress(ctx, x.shape, sample_steps=3, seed=5, gamma=0.8, eta=0.5)
    np.testing.assert_array_equal(rec, _stepped(diff, un, ctx, start, 3, 0.5, 5, _lib.CDC_PRED_X, _lib.CDC_CLIP_ALL))


def test_seeded_decode_repeats_itself_eagerly_and_under_graph_replay(monkeypatch):
    un, kw, sd, x, time, ctx, g = make_unet("full_x")
    diff = _diff(un, "x")
    args = dict(sample_steps=7, eta=0.5, seed=41, gamma=0.8)
    monkeypatch.setenv("CDC_GRAPH", "0")
    eager = diff.decompress(ctx, x.shape, **args)
    np.testing.assert_array_equal(diff.decompress(ctx, x.shape, **args), eager)
    other = diff.decompress(ctx, x.shape, **{**args, "seed": 42})
    assert not np.array_equal(other, eager)
    monkeypatch.setenv("CDC_GRAPH", "1")
    a = diff.decompress(ctx, x.shape, **args)
    b = diff.decompress(ctx, x.shape, **{**args, "seed": 42})          # same captured graph, other seeds
    c = diff.decompress(ctx, x.shape, **{**args, "eta": 0.25})         # other eta -> new capture
    d = diff.decompress(ctx, x.shape, sample_steps=7)                  # the eta = 0 loop after a seeded capture
    monkeypatch.setenv("CDC_GRAPH", "0")
    np.testing.assert_array_equal(a, eager)
    np.testing.assert_array_equal(b, other)
    np.testing.assert_array_equal(c, diff.decompress(ctx, x.shape, **{**args, "eta": 0.25}))
    np.testing.assert_array_equal(d, diff.decompress(ctx, x.shape, sample_steps=7))


def test_rows_of_a_seeded_batch_match_their_batch1_decodes():
    """Launch plans depend on the batch, so this is the project's batch-row bound (TOL_DEC), not bit identity; the draws themselves
    are the same bits in every batch."""
    kw = dict(dim=32, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    un = cdc.Unet(**kw)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = _diff(un, "x")
    B, H, W = 3, 32, 32
    ctx = synth.context_pyramid([8, 32], B, H, W, seed=3)
    seeds = [1234, (1 << 50) + 7, 5]
    rec = diff.decompress(ctx, (B, 3, H, W), sample_steps=4, eta=0.5, seed=seeds, gamma=0.8)
    assert float(np.abs(rec[0] - rec[1]).max()) > 0.05
    for b in range(B):
        r1 = diff.decompress([c[b:b + 1] for c in ctx], (1, 3, H, W), sample_steps=4, eta=0.5, seed=[seeds[b]], gamma=0.8)
        e = relerr(r1[0], rec[b])
        assert e < TOL_DEC, (b, e)


def test_seeded_batch32_256_rows_match_batch1_decodes():
    import torch
    kw, man, sd, *_ = load_case("full_x")
    un = cdc.Unet(**kw)
    un.load_state_dict(sd)
    diff = _diff(un, "x")
    B, S, steps = 32, 256, 6
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(77)
    ctx = [torch.randn((B, c, S >> l, S >> l), generator=gen, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
    rec = diff.decompress(ctx, (B, 3, S, S), sample_steps=steps, eta=0.5, seed=1000, gamma=0.8)
    assert bool(torch.isfinite(rec).all().item())
    assert float((rec[0] - rec[17]).abs().max().item()) > 0.1
    for k in (0, 17, 31):
        r1 = diff.decompress([c[k:k + 1] for c in ctx], (1, 3, S, S), sample_steps=steps, eta=0.5, seed=1000 + k, gamma=0.8)
        e = relerr(r1[0].cpu().numpy(), rec[k].cpu().numpy())
        assert e < TOL_DEC, (k, e)
    assert un.status() == {"arith": 1, "range_faults": 0, "nonfinite_results": 0}


def test_range_guard_repeats_a_seeded_decode_from_its_seeds():
    """The construction of test_fp16_range_overflow_falls_back_to_bf16_planes, decoded seeded: the BF16X3 repetition regenerates the
    start image and the draws, so it equals the same decode on a handle that was in BF16X3 from the start."""
    L = _lib.lib()
    un, kw, sd, x, time, ctx, _ = make_unet("small_eps")
    diff = _diff(un, "eps")
    big = [c * np.float32(3.0e5) for c in ctx]
    args = dict(sample_steps=2, eta=0.5, seed=[(2 ** 63) * (b & 1) + 11 + b for b in range(x.shape[0])], gamma=0.8)
    assert L.cdc_get_arith(un._handle()) == 1
    rec = diff.decompress(big, x.shape, **args)
    assert np.isfinite(rec).all()
    assert L.cdc_get_arith(un._handle()) == 0 and L.cdc_get_range_faults(un._handle()) == 1
    un2, *_ = make_unet("small_eps")
    _lib.check(un2._handle(), L.cdc_set_arith(un2._handle(), 0))
    ref = _diff(un2, "eps").decompress(big, x.shape, **args)
    np.testing.assert_array_equal(rec, ref)


def test_any_size_seeded_compress_and_uint8_output():
    from test_gpu_anysize import _full_x, _images
    diff, un, comp = _full_x()
    u8 = _images()["w500x333"]
    args = dict(sample_steps=3, eta=0.5, seed=7, gamma=0.8)
    rec, bpp = diff.compress(u8, bpp_return_mean=False, **args)
    assert rec.shape == (1, 3, 500, 333) and np.isfinite(rec).all()
    rec2, _ = diff.compress(u8, bpp_return_mean=False, **args)
    np.testing.assert_array_equal(rec, rec2)
    streams = diff.compress_to_bytes(u8)
    out = diff.decompress(streams, as_uint8=True, **args)
    assert out.dtype == np.uint8 and out.shape == (1, 3, 500, 333)
    np.testing.assert_array_equal(out, diff.decompress(streams, as_uint8=True, **args))
    assert not np.array_equal(out, diff.decompress(streams, as_uint8=True, **{**args, "seed": 8}))


def test_torch_gpu_tensors_leave_the_torch_generators_alone():
    import torch
    un, _, sd, x, time, ctx, _ = make_unet("small_x")
    diff = _diff(un, "x")
    dev = torch.device("cuda:0")
    tctx = [torch.from_numpy(c).to(dev) for c in ctx]
    torch.manual_seed(3)
    cpu_state, gpu_state = torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone()
    rec = diff.decompress(tctx, x.shape, sample_steps=3, eta=0.5, seed=9, gamma=0.8)
    assert rec.is_cuda and tuple(rec.shape) == tuple(x.shape)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    np.testing.assert_array_equal(rec.cpu().numpy(), diff.decompress(ctx, x.shape, sample_steps=3, eta=0.5, seed=9, gamma=0.8))
    noise = diff.randn(9, x.shape, draw=2, like=rec)
    assert noise.is_cuda
    np.testing.assert_array_equal(noise.cpu().numpy(), diff.randn(9, x.shape, draw=2))


def test_example_script_device_seed_gives_image_k_the_seed_n_plus_k(tmp_path):
    """examples/test_xparam.py --device_seed N: the k-th image of the folder is what compress(seed=N + k, gamma=--gamma) returns, whatever
    --seed (torch's generator) says; the folder holds the same picture twice, so the two outputs differ by their seeds alone."""
    import subprocess
    import sys
    Image = pytest.importorskip("PIL.Image")
    from test_gpu_anysize import _full_x, _images
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    u8 = _images()["w500x333"][:, :, :100, :70].copy()
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for name in ("a.png", "b.png"):
        Image.fromarray(u8[0].transpose(1, 2, 0)).save(src / name)
    outs = []
    for torch_seed in ("1", "2"):
        d = dst / torch_seed
        r = subprocess.run([sys.executable, os.path.join(root, "examples", "test_xparam.py"), "--ckpt", "synthetic", "--lpips_weight", "0.0",
                            "--n_denoise_step", "3", "--img_dir", str(src), "--out_dir", str(d), "--seed", torch_seed, "--device_seed", "40",
                            "--gamma", "0.7"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append([np.asarray(Image.open(d / n).convert("RGB")).transpose(2, 0, 1) for n in ("a.png", "b.png")])
    for k in range(2):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert not np.array_equal(outs[0][0], outs[0][1])
    diff, un, comp = _full_x()
    for k in range(2):
        rec, _ = diff.compress(u8, sample_steps=3, seed=40 + k, gamma=0.7)
        want = cdc.frame.crop(un._handle(), rec, 100, 70, un.device_index, as_uint8=True)
        np.testing.assert_array_equal(outs[0][k], want[0])
