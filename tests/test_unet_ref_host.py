"""The float64 statement of the U-Net's stages (tests/unet_ref.py) without a GPU: against the real reference's float64 run
(tests/golden/unet_edges.npz, written by tests/golden/make_golden_unet_edges.py) on every configuration and case that
tests/test_gpu_unet_edges.py runs, stage() against forward(), and the conditions under which the cases test what they say."""
import functools
import os

import numpy as np
import pytest

import unet_ref as U

GOLDEN = os.path.join(U.GOLDEN, "unet_edges.npz")
ENTRIES = U.entries()


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=2)
def _run(config_name, case):
    args = U.build(case, config_name)
    cfg, sd, x, time, ctx = args
    y, taps = U.forward(sd, cfg, x, time, ctx)
    return args, y, taps


def _id(e):
    return U.entry_key(*e)


def test_the_fixture_holds_every_entry_and_its_worst_bound_stays_inside_the_chain_tolerance():
    g = _golden()
    assert {k.rsplit("/", 1)[0] for k in g if "|" in k} == {U.entry_key(c, s) for c, s in ENTRIES}
    assert int(g["nsample"]) == U.NSAMPLE and os.path.getsize(GOLDEN) < 500000
    worst = 0.0
    for c, s in ENTRIES:
        key, cfg = U.entry_key(c, s), U.config(c)
        assert g[f"{key}/e32"].shape == (len(U.stage_names(cfg)),) and g[f"{key}/val"].shape == (len(U.tap_names(cfg)), U.NSAMPLE)
        worst = max(worst, float(g[f"{key}/e32"].max()), float(g[f"{key}/e32_end"]))
    assert float(g["worst_bound"]) == max(U.OP_BOUND, 3 * worst)
    print(f"[unet-edges] worst bound of any stage of any case: {float(g['worst_bound']):.3g}")
    assert float(g["worst_bound"]) <= U.TOL_DEC


@pytest.mark.parametrize("entry", ENTRIES, ids=_id)
def test_forward_equals_the_reference_in_float64_and_stage_equals_forward(entry):
    """1e-12 relative on every stored digest of every tap (the inputs are regenerated and their checksum compared first); then every
    stage() on the forward's own intermediates gives the forward's tap again, on both wirings of the tail."""
    g, key = _golden(), U.entry_key(*entry)
    args, y, taps = _run(*entry)
    cfg, sd, x, time, ctx = args
    assert np.array_equal(U.checksum(args), g[f"{key}/sha"]), f"{key}: the builder gives other inputs on this host"
    assert y.dtype == np.float64 and y.shape == (x.shape[0], 3, cfg.H, cfg.W)
    for r, k in enumerate(U.tap_names(cfg)):
        v, amax = taps[k], float(g[f"{key}/amax"][r])
        tol = 1e-12 * max(1.0, amax)
        assert np.abs(v.reshape(-1)[U.sample_idx(v.size)] - g[f"{key}/val"][r]).max() <= tol, (key, k)
        assert abs(float(np.abs(v).max()) - amax) <= tol, (key, k)
        assert abs(float(v.sum(dtype=np.float64)) - float(g[f"{key}/sum"][r])) <= tol * v.size, (key, k)
        assert amax < 1000.0, (key, k)                                 # no tap leaves the fp16 range of the plane operands
    lay, _ = cfg.shift_layout()
    for done in (False, True):
        for name, tap, ins in U.wiring(cfg, done):
            inputs = {"x": [taps[i] for i in ins]}
            if name in lay:                                            # a ResnetBlock: its row slice of the shift table, as the GPU test passes it
                off, c = lay[name]
                inputs["shift"] = taps["temb"][:, 0, 0, off:off + c]
            got = U.stage(sd, cfg, name, inputs)
            assert got.shape == taps[tap].shape and U.relerr(got, taps[tap]) <= 1e-12, (key, name)


def test_the_wiring_names_every_stage_once_and_the_shift_table_has_the_library_layout():
    cfg = U.config("full_x")
    names = [s for s, _, _ in U.wiring(cfg)]
    assert len(names) == len(set(names)) == 1 + 4 * 6 - 1 + 3 + 4 * 5 + 1
    assert U.stage_names(cfg)[-2:] == ["ups.4.3+final_conv.0", "final_conv.1"]
    lay, bs = cfg.shift_layout()
    assert list(lay) == cfg.resblocks() and lay["downs.0.0"] == (0, 64) and lay["downs.1.0"] == (128, 128) and bs == int(U.table_mask(cfg).sum())
    lay, bs = U.config("odd_x").shift_layout()                         # 24 and 72 channels: every row padded to 32
    assert lay["downs.0.1"] == (32, 24) and lay["downs.1.0"] == (64, 72) and bs > int(U.table_mask(U.config("odd_x")).sum())


def test_rows_time_ends_and_the_one_sided_cases_are_what_they_say():
    cfg, sd, x, time, ctx = U.build("rows", "full_x")
    assert np.array_equal(x[0], x[2]) and not np.array_equal(x[0], x[1]) and time[0] == time[2] != time[1]
    assert all(np.array_equal(c[0], c[2]) and not np.array_equal(c[0], c[1]) for c in ctx)
    _, y, taps = _run("full_x", "rows")
    assert all(np.array_equal(v[0], v[2]) and not np.array_equal(v[0], v[1]) for k, v in taps.items() if k != "time")
    _, _, _, time, _ = U.build("time_ends", "full_x")
    assert time.reshape(-1).tolist() == [0.0, 1.0, float(np.float32(1.0 / 8193))]
    _, _, _, time, _ = U.build("normal", "full_x")
    assert len(set(time.reshape(-1).tolist())) == 3
    for c in ("full_x", "full_eps"):
        _, _, x, _, ctx = U.build("x_only", c)
        assert all(not v.any() for v in ctx) and x.any()
        _, _, x, _, ctx = U.build("ctx_only", c)
        assert not x.any() and all(v.any() for v in ctx)
    for c, H, W in (("ragged_x", 1, 3), ("odd_x", 12, 20)):            # the coarsest level: narrower than 4 pixels / no multiple of 32
        cfg = U.config(c)
        assert (cfg.H >> (cfg.n - 1), cfg.W >> (cfg.n - 1)) == (H, W)


@pytest.mark.parametrize("config_name", ["full_x", "full_eps", "odd_x"])
def test_offset_reaches_its_ratio_at_every_prenorm_input(config_name):
    args, _, taps = _run(config_name, "offset")
    for p in U.offset_blocks(args[0]):
        v = taps[p]
        ratio = float(np.median(np.abs(v.mean(1)) / v.std(1)))
        print(f"[unet-edges] offset {config_name} {p}: median |mean| / std {ratio:.1f}, max |x| {float(np.abs(v).max()):.1f}, "
              f"attention output max {float(np.abs(taps[U.offset_attention(p)]).max()):.1f}")
        assert ratio >= (U.OFFSET_RATIO_0 if p == "downs.0.1" else U.OFFSET_RATIO), (p, ratio)
        if p.startswith("downs."):
            assert float(taps[p + ".stat_mean"].min()) > 20.0, p        # the statistics taps carry the offset


@pytest.mark.parametrize("config_name", ["full_x", "full_eps", "small_x"])
def test_const_channels_has_variance_zero_and_dead_has_exact_zeros(config_name):
    cfg, sd, x, time, ctx = U.build("const_channels", config_name)
    _, _, taps = _run(config_name, "const_channels")
    blocks = U.const_blocks(cfg)
    assert len(blocks) == (len(U.CONST_BLOCKS) if config_name.startswith("full") else 5)
    lay, _ = cfg.shift_layout()
    for name, tap, ins in U.wiring(cfg):
        if name not in blocks:
            continue
        xin = np.concatenate([taps[i] for i in ins], axis=1)
        w = sd[name + ".block1.block.0.weight"]
        v = U._conv(xin, w, sd[name + ".block1.block.0.bias"], 1, w.shape[-1] // 2)
        assert np.array_equal(v, np.full_like(v, U.CONST_C)) and float(v.var(1).max()) == 0.0         # exactly, in float64
        off, c = lay[name]
        shift = taps["temb"][:, 0, 0, off:off + c]
        h1 = U.resnet_block(sd, name, xin, shift, parts=True)[1]
        want = np.maximum(U._f64(sd[name + ".block1.block.1.b"]), 0.0) + shift[:, :, None, None]
        assert np.array_equal(h1, np.broadcast_to(want, h1.shape)), name                             # LN returns b exactly
    cfg, sd, x, time, ctx = U.build("dead", config_name)
    _, y, taps = _run(config_name, "dead")
    assert len(U.dead_blocks(cfg)) >= 3 and np.isfinite(y).all()
    for name, tap, ins in U.wiring(cfg):
        if name not in U.dead_blocks(cfg):
            continue
        xin = np.concatenate([taps[i] for i in ins], axis=1)
        out, h1 = U.resnet_block(sd, name, xin, np.zeros((x.shape[0], sd[name + ".mlp.1.bias"].shape[0])), parts=True)
        assert not h1.any(), name                                                                    # block2 convolves exact zeros
        bias = np.broadcast_to(U._f64(sd[name + ".block2.block.0.bias"]).reshape(1, -1, 1, 1), out.shape)
        res = U._conv(xin, sd[name + ".res_conv.weight"], sd[name + ".res_conv.bias"]) if name + ".res_conv.weight" in sd else xin
        want = U._ln(np.ascontiguousarray(bias), sd[name + ".block2.block.1.g"], sd[name + ".block2.block.1.b"], True) + res
        assert U.relerr(taps[tap], want) <= 1e-12, name                                              # LN(bias)-derived + the residual path
