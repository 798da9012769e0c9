"""LPIPS-VGG without a GPU: the two float64 restatements of tests/lpips_ref.py against each other and against closed forms, the
manifest and the loading rules of LpipsVGG, GaussianDiffusion.load_state_dict with and without "loss_fn_vgg.*" keys, and the
argument rules, which raise before the library is touched.  Computing needs the GPU and says so."""
import functools
import os
import re

import numpy as np
import pytest

import cdc_compression_amd as cdc
import lpips_ref as LR
import metrics_ref as R
from cdc_compression_amd import _lib, lpips, metrics, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (33, 47), (64, 64)]


@functools.lru_cache(maxsize=None)
def _sd():
    return synth.lpips_vgg_state_dict(seed=0)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    p, q = LR.operands(3, H, W)
    a, b = R.as_f32(p), R.as_f32(q)
    return a, b, LR.lpips_torch(_sd(), a, b), LR.lpips_numpy(_sd(), a, b)


# ---- 1. the restatements ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SIZES)
def test_the_two_restatements_agree(H, W):
    _, _, (tot_t, lay_t), (tot_n, lay_n) = _case(H, W)
    assert lay_t.shape == (3, 5) and tot_t.shape == (3,) and np.all(lay_t > 0)
    assert np.abs((lay_t - lay_n) / lay_t).max() <= 1e-12 and np.abs((tot_t - tot_n) / tot_t).max() <= 1e-12
    assert np.array_equal(tot_t, lay_t.sum(1))
    # the recipe: a noisy copy of a smooth picture scores between 3e-4 and 3e-2 (the smallest-noise image is the hard one)
    assert 3e-4 <= tot_t.min() and tot_t.max() <= 3e-2, tot_t


@pytest.mark.parametrize("H,W", SIZES)
def test_float32_arithmetic_sits_inside_the_forward_bound(H, W):
    """Plain float32 convolutions stay a factor of five inside the 1e-5 the GPU test asks of the kernels."""
    a, b, (tot, lay), _ = _case(H, W)
    tot32, lay32 = LR.lpips_torch(_sd(), a, b, dtype="float32")
    assert np.abs((lay32 - lay) / lay).max() <= 2e-6 and np.abs((tot32 - tot) / tot).max() <= 2e-6


def test_identical_operands_give_exactly_zero():
    a = _case(33, 47)[0]
    for fn in (LR.lpips_torch, LR.lpips_numpy):
        tot, lay = fn(_sd(), a, a.copy())
        assert np.all(tot == 0.0) and np.all(lay == 0.0)
    u = R.as_u8(LR.operands(2, 16, 16)[0])
    assert np.all(LR.lpips_numpy(_sd(), u, R.as_f32(u / 255.0), saved_b=True)[0] == 0.0)      # the saved byte IS the byte


def test_the_distance_is_symmetric():
    a, b, _, (tot, lay) = _case(33, 47)
    tot2, lay2 = LR.lpips_numpy(_sd(), b, a)
    assert np.array_equal(tot, tot2) and np.array_equal(lay, lay2)


def test_floor_mode_pooling_by_hand():
    x = np.arange(25, dtype=np.float64).reshape(1, 1, 5, 5)
    x[0, 0, 4, :] = 1000.0          # the last row and the last column are ignored
    x[0, 0, :, 4] = 2000.0
    want = np.array([[6.0, 8.0], [16.0, 18.0]])
    assert np.array_equal(LR.pool_reshape(x)[0, 0], want)
    import torch
    assert np.array_equal(torch.nn.functional.max_pool2d(torch.from_numpy(x), 2, 2).numpy()[0, 0], want)


def test_the_scaling_layer_and_the_operand_mapping():
    shift, scale = np.array(LR.SHIFT), np.array(LR.SCALE)
    u = np.array([0, 128, 255], np.uint8).reshape(1, 3, 1, 1)
    x = LR.net_input(u, False, shift, scale)[0, :, 0, 0]
    assert np.allclose(x, (2 * np.array([0, 128, 255]) / 255.0 - 1 - shift) / scale, rtol=0, atol=1e-15)
    f = np.array([-3.0, 0.0, 0.5], np.float32).reshape(1, 3, 1, 1)                            # clamped to [-1, 1]
    assert np.allclose(LR.net_input(f, False, shift, scale)[0, :, 0, 0], (np.array([-1.0, 0.0, 0.5]) - shift) / scale, rtol=0, atol=1e-15)
    sd = dict(_sd())
    sd["scaling_layer.shift"] = np.zeros((1, 3, 1, 1), np.float32)
    sd["scaling_layer.scale"] = np.ones((1, 3, 1, 1), np.float32)
    a, b = _case(16, 16)[:2]
    assert np.all(LR.lpips_numpy(sd, a, b)[0] != _case(16, 16)[3][0])                         # the state dict's own values are used


# ---- 2. the manifest and the loading rules ---------------------------------------------------------------------------------------------

def test_manifest_names_and_shapes():
    man = cdc.LpipsVGG().manifest()
    assert man == [(n, tuple(s)) for n, s in synth.lpips_vgg_manifest()] and len(man) == 31
    d = dict(man)
    assert d["net.slice1.0.weight"] == (64, 3, 3, 3) and d["net.slice4.17.weight"] == (512, 256, 3, 3) and d["net.slice5.28.bias"] == (512,)
    assert [d[f"lin{k}.model.1.weight"] for k in range(5)] == [(1, c, 1, 1) for c in (64, 128, 256, 512, 512)]
    assert sorted(k for k in d if k.endswith(".weight") and k.startswith("net.")) == sorted(
        f"net.slice{s}.{i}.weight" for s, idx in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))) for i in idx)


def test_load_state_dict_rules():
    sd = _sd()
    m = cdc.LpipsVGG().load_state_dict(sd)                                   # no prefix in the keys: none is taken
    assert sorted(m.state_dict()) == sorted(sd)
    pre = {"loss_fn_vgg." + k: v for k, v in sd.items()}
    pre["denoise_fn.something"] = np.zeros(3, np.float32)                    # a whole checkpoint: the prefix is found
    assert sorted(cdc.LpipsVGG().load_state_dict(pre).state_dict()) == sorted(sd)
    assert sorted(cdc.LpipsVGG().load_state_dict(pre, prefix="loss_fn_vgg.").state_dict()) == sorted(sd)
    bad = dict(sd)
    bad.pop("net.slice3.12.bias")
    with pytest.raises(RuntimeError, match="missing"):
        cdc.LpipsVGG().load_state_dict(bad)
    cdc.LpipsVGG().load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError, match="unexpected"):
        cdc.LpipsVGG().load_state_dict(dict(sd, extra=np.zeros(1, np.float32)))
    with pytest.raises(RuntimeError, match="size mismatch"):
        cdc.LpipsVGG().load_state_dict(dict(sd, **{"lin2.model.1.weight": np.zeros((1, 255, 1, 1), np.float32)}))
    # the ModuleList copies and the scaling layer's buffers are accepted; a copy that differs is not
    full = synth.lpips_vgg_state_dict(seed=0, with_duplicates=True)
    full["scaling_layer.shift"] = np.asarray(LR.SHIFT, np.float32).reshape(1, 3, 1, 1)
    full["scaling_layer.scale"] = np.asarray(LR.SCALE, np.float32).reshape(1, 3, 1, 1)
    assert len(cdc.LpipsVGG().load_state_dict(full).state_dict()) == 31 + 5 + 2
    full["lins.3.model.1.weight"] = full["lins.3.model.1.weight"] + 1e-3
    with pytest.raises(RuntimeError, match="differs"):
        cdc.LpipsVGG().load_state_dict(full)
    with pytest.raises(RuntimeError, match="differs"):
        cdc.LpipsVGG().load_state_dict(full, strict=False)


class _Part:
    """Stands in for the U-Net / the context model: records what load_state_dict hands it."""
    device_index = 0

    def load_state_dict(self, sd, strict=True):
        self.got = dict(sd)


@pytest.mark.parametrize("cls,kw", [(cdc.GaussianDiffusionX, dict(ae_fn=None, pred_mode="x", var_schedule="cosine")), (cdc.GaussianDiffusionEps, {})])
def test_diffusion_load_state_dict_with_and_without_the_lpips_keys(cls, kw):
    base = {"denoise_fn.w": np.ones(2, np.float32), "context_fn.v": np.ones(3, np.float32)}
    diff = cls(_Part(), _Part(), **kw)
    assert diff.loss_fn_vgg is None
    diff.load_state_dict(base)
    assert diff.loss_fn_vgg is None and sorted(diff.denoise_fn.got) == ["w"] and sorted(diff.context_fn.got) == ["v"]
    diff.load_state_dict(dict(base, **synth.lpips_vgg_state_dict(seed=1, prefix="loss_fn_vgg.", with_duplicates=True)))
    assert isinstance(diff.loss_fn_vgg, cdc.LpipsVGG) and len(diff.loss_fn_vgg.state_dict()) == 36
    assert sorted(diff.denoise_fn.got) == ["w"] and sorted(diff.context_fn.got) == ["v"]
    with pytest.raises(RuntimeError, match="missing"):
        cls(_Part(), _Part(), **kw).load_state_dict(dict(base, **{"loss_fn_vgg.lin0.model.1.weight": np.zeros((1, 64, 1, 1), np.float32)}))


# ---- 3. arguments, and no GPU ----------------------------------------------------------------------------------------------------------

class _Untouchable:
    device_index = 0

    def _ready(self):
        raise AssertionError("the library was touched")

    _handle = _ready


def test_argument_rules_raise_before_the_library_is_touched():
    m = _Untouchable()
    f = np.zeros((2, 3, 32, 32), np.float32)
    with pytest.raises(ValueError, match="H, W >= 16"):
        metrics.lpips(m, f[:, :, :15], f[:, :, :15])
    with pytest.raises(ValueError, match="H, W >= 16"):
        metrics.lpips(m, f, f, size=(32, 15))
    with pytest.raises(ValueError, match="float32 or uint8"):
        metrics.lpips(m, f.astype(np.float64), f)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        metrics.lpips(m, f[:, :2], f)
    with pytest.raises(ValueError, match="images"):
        metrics.lpips(m, f[:1], f)
    with pytest.raises(ValueError, match="size="):
        metrics.lpips(m, f, np.zeros((2, 3, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="larger than operand"):
        metrics.lpips(m, f, f, size=(33, 32))
    with pytest.raises(ValueError, match="as_saved"):
        metrics.lpips(m, f, f, as_saved=(True,))
    with pytest.raises(AssertionError, match="touched"):
        metrics.lpips(m, f, f)


def test_compute_fails_loudly_without_gpu():
    m = cdc.LpipsVGG()
    f = np.zeros((1, 3, 16, 16), np.float32)
    with pytest.raises(_lib.CdcError, match="load_state_dict"):
        m(f, f)
    m.load_state_dict(_sd())
    with pytest.raises(_lib.CdcError, match="no HIP device"):
        m(f, f)
    with pytest.raises(_lib.CdcError, match="no HIP device"):
        metrics.lpips(m, f, f, return_layers=True)


def test_the_header_declares_both_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cdc_hip.h")).read()
    declared = set(re.findall(r"\b(cdc_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("cdc_lpips_create", "cdc_lpips"):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name)
    assert lpips.PREFIX == "loss_fn_vgg." and "loss_fn_vgg." in hdr
