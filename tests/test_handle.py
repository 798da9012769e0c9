"""CPU tests of _lib.Handle, the one owner of a library handle in the Python mirror: a move to another device keeps what was loaded and
replays it into the handle the next use creates, touches no device and leaks no handle.  They lean on one fact of the library:
cdc_finalize_weights reports a missing key before it touches a device."""
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib
from cdc_compression_amd.compressor import _enable_vbr
from helpers import GOLDEN


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _handles():
    """(label, Handle) of every handle kind the mirror owns; the models are returned too so that they outlive the test."""
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    comp = cdc.ResnetCompressor(**json.load(open(os.path.join(GOLDEN, "manifest_encoder_small_x.json")))["kwargs"])
    lp = cdc.LpipsVGG()
    return (un, comp, lp), [("unet", un._lh), ("dec", comp._dec), ("hyper_dec", comp._hyper), ("enc", comp._enc), ("lpips", lp._lh)]


def _finalize_elsewhere(lh):
    """move(1), then the next use: the error finalize() gives.  On a host with GPUs the handle goes back to device 0 first, so that no
    second device is touched; the handle is a new one either way.  (There finalize() succeeds and "" comes back: the positive
    assertion of the caller then says little, and its left-out-tensor half is what proves the replay; on a host without a GPU, where
    this test is meant to run, "no HIP device" proves it.)"""
    lh.move(1)
    assert lh.raw is None and lh.device_index == 1
    if _has_gpu():
        lh.move(0)
    assert lh.ptr is not None and lh.raw is not None
    try:
        lh.finalize()
    except _lib.CdcError as e:
        return str(e)
    return ""


@pytest.mark.parametrize("kind", ["unet", "dec", "hyper_dec", "enc", "lpips"])
def test_move_replays_every_loaded_tensor(kind):
    keep, hs = _handles()
    lh = dict(hs)[kind]
    man = lh.manifest()
    for name, shape in man:
        lh.load(name, np.zeros(shape, np.float32))
    assert list(lh.tensors) == [n for n, _ in man] and not lh.finalized
    msg = _finalize_elsewhere(lh)
    assert "missing key" not in msg, msg
    if not _has_gpu():
        assert "no HIP device" in msg, msg
    # ... and a handle that had one tensor left out still says which one
    keep2, hs2 = _handles()
    lh2 = dict(hs2)[kind]
    left_out = man[len(man) // 2][0]
    for name, shape in man:
        if name != left_out:
            lh2.load(name, np.zeros(shape, np.float32))
    assert f'missing key "{left_out}"' in _finalize_elsewhere(lh2)


def test_squeezed_prior_tensors_replay_as_loaded():
    """load() remembers the array exactly as handed over: load_hyper_state_dict() squeezes the singleton axes of the prior.* entries, and
    the reference's 5-d shapes would be refused on replay."""
    meta = json.load(open(os.path.join(GOLDEN, "manifest_hyperdec_small_x.json")))
    comp = cdc.ResnetCompressor(**meta["kwargs"])
    sd = {k: np.zeros(s, np.float32) for k, s in meta["manifest"] + meta["prior_manifest"]}
    try:
        comp.load_hyper_state_dict(sd)
    except _lib.CdcError as e:                     # every tensor is loaded before the weights become final on a device
        assert not _has_gpu() and "no HIP device" in str(e), e
    lh, C = comp._hyper, comp.reversed_hyper_dims[0]
    assert set(lh.tensors) == set(sd)
    assert lh.tensors["prior.affine.1.weight"].shape == (C, 3, 3) and lh.tensors["prior.a.0"].shape == (C, 3)
    lh.move(1)
    if _has_gpu():
        lh.move(0)
    assert lh.ptr is not None                      # the replay passed the library's shape check
    with pytest.raises(_lib.CdcError, match="size mismatch"):
        lh.load("prior.a.0", sd["prior.a.0"])


def test_move_touches_no_device_and_leaks_no_handle():
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    assert un._h is None                           # created on first use
    first = un._handle()
    assert un._h is first and un._handle() is first
    un.to(0)
    assert un._h is first                          # same device: nothing happens
    un.to("cuda:1")
    assert un._h is None and un.device_index == 1 and un.status()["arith"] is None
    assert un._handle() is not None and un._h is not None
    lh = un._lh
    lh.close()
    lh.close()                                     # twice is harmless
    assert un._h is None
    comp = cdc.BigCompressor(dim=8, dim_mults=(1, 2), hyper_dims_mults=(2, 2, 2))
    comp._handle(), comp._hyper_handle(), comp._enc_handle()
    comp.to(1)
    assert (comp._h, comp._hh, comp._eh) == (None, None, None) and comp.device_index == 1
    assert all(v["arith"] is None for v in comp.status().values())


def test_load_copies_and_a_hand_destroyed_handle_is_not_destroyed_twice():
    un = cdc.Unet(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
    name, shape = un.manifest()[0]
    a = np.ones(shape, np.float32)
    un._lh.load(name, a)
    a[...] = 7.0                                   # what a move replays is what was loaded
    assert np.all(un.state_dict()[name] == 1.0)
    _lib.lib().cdc_destroy(un._handle())           # a caller that frees the handle itself tells the owner
    un._h = None
    assert un._h is None and un._handle() is not None
    del un


def test_a_raising_setup_leaves_no_handle_behind():
    seen = []

    def setup(h):
        seen.append(h.value)
        raise _lib.CdcError("setup refused")

    lp = cdc.LpipsVGG()
    lh = _lib.Handle("cdc_lpips_create", None, 0, setup)
    for _ in range(2):                             # the object stays usable: the next use tries again and raises the same error
        with pytest.raises(_lib.CdcError, match="setup refused"):
            lh.ptr
        assert lh.raw is None
    assert len(seen) == 2
    lh.setup = None
    assert lh.ptr is not None and len(lh.manifest()) == len(lp.manifest())
    # the compressor's own setup: cdc_enable_vbr on a model whose resampling layer is at index 1 is refused by the library
    comp = cdc.ResnetCompressor(dim=8, dim_mults=[1, 2], reverse_dim_mults=[2, 1], hyper_dims_mults=[2, 2, 2])
    comp._dec.setup = _enable_vbr
    with pytest.raises(_lib.CdcError, match=r"cdc_enable_vbr failed \(-1\): variable bitrate"):
        comp._handle()
    assert comp._h is None


def test_device_index_of():
    torch = pytest.importorskip("torch")

    class NoIndex:
        index = None

    for device, want in ((0, 0), (3, 3), ("cuda", 0), ("cuda:3", 3), (NoIndex(), 0), (torch.device("cuda:2"), 2),
                         (torch.device("cuda"), 0), (None, 0)):
        assert _lib.device_index_of(device) == want, device
    assert cdc.Unet(dim=16, device="cuda:3").device_index == 3
    assert cdc.LpipsVGG(device=torch.device("cuda", 2)).to(torch.device("cuda")).device_index == 0
