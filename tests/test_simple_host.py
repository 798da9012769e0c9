"""SimpleCompressor (the GDN context model of the epsilon tree) without a GPU: a numpy restatement of the GDN1 reparametrisation and
of the operator against the real reference's fixtures (tests/golden/make_golden_simple.py), the manifests, the refusal of vbr=True,
the synthetic parameters and the export."""
import json
import os

import numpy as np
import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import synth
from helpers import GOLDEN
from simple_ref import full_manifest, gdn1_np, gdn_case, gdn_reparam_np


@pytest.fixture(scope="module")
def gdn_ops():
    return np.load(os.path.join(GOLDEN, "gdn_ops.npz"))


def test_fixture_shapes_are_the_stated_ones(gdn_ops):
    assert [tuple(s) for s in gdn_ops["shapes"]] == [(1, 16, 5, 7), (3, 48, 33, 31), (2, 64, 16, 16), (1, 192, 9, 20)]


@pytest.mark.parametrize("k", range(4))
def test_reparametrisation_matches_reference_bit_for_bit(gdn_ops, k):
    shape, x, beta, gamma, _, _ = gdn_case(gdn_ops, k)
    b2, g2 = gdn_reparam_np(beta, gamma)
    assert b2.dtype == np.float32 and g2.dtype == np.float32
    np.testing.assert_array_equal(b2.view(np.uint32), gdn_ops[f"c{k}_beta_r"].view(np.uint32))
    np.testing.assert_array_equal(g2.view(np.uint32), gdn_ops[f"c{k}_gamma_r"].view(np.uint32))
    # the synthetic parameters are those of synth, and the clamps act: beta[0] sits on the bound, the negative gammas give 0
    sb, sg = synth.gdn_layer_params(shape[1], seed=int(gdn_ops["seed"]) + k)
    np.testing.assert_array_equal(sb, beta)
    np.testing.assert_array_equal(sg, gamma)
    assert beta[0] == 0 and abs(float(b2[0]) - 1e-6) < 1e-9
    assert (g2[gamma < 2.0 ** -18] == 0).all() and (gamma < 0).mean() > 0.3
    assert (b2 >= 9e-7).all() and (g2 >= 0).all()           # norm > 0 always


@pytest.mark.parametrize("k", range(4))
def test_numpy_gdn1_matches_reference_outputs(gdn_ops, k):
    shape, x, beta, gamma, y, yinv = gdn_case(gdn_ops, k)
    assert y.shape == shape and yinv.shape == shape
    assert (x.reshape(-1)[0:35:7] == 0).all() and x.reshape(-1)[3] == 1e4 and x.reshape(-1)[-1] == -1e4
    b2, g2 = gdn_reparam_np(beta, gamma)
    for ref, inverse in ((y, False), (yinv, True)):
        want = gdn1_np(x, b2, g2, inverse)
        # float32 round-off of the reference's own C-term sum: a few C * 2^-24 relative per element
        err = np.abs(ref - want) / np.maximum(np.abs(want), 1e-30)
        assert float(err[want != 0].max()) < 64 * 2.0 ** -24 * np.sqrt(shape[1]), float(err[want != 0].max())
        assert (ref[want == 0] == 0).all()


@pytest.mark.parametrize("name", ["simple_small", "simple_full"])
def test_manifest_equals_reference(name):
    meta = json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))
    assert meta["class"] == "SimpleCompressor"
    m = cdc.epsilonparam.SimpleCompressor(**meta["kwargs"])
    ours = full_manifest(m)
    want = [(k, tuple(v)) for k, v in meta["manifest"] if not k.startswith("prior.")]
    assert ours == want
    # the reference's prior tensors are [C, 1, 1, in, out]; the library takes them squeezed (as for BigCompressor)
    assert [k for k, _ in meta["manifest"] if k.startswith("prior.")] != []
    assert m.padded_size(50, 70) == (64, 128) and m.frame_multiple == 64


def test_e2e_manifest_equals_reference():
    meta = json.load(open(os.path.join(GOLDEN, "manifest_simple_e2e.json")))
    m = cdc.epsilonparam.SimpleCompressor(**meta["comp_kwargs"])
    ours = full_manifest(m)
    assert ours == [(k, tuple(v)) for k, v in meta["comp_manifest"] if not k.startswith("prior.")]


def test_vbr_is_refused_with_the_reference_reason():
    with pytest.raises(NotImplementedError, match=r"TypeError: Identity\.forward\(\) takes 2 positional arguments but 3 were given"):
        cdc.epsilonparam.SimpleCompressor(vbr=True)
    # ... and by the library itself on a handle of these kinds
    from cdc_compression_amd import _lib
    m = cdc.epsilonparam.SimpleCompressor(dim=16)
    L = _lib.lib()
    for h in (m._handle(), m._enc_handle()):
        assert L.cdc_enable_vbr(h) == -1 and b"SimpleCompressor" in L.cdc_last_error(h)


def test_synthetic_state_dict_is_deterministic_and_clamped():
    m = cdc.epsilonparam.SimpleCompressor(dim=16, dim_mults=(1, 2, 3, 4), hyper_dims_mults=(4, 4, 4))
    man = m.encoder_manifest() + m.manifest()
    a = synth.simple_compressor_state_dict(man, seed=5)
    b = synth.simple_compressor_state_dict(man, seed=5)
    c = synth.simple_compressor_state_dict(man, seed=6)
    assert list(a) == [n for n, _ in man]
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 and a[k].shape == tuple(s) for k, s in man)
    assert not np.array_equal(a["enc.0.2.gamma"], c["enc.0.2.gamma"])
    n_gdn = 0
    for k, v in a.items():
        if k.endswith(".beta"):
            n_gdn += 1
            assert v[0] == 0 and abs(float(v[1:].mean()) - 1.0) < 0.1
        if k.endswith(".gamma"):
            off = v[~np.eye(v.shape[0], dtype=bool)]
            assert 0.3 < (off < 0).mean() < 0.7 and abs(float(np.diag(v).mean()) - np.sqrt(0.1)) < 0.05
    assert n_gdn == 6
    conv = synth.unet_state_dict([("enc.1.0.weight", (32, 16, 5, 5))], seed=5)
    np.testing.assert_array_equal(a["enc.1.0.weight"], conv["enc.1.0.weight"])


def test_simple_compressor_is_exported():
    from cdc_compression_amd import epsilonparam
    from cdc_compression_amd.compressor import SimpleCompressor, _ContextDecoder
    assert epsilonparam.SimpleCompressor is SimpleCompressor and issubclass(SimpleCompressor, _ContextDecoder)
    from cdc_compression_amd import _lib
    for s in ("cdc_simple_encoder_create", "cdc_simple_ctxdec_create", "cdc_op_gdn"):
        assert s in _lib.EXPORTS and hasattr(_lib.lib(), s)
