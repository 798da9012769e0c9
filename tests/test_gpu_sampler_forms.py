"""The sampler step's two sources of the model output hold the same bits: the tensor the final convolution's combine launch wrote
(CDC_NO_COMBINE_FUSE=1) and the 7-row combine evaluated inside the sampler kernel (the default).  On small_x's 32 x 32 frame both reads
happen in the four-pixel form, on odd_x's model at 24 x 42 both in the scalar form; DDIM at eta = 0, the seeded DDIM and the multistep
update each.

The switch is read once per process, so every decode runs in a child process of its own (this file, run as a script)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VARIANTS = {
    "ddim": dict(sample_steps=4),
    "ddim_seeded": dict(sample_steps=4, eta=0.5, gamma=1.0, seed=(3 << 33) + 17),
    "dpmpp_2m": dict(sample_steps=5, sampler="dpmpp_2m"),
}


def _decode(frame, variant, out):
    import cdc_compression_amd as cdc
    from cdc_compression_amd import synth
    from helpers import load_case
    from test_gpu_parity import make_unet
    if frame == "small_x":
        un, _, _, x, _, ctx, _ = make_unet("small_x")
        shape = x.shape
        assert shape[3] % 4 == 0
    else:
        kw, _, sd, *_ = load_case("odd_x")
        un = cdc.Unet(**kw)
        un.load_state_dict(sd)
        shape = (2, 3, 24, 42)
        ctx = synth.context_pyramid([5], 2, 24, 42, seed=3)
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    args = dict(VARIANTS[variant])
    if "seed" not in args:
        args["init"] = synth.normal("init", shape, seed=1, std=0.8)
    rec = diff.decompress(ctx, shape, **args)
    np.save(out, rec)
    print(json.dumps(un.status()))


def _child(frame, variant, fused, out):
    env = {k: v for k, v in os.environ.items() if k != "CDC_NO_COMBINE_FUSE"}
    if not fused:
        env["CDC_NO_COMBINE_FUSE"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), frame, variant, out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out), json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("frame", ["small_x", "24x42"])
def test_model_output_from_the_tensor_and_from_the_fused_combine_hold_the_same_bits(frame, variant, tmp_path):
    given, st_given = _child(frame, variant, False, str(tmp_path / "given.npy"))
    fused, st_fused = _child(frame, variant, True, str(tmp_path / "fused.npy"))
    assert np.isfinite(fused).all() and float(np.abs(fused).max()) > 0.05
    assert st_given["range_faults"] == 0 and st_fused["range_faults"] == 0, (st_given, st_fused)
    np.testing.assert_array_equal(given, fused)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _decode(*sys.argv[1:4])
