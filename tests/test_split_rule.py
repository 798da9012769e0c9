"""cdc_decode_chains (include/cdc_hip.h): how many chains a decode runs is decided in one host function, which touches
no device.  A Python restatement of it over a grid of batches, sizes, setter values and the handle state that forces one chain."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

import cdc_compression_amd as cdc
from cdc_compression_amd import _lib, tiles

KW = dict(dim=16, channels=3, context_channels=8, dim_mults=(1, 2, 3), context_dim_mults=(1, 2))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def library_rule(B, H, W):
    """The default (setter 0): the shapes profiles/split_decode.md measured faster as two chains and nothing smaller than them --
    at least 8 images and at least as many pixels as 32 images of 256 x 256 (or 8 of 512 x 512)."""
    return 2 if B >= 8 and B * H * W >= 32 * 256 * 256 else 1


def expected(setter, B, H, W, traced=False, frames=False, graph=False, env=0):
    if B < 2 or H < 1 or W < 1 or traced or frames or graph:
        return 1
    want = setter or env
    return want if want in (1, 2) else library_rule(B, H, W)


def test_rule_over_a_grid_of_batches_sizes_and_handle_state():
    L = _lib.lib()
    un = cdc.Unet(**KW)
    h = un._handle()
    assert os.environ.get("CDC_GRAPH") in (None, "0") and not os.environ.get("CDC_DECODE_CHAINS")
    steps = (ctypes.c_int * 1)(0)
    for setter, traced, frames in itertools.product((0, 1, 2), (False, True), (False, True)):
        un.set_decode_chains(setter)
        _lib.check(h, L.cdc_set_trace(h, steps, 1 if traced else 0, _lib.CDC_TRACE_X0, 0, 0))
        for B, S in itertools.product((1, 2, 3, 4, 7, 8, 16, 31, 32, 64), (32, 64, 256, 512, 1024)):
            rows = [(S, S, 0, 0)] * B if frames else None
            with tiles.noise_frames(h, rows):
                assert un.decode_chains(B, S, S) == expected(setter, B, S, S, traced, frames), (setter, traced, frames, B, S)
    _lib.check(h, L.cdc_set_trace(h, steps, 0, 0, 0, 0))
    un.set_decode_chains(2)
    assert un.decode_chains(1, 64, 64) == 1 and un.decode_chains(0, 64, 64) == 1 and un.decode_chains(2, 64, 64) == 2
    # out of range: refused, the setting stays
    assert L.cdc_set_decode_chains(h, 3) != 0 and L.cdc_set_decode_chains(h, -1) != 0
    assert un.decode_chains(2, 64, 64) == 2


@pytest.mark.parametrize("env,want", [({"CDC_GRAPH": "1"}, [1, 1, 1]), ({"CDC_DEV": "1", "CDC_DECODE_CHAINS": "2"}, [2, 1, 2]),
                                      ({"CDC_DEV": "1", "CDC_DECODE_CHAINS": "2s"}, [2, 1, 2]), ({"CDC_DEV": "1", "CDC_DECODE_CHAINS": "1"}, [1, 1, 2]),
                                      ({"CDC_DEV": "0", "CDC_DECODE_CHAINS": "2"}, [library_rule(32, 256, 256), 1, 2])])
def test_rule_under_the_environment_switches(env, want):
    """hipGraph replay (CDC_GRAPH) is a fall-back; the development switch CDC_DECODE_CHAINS stands in for the setter's 0 only, and
    only in a CDC_DEV process.  (The library reads its environment once: a process of its own.)  Setter 0 / 1 / 2 at batch 32."""
    code = ("import cdc_compression_amd as cdc\n"
            f"un = cdc.Unet(**{KW!r})\n"
            "print([un.set_decode_chains(s).decode_chains(32, 256, 256) for s in (0, 1, 2)])\n")
    e = {k: v for k, v in os.environ.items() if k not in ("CDC_GRAPH", "CDC_DECODE_CHAINS", "CDC_DEV")}
    e.update(env, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == str(want), out
