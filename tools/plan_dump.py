"""The launch programs the planner builds (csrc/cdc_planner.hip), as text: for each configuration below one forward (or one
single-operator call) builds the program, then its name and every op of cdc_prof_op -- label and flops, in program order -- go to
stdout.  Two builds of the library plan alike when their dumps are equal:

    CDC_DEBUG_PLAN=1 python tools/plan_dump.py > a.txt 2> a.err
    CDC_DEBUG_PLAN=1 CDC_HIP_LIB=/path/to/other/libcdc_hip.so python tools/plan_dump.py > b.txt 2> b.err
    diff a.txt b.txt; diff <(grep '^\\[plan\\]' a.err) <(grep '^\\[plan\\]' b.err)

python tools/plan_dump.py [NAME ...] dumps only the configurations whose name starts with one of NAME.  Inputs are zeros (a plan
depends on shapes alone), parameters the synthetic ones of the tests."""
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CDC_DEV"] = "1"       # the development switches below are read only in such a process (csrc/cdc_internal.h: dev_env)

import numpy as np  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import _lib, synth  # noqa: E402
from cdc_compression_amd.ops import Ops  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ALL_PLANES = {"CDC_PF_MIN_WAVES": "1", "CDC_PF_S2_MIN_WGS": "1", "CDC_PF_TZ_MIN_WGS": "1"}    # every planes-only site at batch 1


def meta(name):
    m = json.load(open(os.path.join(GOLDEN, f"manifest_{name}.json")))
    return m, [(k, tuple(v)) for k, v in m["manifest"]]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def dump(name, handle):
    """The op table of `handle`'s current program (a single-operator handle: of the calls it has made)."""
    L = _lib.lib()
    print(f"== {name}")
    print(f"[plan] == {name}", file=sys.stderr, flush=True)
    for i in range(L.cdc_prof_num_ops(handle)):
        lab, fl = ctypes.c_char_p(), ctypes.c_double()
        _lib.check(handle, L.cdc_prof_op(handle, i, ctypes.byref(lab), None, None, ctypes.byref(fl)))
        print(f"{i:4d} {lab.value.decode()} | {fl.value:.0f}")
    sys.stdout.flush()


_sd = {}


def unet(case, B, H, W):
    """One forward of a golden U-Net case at batch B, H x W (None: the case's golden shape).  Like every step below a generator of
    (name or None, handle): the object that owns the handle lives until the table has been read."""
    m, man = meta(case)
    kw = dict(m["unet_kwargs"])
    kw.pop("embd_type", None)
    if case not in _sd:
        _sd[case] = synth.unet_state_dict(man, seed=0, final_gain=0.2 if "eps" in case else 1.0)
    if B is None:
        g = np.load(os.path.join(GOLDEN, f"unet_{case}.npz"))
        B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    un = cdc.Unet(**kw)
    un.load_state_dict(_sd[case])
    ctx = [np.zeros((B, c, H >> l, W >> l), np.float32) for l, c in enumerate(m["context_channels_per_level"])]
    un(np.zeros((B, 3, H, W), np.float32), np.full((B, 1), 0.37, np.float32), ctx)
    yield None, un._handle()


def compressor(case, make_sd, **ckw):
    m, man = meta(case)
    comp = getattr(cdc.epsilonparam if m["class"] == "SimpleCompressor" else cdc, m["class"])(**m["kwargs"], **ckw)
    comp.load_state_dict(make_sd(man, seed=m.get("seed", 15)))
    return comp


def compressor_programs(tag, comp, B, rates=None, hyper=True):
    """Encoder, hyper decoder (as a batched call plans it, and as the entropy coder does: every image as a batch of one) and
    context decoder of one compressor at batch B, 256 x 256 images."""
    r = None if rates is None else np.full(B, rates, np.float32)
    x = np.zeros((B, 3, 256, 256), np.float32)
    latent, hyp = comp.analysis(x, r)
    yield f"{tag} encoder B={B}", comp._enc_handle()
    if hyper:
        comp.hyper_decode(np.zeros_like(hyp), cond=r)
        yield f"{tag} hyper decoder B={B}", comp._hyper_handle()
        comp.latents_to_bytes(latent, hyp, r)
        yield f"{tag} hyper decoder B={B} batch-1 plan", comp._hyper_handle()
    comp.decode(np.zeros_like(latent), r)
    yield f"{tag} context decoder B={B}", comp._handle()


def configurations():
    for B in (1, 32):
        yield f"unet full_x 256x256 B={B}", lambda B=B: unet("full_x", B, 256, 256)
        for pf in "012":
            yield f"unet full_x 256x256 B={B} CDC_PF={pf}", lambda B=B, pf=pf: env(CDC_PF=pf), lambda B=B: unet("full_x", B, 256, 256)
        yield f"unet full_x 256x256 B={B} CDC_ARITH=0", lambda: env(CDC_ARITH="0"), lambda B=B: unet("full_x", B, 256, 256)
        yield f"unet full_x 256x256 B={B} all planes", lambda: env(**ALL_PLANES), lambda B=B: unet("full_x", B, 256, 256)
        yield (f"unet full_x 256x256 B={B} all planes, joins miss", lambda: env(CDC_TEST_JOIN_MISS="1", **ALL_PLANES),
               lambda B=B: unet("full_x", B, 256, 256))
    yield "unet full_eps 256x256 B=32", lambda: unet("full_eps", 32, 256, 256)
    yield "unet full_x 512x512 B=16", lambda: unet("full_x", 16, 512, 512)
    yield "unet small_x 32x32 B=2", lambda: unet("small_x", 2, 32, 32)
    yield "unet odd_x golden shape", lambda: unet("odd_x", None, None, None)
    yield "unet full_x 64x64 B=1", lambda: unet("full_x", 1, 64, 64)
    for B in (1, 4):
        yield f"compressor full_x B={B}", lambda B=B: compressor_programs("full_x", compressor("encoder_full_x", synth.unet_state_dict), B)
        yield f"compressor vbr_full B={B}", lambda B=B: compressor_programs(
            "vbr_full", compressor("vbr_full", synth.compressor_state_dict, vbr=True), B, rates=0.37)
        yield f"compressor simple_full B={B}", lambda B=B: compressor_programs(
            "simple_full", compressor("simple_full", synth.simple_compressor_state_dict), B, hyper=False)
    yield "lpips 64x64 2 pairs", lpips
    for name, call in single_operators():
        yield f"op {name}", call


def lpips():
    model = cdc.LpipsVGG().load_state_dict(synth.lpips_vgg_state_dict(seed=0))
    a = np.zeros((2, 3, 64, 64), np.float32)
    model(a, a)
    yield None, model._handle()


def single_operators():
    z = lambda *s: synth.normal("plan_dump", s, seed=1, std=0.5)     # noqa: E731  (weights too: not zeros, their scale is divided by)

    def op(fn):
        def call():
            G = Ops(0)
            fn(G)
            yield None, G._h
        return call
    yield "conv2d 3x3 64->64 32x32 LN ReLU shift resid", op(lambda G: G.conv2d(
        z(2, 64, 32, 32), z(64, 64, 3, 3), z(64), padding=1, ln_g=z(64), ln_b=z(64), relu=True, shift=z(2, 64), resid=z(2, 64, 32, 32)))
    yield "conv2d 1x1 384->128 16x16", op(lambda G: G.conv2d(z(2, 384, 16, 16), z(128, 384, 1, 1), z(128)))
    yield "conv2d 3x3 stride 2 64->128 32x32", op(lambda G: G.conv2d(z(2, 64, 32, 32), z(128, 64, 3, 3), z(128), stride=2, padding=1))
    yield "conv_transpose2d 128->64 16x16", op(lambda G: G.conv_transpose2d(z(2, 128, 16, 16), z(128, 64, 4, 4), z(64)))
    yield "chan_layernorm_ex statistics only", op(lambda G: G.chan_layernorm_ex(z(2, 64, 16, 16), want_y=False))
    yield "chan_layernorm_ex nparts=4", op(lambda G: G.chan_layernorm_ex(z(4, 2, 64, 16, 16), g=z(64), b=z(64), relu=True))
    for C, S in ((64, 64), (192, 8)):
        yield f"linear_attention C={C} {S}x{S}", op(lambda G, C=C, S=S: G.linear_attention(
            z(2, C, S, S), z(C), z(C), z(3 * C, C), z(C, C), z(C)))


def main():
    want = sys.argv[1:]
    for name, *steps in configurations():
        if want and not any(name.startswith(w) for w in want):
            continue
        with (steps[0]() if len(steps) == 2 else contextlib.nullcontext()):
            for sub, handle in steps[-1]():
                dump(sub or name, handle)


if __name__ == "__main__":
    main()
