"""Float64 statement of the denoising U-Net (xparam / epsilonparam modules/unet.py:18-135, network_components.py:10-139), stage by
stage, and the input cases that put the forms only a network program runs at their edges.  What tests/test_gpu_unet_edges.py compares
the library's taps with, pinned to the real reference's float64 run by tests/golden/unet_edges.npz
(tests/golden/make_golden_unet_edges.py, tests/test_unet_ref_host.py).

Float64 throughout, no float32 rounding between operations (oracle/model.py rounds between operators and stays the suite's float32
oracle).  The operators are not restated: a convolution is conv_ref._conv, a LayerNorm attention_ref._layernorm (see _ln), the PreNorm
statistics ln_ref.ln_f64, an attention attention_ref.linear_attention; this module owns the wiring, the time MLP and the cases.

    forward(sd, cfg, x, time, ctx) -> (y, taps)      every name cdc_unet_tap knows, but the attention kernels' own intermediates
                                                     (<attn>.kv/.S/.Z/.kmax/.M: scaled, kernel-dependent layouts; tests/test_gpu_attention_edges.py)
    stage(sd, cfg, name, inputs) -> output           one stage alone from ITS inputs (wiring() says which taps those are)
    build(case, config) -> (cfg, sd, x, time, ctx)   the seeded draw of tests/helpers.py (synth.unet_state_dict seed 0, image seed 1,
                                                     context seed 3) with the case's edit

Cases, and the kernel mistake each is for:
    normal          B = 3, time 0.05 / 0.5 / 0.93: the rows of the shift table differ, so a shift, a per-image weight or a hoisted
                    partial sum taken from another image is an error of the size of the activations.
    time_ends       time 0, 1 and 1 / 8193 (the ends of embd_type "01" and the smallest step of the longest schedule): the time MLP's
                    GELU at its tails and every mlp.1 shift.
    rows            B = 3, image, context and time of row 2 equal to row 0, row 1 different: rows 0 and 2 are bit-equal at every tap,
                    whatever the arithmetic -- per-image weights, per-image shifts and hoisted sums indexed by the image.
    x_only          context = 0: the hoisted context-only partial sums are a bias-free convolution of zeros; the x-part is alone.
    ctx_only        image = 0: the unfolded / 3-channel first layer contributes nothing; the hoisted part is alone.  Together the two
                    catch a wrong channel offset in a concatenated first layer, which `normal` lets cancel.
    offset          block2's LayerNorm of every level's second ResnetBlock and of mid_block1 (the tensors a PreNorm reads) gets
                    g x OFFSET_G and b + OFFSET_B: each pixel's channel vector has a mean many times its spread -- the PreNorm
                    statistics from the convolution epilogue and the folded PreNorm that subtracts the mean on load.  The attention
                    that reads it gets to_out.bias - OFFSET_B, so its output and the next level start from ordinary values again:
                    without that the Downsample turns the mean into spread (40 sum(w) per channel) and only level 0 keeps a ratio
                    above 2.  Median |mean| / std over the pixels, full-width model: 46 at level 0, 19, 14, 14, 9, 9 below and 7 at
                    mid_block1 (the deeper residual streams are wider); OFFSET_RATIO and OFFSET_RATIO_0 are asserted in
                    tests/test_unet_ref_host.py.
    const_channels  block1 of CONST_BLOCKS (one per kernel family) has weight 0 and bias CONST_C: the variance over channels is exactly
                    0, rstd = 1 / sqrt(1e-5), block1 returns ReLU(b) + shift exactly.  E[x^2] - mean^2 gives rubbish here.
    dead            block1 of DEAD_BLOCKS has LayerNorm g x 0.25, b = -10 and a zero time projection: its ReLU output is exactly 0,
                    block2 convolves zeros (zero planes) and the block's output is ReLU(LN(bias)) + residual.
    ragged          the seeded draw at a frame whose tiles are ragged at several levels and whose coarse levels are narrower than 4
                    pixels (32 x 96 on the six-level model: 1 x 3 at the bottom; odd_x's 24 x 40).

No case was made milder: tests/golden/make_golden_unet_edges.py finds the largest bound max(5e-6, 3 e32) of any stage of any case at
OFFSET_B = 40 and CONST_C = 100 below TOL_DEC (it is stored as `worst_bound`, and tests/test_unet_ref_host.py asserts it)."""
import functools
import json
import math
import os
import re

import numpy as np

import attention_ref
import conv_ref
import ln_ref
from cdc_compression_amd import synth
from oracle import model as om

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_DEC = 5e-5          # tests/test_gpu_parity.py: the loosest figure the suite grants a chain; no stage-local bound may exceed it
OP_BOUND = 5e-6         # tests/test_gpu_parity.py: the operator bound
NSAMPLE = 32            # sampled values per tap in the fixture

OFFSET_G, OFFSET_B = 0.25, 40.0
OFFSET_RATIO = 6.0      # the median |mean| / std over the pixels of every PreNorm input of `offset` is at least this ...
OFFSET_RATIO_0 = 40.0   # ... and at level 0 this
CONST_C = 100.0
CONST_BLOCKS = ("downs.0.0", "downs.1.0", "downs.2.1", "downs.5.0", "mid_block1", "ups.0.0", "ups.4.0", "ups.4.1")
DEAD_BLOCKS = ("downs.0.0", "downs.1.1", "downs.3.0", "mid_block2", "ups.1.1", "ups.4.0")
BATCH3 = ("normal", "time_ends", "rows")
TIMES = {"normal": (0.05, 0.5, 0.93), "time_ends": (0.0, 1.0, 1.0 / 8193), "rows": (0.05, 0.5, 0.05)}
CASES = ("normal", "time_ends", "rows", "x_only", "ctx_only", "offset", "const_channels", "dead")

# configuration -> (golden manifest, H, W, cases)
CONFIGS = {
    "full_x": ("full_x", 64, 64, CASES),
    "full_eps": ("full_eps", 64, 64, CASES),
    "ragged_x": ("full_x", 32, 96, ("ragged",)),
    "small_x": ("small_x", 32, 32, ("normal", "rows", "const_channels", "dead")),
    "odd_x": ("odd_x", 24, 40, ("ragged", "offset")),
    # The attention folds its output projection where N >= 16 C (attention_ref.PATHS): at 64 x 64 the full-width model does so at
    # C = 64 only (level 0, and 32 x 32 of the last decoder level), its 128- and 192-channel levels take the one-launch few-pixel
    # chain.  The smallest models and frames that fold at C = 128 (fused k/v pass: N = 2048) and at C = 192 (N = 3072):
    "fold128": (dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2), context_dim_mults=(1,)), 64, 128, ("rows", "offset")),
    "fold192": (dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 3), context_dim_mults=(1,)), 96, 128, ("rows", "offset")),
}


class Config:
    def __init__(self, name):
        man, self.H, self.W, self.cases = CONFIGS[name]
        self.name = name
        if isinstance(man, dict):           # no golden manifest: the oracle's, which make_golden_unet_edges.py compares with the reference's state_dict
            self.kw = dict(man)
            ocfg = om.UnetConfig(**self.kw)
            self.manifest = [(a, tuple(b)) for a, b in om.unet_manifest(ocfg)]
            self.ctx_channels = ocfg.context_dims[:min(ocfg.num_resolutions - 1, len(ocfg.context_dims) - 1)]
        else:
            mj = json.load(open(os.path.join(GOLDEN, f"manifest_{man}.json")))
            self.kw = dict(mj["unet_kwargs"])
            self.kw.pop("embd_type", None)
            self.manifest = [(a, tuple(b)) for a, b in mj["manifest"]]
            self.ctx_channels = list(mj["context_channels_per_level"])
        self.final_gain = 0.2 if "eps" in name else 1.0
        self.dim = self.kw["dim"]
        self.dims = [self.kw["channels"]] + [self.dim * m for m in self.kw["dim_mults"]]
        self.n = len(self.dims) - 1
        self.n_ctx = len(self.ctx_channels)
        self.names = {n for n, _ in self.manifest}

    def resblocks(self):
        """ResnetBlock prefixes in the library's order (csrc/cdc_weights.hip), which is the order of the shift table."""
        out = []
        for i in range(self.n):
            out += [f"downs.{i}.0", f"downs.{i}.1"]
        out += ["mid_block1", "mid_block2"]
        for i in range(self.n - 1):
            out += [f"ups.{i}.0", f"ups.{i}.1"]
        return out

    def shift_layout(self):
        """({prefix: (offset, channels)}, row length) of the shift table [B, shift_bs]: every block's row padded to 32."""
        off, lay = 0, {}
        for p in self.resblocks():
            c = dict(self.manifest)[p + ".mlp.1.bias"][0]
            lay[p] = (off, c)
            off += -(-c // 32) * 32
        return lay, off


@functools.lru_cache(maxsize=None)
def config(name):
    return Config(name)


def wiring(cfg, final_ln_done=False):
    """[(stage, the tap that holds its output, the taps concatenated on its input)] in program order; "x", "time", "ctx<l>" are the
    inputs, "y" the output.  final_ln_done: the program applied the final LayerNorm in the last Upsample's epilogue, `ups.<n-2>` is
    absent and `final_conv.0` holds LN(Upsample(.)): that pair is one stage, the 7 x 7 convolution the next."""
    n = cfg.n
    out, prev = [("temb", "temb", ["time"])], "x"
    for i in range(n):
        out.append((f"downs.{i}.0", f"downs.{i}.0", [prev] + ([f"ctx{i}"] if i < cfg.n_ctx else [])))
        out.append((f"downs.{i}.1", f"downs.{i}.1", [f"downs.{i}.0"]))
        out.append((f"downs.{i}.2", f"downs.{i}.2", [f"downs.{i}.1"]))
        prev = f"downs.{i}.2"
        if i < n - 1:
            out.append((f"downs.{i}.3", f"downs.{i}.3", [prev]))
            prev = f"downs.{i}.3"
    out += [("mid_block1", "mid_block1", [prev]), ("mid_attn", "mid_attn", ["mid_block1"]), ("mid_block2", "mid_block2", ["mid_attn"])]
    prev = "mid_block2"
    for i in range(n - 1):
        out.append((f"ups.{i}.0", f"ups.{i}.0", [prev, f"downs.{n - 1 - i}.2"]))
        out.append((f"ups.{i}.1", f"ups.{i}.1", [f"ups.{i}.0"]))
        out.append((f"ups.{i}.2", f"ups.{i}.2", [f"ups.{i}.1"]))
        if final_ln_done and i == n - 2:
            out.append((f"ups.{i}.3+final_conv.0", "final_conv.0", [f"ups.{i}.2"]))
            out.append(("final_conv.1", "y", ["final_conv.0"]))
            return out
        out.append((f"ups.{i}.3", f"ups.{i}", [f"ups.{i}.2"]))
        prev = f"ups.{i}"
    out.append(("final", "y", [prev]))
    return out


def stage_names(cfg):
    """Every stage either wiring names, in a fixed order: the rows of the fixture's `e32`."""
    a = [s for s, _, _ in wiring(cfg)]
    return a + [s for s, _, _ in wiring(cfg, True) if s not in a]


def tap_names(cfg):
    """Every tap forward() returns, in a fixed order: the rows of the fixture's `val` / `sum` / `amax`."""
    out = []
    for _, tap, _ in wiring(cfg):
        if tap == "y":
            continue
        out.append(tap)
        if tap.startswith("downs.") and tap.endswith(".1"):
            out += [tap + ".stat_mean", tap + ".stat_rstd"]
    return out + ["final_conv.0", "y"]


# ---- the operators (each stated once, elsewhere) -----------------------------------------------------------------------------------------

def _f64(a):
    return np.asarray(a, np.float64)


def _conv(x, w, b, stride=1, pad=0):
    B, Ci, H, W = x.shape
    w = _f64(w)
    y = conv_ref._conv(x, w, (B, Ci, H, W, w.shape[0], w.shape[-1], stride, pad))
    return y if b is None else y + _f64(b).reshape(1, -1, 1, 1)


def _conv_transpose(x, w, b):
    B, Ci, H, W = x.shape
    return conv_ref._conv(x, _f64(w), (B, Ci, H, W, w.shape[1])) + _f64(b).reshape(1, -1, 1, 1)


def _ln(x, g, b, relu=False, shift=None):
    """LayerNorm, ReLU, + shift[b, c].  attention_ref's statement, whose eps is the reference's 1e-5 in float64; ln_ref.ln_f64 states the
    same with eps = float32(1e-5), what a float32 evaluation adds -- 2.5e-13 of eps apart, which a variance of 0.01 turns into 1e-11 of
    the result, more than the 1e-12 the fixture is held to.  (The statistics taps are ln_ref's: its bound is what they are held to.)"""
    y = attention_ref._layernorm(_f64(x), _f64(g), _f64(b))
    if relu:
        y = np.maximum(y, 0.0)
    return y if shift is None else y + _f64(shift)[:, :, None, None]


def _gelu(h):
    return 0.5 * h * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(h / math.sqrt(2.0)))


def time_embedding(sd, time):
    """unet.py:41: Linear(1, 4 dim), GELU (erf), Linear(4 dim, dim); [B, dim]."""
    t = _f64(time).reshape(-1, 1)
    h = _gelu(t @ _f64(sd["time_mlp.0.weight"]).T + _f64(sd["time_mlp.0.bias"]))
    return h @ _f64(sd["time_mlp.2.weight"]).T + _f64(sd["time_mlp.2.bias"])


def block_shift(sd, p, temb):
    """ResnetBlock.mlp (network_components.py:97-100): Linear(LeakyReLU(0.2)(temb)); [B, dim_out]."""
    t = np.where(temb >= 0, temb, 0.2 * temb)
    return t @ _f64(sd[p + ".mlp.1.weight"]).T + _f64(sd[p + ".mlp.1.bias"])


def block(sd, p, x, shift=None):
    """Block (network_components.py:83-91) and, with `shift`, the time embedding ResnetBlock.forward adds to block1."""
    w = sd[p + ".block.0.weight"]
    return _ln(_conv(x, w, sd[p + ".block.0.bias"], 1, w.shape[-1] // 2), sd[p + ".block.1.g"], sd[p + ".block.1.b"], True, shift)


def resnet_block(sd, p, x, shift, parts=False):
    """ResnetBlock.forward (network_components.py:107-114); shift = block_shift(...).  parts: (output, block1's output h1)."""
    h1 = block(sd, p + ".block1", x, shift)
    res = _conv(x, sd[p + ".res_conv.weight"], sd[p + ".res_conv.bias"]) if p + ".res_conv.weight" in sd else x
    y = block(sd, p + ".block2", h1) + res
    return (y, h1) if parts else y


def attention(sd, p, x):
    return attention_ref.linear_attention(x, sd[p + ".fn.norm.g"], sd[p + ".fn.norm.b"], sd[p + ".fn.fn.to_qkv.weight"],
                                          sd[p + ".fn.fn.to_out.weight"], sd[p + ".fn.fn.to_out.bias"])


def shift_table(sd, cfg, temb):
    """The library's `temb` tap: [B, 1, 1, shift_bs], block_shift of every ResnetBlock at its offset (the padding is 0 here and
    unwritten there: table_mask)."""
    lay, bs = cfg.shift_layout()
    out = np.zeros((temb.shape[0], 1, 1, bs))
    for p, (off, c) in lay.items():
        out[:, 0, 0, off:off + c] = block_shift(sd, p, temb)
    return out


def table_mask(cfg):
    lay, bs = cfg.shift_layout()
    m = np.zeros(bs, bool)
    for off, c in lay.values():
        m[off:off + c] = True
    return m


def stage(sd, cfg, name, inputs):
    """One stage alone.  inputs: {"x": the arrays wiring() lists for the stage (concatenated on the channel axis; [time] for `temb`),
    and for a ResnetBlock "shift" [B, dim_out] (a row slice of the shift table) or "temb" [B, dim]}."""
    if name == "temb":
        return shift_table(sd, cfg, time_embedding(sd, inputs["x"][0]))
    x = np.concatenate([_f64(a) for a in inputs["x"]], axis=1)
    if "+" in name:                                        # "ups.<i>.3+final_conv.0"
        for part in name.split("+"):
            x = stage(sd, cfg, part, {"x": [x]})
        return x
    if name == "final":
        return stage(sd, cfg, "final_conv.1", {"x": [stage(sd, cfg, "final_conv.0", {"x": [x]})]})
    if name == "final_conv.0":
        return _ln(x, sd["final_conv.0.g"], sd["final_conv.0.b"])
    if name == "final_conv.1":
        return _conv(x, sd["final_conv.1.weight"], sd["final_conv.1.bias"], 1, 3)
    if name in cfg.resblocks():
        shift = _f64(inputs["shift"]) if "shift" in inputs else block_shift(sd, name, _f64(inputs["temb"]))
        return resnet_block(sd, name, x, shift)
    if name.endswith(".2") or name == "mid_attn":
        return attention(sd, name, x)
    if name.startswith("downs."):
        return _conv(x, sd[name + ".conv.weight"], sd[name + ".conv.bias"], 2, 1)
    return _conv_transpose(x, sd[name + ".conv.weight"], sd[name + ".conv.bias"])


def forward(sd, cfg, x, time, ctx):
    """Unet.forward (unet.py:106-135) as the chain of stage() over wiring(): (y, taps)."""
    taps = {"x": _f64(x), "time": _f64(time)}
    for l, c in enumerate(ctx):
        taps[f"ctx{l}"] = _f64(c)
    temb = time_embedding(sd, time)
    for name, tap, ins in wiring(cfg):
        taps[tap] = stage(sd, cfg, name, {"x": [taps[k] for k in ins], "temb": temb})
        if tap.startswith("downs.") and tap.endswith(".1"):
            B, C, H, W = taps[tap].shape
            st = ln_ref.ln_f64(taps[tap].reshape(1, B, C, 1, H * W))
            taps[tap + ".stat_mean"] = st["mean"].reshape(B, 1, H, W)
            taps[tap + ".stat_rstd"] = st["rstd"].reshape(B, 1, H, W)
    taps["final_conv.0"] = stage(sd, cfg, "final_conv.0", {"x": [taps[f"ups.{cfg.n - 2}"]]})
    return taps["y"], taps


def relerr(got, ref):
    return attention_ref.relerr(got, ref)


def row_errors(got, ref):
    """Per image: max |got - ref| / max(1, max |ref| over the batch)."""
    ref = _f64(ref)
    B = ref.shape[0]
    return np.abs(_f64(got) - ref).reshape(B, -1).max(1) / max(1.0, float(np.abs(ref).max()))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def offset_blocks(cfg):
    return [f"downs.{i}.1" for i in range(cfg.n)] + ["mid_block1"]


def offset_attention(p):
    """The attention that reads ResnetBlock `p` of offset_blocks."""
    return "mid_attn" if p == "mid_block1" else p[:-1] + "2"


def const_blocks(cfg):
    return [p for p in CONST_BLOCKS if p + ".mlp.1.bias" in cfg.names]


def dead_blocks(cfg):
    return [p for p in DEAD_BLOCKS if p + ".mlp.1.bias" in cfg.names]


def build(case, config_name):
    """(cfg, sd, x, time [B, 1], ctx) of a case: float32, a pure function of its arguments made of exact operations only."""
    cfg = config(config_name)
    assert case in cfg.cases, (case, config_name)
    B, H, W = (3 if case in BATCH3 else 1), cfg.H, cfg.W
    sd = synth.unet_state_dict(cfg.manifest, seed=0, final_gain=cfg.final_gain)
    x = synth.normal("x", (B, 3, H, W), seed=1, std=0.8)
    ctx = synth.context_pyramid(cfg.ctx_channels, B, H, W, seed=3)
    time = np.array(TIMES.get(case, (0.4,)), np.float64).astype(np.float32).reshape(B, 1)
    if case == "rows":
        x[2] = x[0]
        for c in ctx:
            c[2] = c[0]
    elif case == "x_only":
        ctx = [np.zeros_like(c) for c in ctx]
    elif case == "ctx_only":
        x = np.zeros_like(x)
    elif case == "offset":
        for p in offset_blocks(cfg):
            sd[p + ".block2.block.1.g"] = sd[p + ".block2.block.1.g"] * np.float32(OFFSET_G)
            sd[p + ".block2.block.1.b"] = sd[p + ".block2.block.1.b"] + np.float32(OFFSET_B)
            q = offset_attention(p) + ".fn.fn.to_out.bias"
            sd[q] = sd[q] - np.float32(OFFSET_B)
    elif case == "const_channels":
        for p in const_blocks(cfg):
            sd[p + ".block1.block.0.weight"] = np.zeros_like(sd[p + ".block1.block.0.weight"])
            sd[p + ".block1.block.0.bias"] = np.full_like(sd[p + ".block1.block.0.bias"], CONST_C)
    elif case == "dead":
        for p in dead_blocks(cfg):
            sd[p + ".block1.block.1.g"] = sd[p + ".block1.block.1.g"] * np.float32(0.25)
            sd[p + ".block1.block.1.b"] = np.full_like(sd[p + ".block1.block.1.b"], -10.0)
            sd[p + ".mlp.1.weight"] = np.zeros_like(sd[p + ".mlp.1.weight"])
            sd[p + ".mlp.1.bias"] = np.zeros_like(sd[p + ".mlp.1.bias"])
    return cfg, sd, x, time, ctx


def checksum(args):
    """sha256 over the bytes of the float32 inputs and parameters (as attention_ref.checksum): a host on which build() gives other
    bits fails loudly."""
    cfg, sd, x, time, ctx = args
    return attention_ref.checksum([x, time, *ctx] + [sd[n] for n, _ in cfg.manifest])


def entries():
    """Every (configuration, case), in a fixed order: the entries of tests/golden/unet_edges.npz."""
    return [(c, case) for c in CONFIGS for case in CONFIGS[c][3]]


def entry_key(config_name, case):
    return f"{config_name}|{case}"


def sample_idx(size):
    return attention_ref.sample_idx(NSAMPLE, size)


# ---- which cases run under which switches, and the forms each program must show ------------------------------------------------------------

_PLANES = {"CDC_PF_MIN_WAVES": "1", "CDC_PW_MIN_WAVES": "1", "CDC_PF_S2_MIN_WGS": "1", "CDC_PF_TZ_MIN_WGS": "1", "CDC_PF_17_MIN_WGS": "1",
           "CDC_PF_UF_MIN_WGS": "1"}
# every switch is one that test_unet_forward_alternate_kernel_modes (tests/test_gpu_parity.py) runs
SWITCHES = {
    "default": {},
    "planes": _PLANES,                       # small launches take the plane forms (stride 2, fused phases, first and final layer) and planes-only tensors
    "pf0": {"CDC_PF": "0"},                  # no plane operands: the register-staged split kernels
    "exact": {"CDC_ARITH": "0"},             # bf16x3 arithmetic
    "nohoist": {"CDC_NO_HOIST": "1"},        # the context halves evaluated every step, inside the concatenated layers
    "nofold": {"CDC_NO_ATTN_FOLD": "1"},     # q, k, v staged, out = ctx^T q with per-image weights, to_out separately
}
_B1 = tuple(c for c in CASES if c not in BATCH3)
# (configuration, switch set) -> cases.  The default program and the plane forms take every case; a switch that replaces one form takes
# `normal` and the cases aimed at that form (the others would run the very kernels `default` already ran them on).
RUNS = {
    ("full_x", "default"): CASES, ("full_x", "planes"): CASES,
    ("full_x", "pf0"): ("normal", "offset", "const_channels"), ("full_x", "exact"): ("normal", "offset", "const_channels"),
    ("full_x", "nohoist"): ("normal", "x_only", "ctx_only"), ("full_x", "nofold"): ("normal", "offset"),
    ("full_eps", "default"): CASES, ("full_eps", "planes"): ("normal", "rows", "x_only", "ctx_only", "offset"),
    ("full_eps", "pf0"): ("normal",), ("full_eps", "exact"): ("normal",), ("full_eps", "nohoist"): ("x_only", "ctx_only"),
    ("full_eps", "nofold"): ("normal",),
    ("ragged_x", "default"): ("ragged",), ("ragged_x", "planes"): ("ragged",), ("ragged_x", "pf0"): ("ragged",), ("ragged_x", "exact"): ("ragged",),
    ("small_x", "default"): ("normal", "rows", "const_channels", "dead"), ("small_x", "planes"): ("normal", "rows"), ("small_x", "exact"): ("normal",),
    ("odd_x", "default"): ("ragged", "offset"), ("odd_x", "planes"): ("ragged",), ("odd_x", "pf0"): ("ragged",), ("odd_x", "exact"): ("ragged", "offset"),
    ("fold128", "default"): ("rows", "offset"), ("fold128", "planes"): ("rows", "offset"), ("fold128", "exact"): ("offset",),
    ("fold192", "default"): ("rows", "offset"), ("fold192", "planes"): ("rows", "offset"), ("fold192", "exact"): ("offset",),
}


# (configuration, switch set) -> (present, absent[, {batch: more that is present at that batch}]): regular expressions over the program's labels (white space collapsed; csrc/cdc_state.h:
# op_label).  An entry of several expressions must match ONE label.  Every entry of `present` is in the program, none of `absent`.
# The plan of a layer depends on the launch size: where the one-image cases (B = 1) and `normal` / `rows` / `time_ends` (B = 3) take
# different kernels for a form, the third element says which.
_PRE, _PERIMG = r" pre( |$)", r" perimg( |$)"                                  # folded PreNorm (mean on load, rstd in the epilogue); per-image weights
_FIRST = [r"^temb$", (r"^conv 7x7 ", r" HOIST$"), r"^unfold$", r"^conv 7x1 s1 21->64 "]      # time MLP; hoisted context half, explicit unfold pass and unfolded first layer
_FINAL = [r"^conv 1x7 s1 64->21 ", r"^combine$"]                               # the row-folded final convolution and its 7-row combine
_FULL = _FIRST + _FINAL + [
    (r"^conv 3x3 s1 ", r" pre_add$"), (r"^conv 1x1 s1 ", r" WS1 pre_add$"),      # hoisted partial sums entering block1 and the res_conv of the levels with context
    r"^copy HOIST$",                                                             # the context half of downs.1.0's concatenated identity residual, copied once
    r"^kvctx C=64 N=4096 ", r"^ctxf C=64 N=4096 ", (r"^conv 1x1 s1 64->64 out 64x64 ", r" pre .*\+res$"),   # level 0: fused k/v pass, fold, folded output
    r"^kstats C=64 N=1024 ", r"^ctxf C=64 N=1024 ",                              # ups.4: the unfused folded chain
    r"^ctx1 C=128 N=1024 ", r"^ctx1 C=384 N=4 ", (r" WS1 ", _PRE), (r" WS1 ", _PERIMG),     # few-pixel levels: one-launch context, folded-PreNorm projection, ctx^T q per image
    (r" WS1 pre perimg \+res$",),                                                # ... and a folded output on per-image planes
    r"^conv 3x3 s2 ", (r"^conv 2x2 s1 64->64 out 32x32 ", r" LN$"),              # Downsample; the last Upsample with the final LayerNorm in its epilogue (final_conv.0)
]
_L0_OUT = {3: [(r"^conv 1x1 s1 64->64 out 64x64 ", r" SPLIT2H pre \+res$")], 1: [(r"^conv 1x1 s1 64->64 out 64x64 ", r" WS1 pre perimg \+res$")]}
_NO_PLANES = [r" PF", r" PW", r" nof32", r"\+resP", r"^pfunpack$"]
_PLANE_FORMS = [(r"^conv 7x1 s1 32->64 ", r" PF LN nof32 \+pf$"),                # the first layer's UF form, its output planes only
                (r"^conv 3x3 s2 64->64 ", r" PF \+pf$"),                          # the stride-2 form
                (r"^conv 1x7 s1 64->21 ", r" PF$"),                               # the row-folded final convolution on planes
                (r"^conv 3x3 s1 ", r" PF LN \+resP$"),                            # a residual read from planes
                r"^pfpack HOIST$"]                                               # hoisted partial sums repacked in accumulator order
FORMS = {
    # (small launches: the default program of B <= 3 at 64 x 64 has no plane kernel; the level-0 folded output runs on the split kernel
    #  at B = 3 and on the few-pixel-block kernel, per-image planes, at B = 1)
    ("full_x", "default"): (_FULL, _NO_PLANES, _L0_OUT),
    ("full_x", "pf0"): (_FULL, _NO_PLANES, _L0_OUT),
    ("full_x", "exact"): ([f for f in _FULL if "WS1" not in str(f) and "pre_add" not in str(f)] + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"]),
    ("full_x", "nohoist"): ([r"^temb$", r"^conv 7x7 s1 67->64 "] + _FINAL, [r"HOIST", r"pre_add", r"^unfold$"]),
    ("full_x", "nofold"): (_FIRST + _FINAL + [r"^ctxr C=64 N=4096 ", (r" WS1 ", _PERIMG)], [r"^ctxf ", r"^kvctx "],
                           {3: [(r"^conv 1x1 s1 64->192 out 64x64 ", r" PW pre$")], 1: [(r"^conv 1x1 s1 64->192 out 64x64 ", r" WS1 pre$")]}),
}
FORMS[("full_eps", "default")] = FORMS[("full_eps", "pf0")] = FORMS[("full_x", "default")]
FORMS[("full_eps", "exact")] = FORMS[("full_x", "exact")]
FORMS[("full_eps", "nohoist")] = ([r"^temb$", r"^conv 7x7 s1 6->64 "] + _FINAL, [r"HOIST", r"pre_add", r"^unfold$"])
FORMS[("full_eps", "nofold")] = FORMS[("full_x", "nofold")]

# 32 x 96 on the six-level model: generic (N % 4 != 0) attention and element-wise LayerNorm at 1 x 3, the few-pixel chain at 2 x 6, a
# folded level 0 whose N = 3072 is no multiple of 2048 (the unfused chain and a folded output on per-image planes)
_RAGGED = _FIRST + _FINAL + [r"^ln C=384 HW=3$", r"^ctxp C=384 N=3 ", r"^ctxr C=320 N=3 ", r"^ctx1 C=320 N=12 ", r"^ctx1 C=128 N=768 ",
                             r"^kstats C=64 N=3072 ", r"^ctxf C=64 N=3072 ", (r"^conv 1x1 s1 384->1152 out 1x3 ", _PRE),
                             r"^conv 3x3 s2 320->320 out 1x3 ", r"^conv 2x2 s1 320->320 out 1x3 ", (r"^conv 2x2 s1 64->64 out 16x48 ", r" LN$")]
FORMS[("ragged_x", "default")] = FORMS[("ragged_x", "pf0")] = (_RAGGED + [(r" WS1 pre perimg \+res$",)], _NO_PLANES)
FORMS[("ragged_x", "exact")] = (_RAGGED + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"])
# channel counts that are no multiple of 16 (16 / 32 / 48 and 24 / 72): the final LayerNorm as statistics + LN on load of the row-folded
# convolution (no final_conv.0 tap: `ups.<n-2>` and `final` are the stages), the unfused folded chain, the split chain
_SMALL = [r"^temb$", (r"^conv 7x7 s1 8->16 ", r" HOIST$"), r"^unfold$", r"^conv 7x1 s1 21->16 ", r"^ln C=16 HW=1024 stats$",
          (r"^conv 1x7 s1 16->21 ", _PRE), r"^combine$", r"^ctxf C=16 N=1024 ", r"^ctxr C=48 N=64 ", (r"^conv 1x1 s1 16->16 out 32x32 ", r" pre \+res$")]
FORMS[("small_x", "default")] = (_SMALL + [(r" WS1 ", _PERIMG)], [r"^pfunpack$"])
FORMS[("small_x", "exact")] = (_SMALL + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"])
_ODD = [r"^temb$", (r"^conv 7x7 s1 5->24 ", r" HOIST$"), r"^unfold$", r"^conv 7x1 s1 21->24 ", r"^ln C=24 HW=960 stats$",
        (r"^conv 1x7 s1 24->21 ", _PRE), r"^combine$", r"^ctxf C=24 N=960 ", r"^ctxr C=72 N=240 ", (r"^conv 1x1 s1 24->24 out 24x40 ", r" pre \+res$"),
        r"^conv 3x3 s1 144->24 out 12x20 "]
FORMS[("odd_x", "default")] = FORMS[("odd_x", "pf0")] = (_ODD, _NO_PLANES)
FORMS[("odd_x", "exact")] = (_ODD + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"])
# the plane forms: small launches forced onto conv_pf_kernel / conv_pw_kernel.  (The fused-phase Upsample, TZ4, needs an input at least
# 32 pixels wide with planes from a pointwise folded attention output: fold128 / fold192 reach it, the 64 x 64 frame does not.)
_TZ4 = r" PF LN nof32 \+pf TZ4$"
FORMS[("full_x", "planes")] = FORMS[("full_eps", "planes")] = (
    [r"^temb$", (r"^conv 7x7 ", r" HOIST$")] + _FINAL + [f for f in _PLANE_FORMS if "s2" not in str(f)] +
    [(r"^conv 3x3 s1 128->128 out 32x32 ", r" PF LN nof32 \+pf \+res$"), r"^kvctx C=64 N=4096 ", r"^ctx1 C=384 N=4 ", (r" WS1 ", _PERIMG)],
    [r"^pfunpack$", r"^unfold$"],                                              # (every planes-only tensor has a plane reader: nothing is unpacked)
    # B = 3: folded PreNorm on the pointwise kernel, its output planes only, read by the stride-2 form; B = 1: the few-pixel-block kernel (fp32 out)
    {3: [(r"^conv 1x1 s1 64->64 out 64x64 ", r" PW pre nof32 \+pf \+res$"), (r"^conv 3x3 s2 64->64 ", r" PF \+pf$")], 1: _L0_OUT[1]})
FORMS[("ragged_x", "planes")] = ([f for f in _PLANE_FORMS if "s2" not in str(f)] + _FINAL + [r"^ln C=384 HW=3$", r"^ctxr C=320 N=3 "], [r"^pfunpack$", r"^unfold$"])
# (no plane form takes 16 / 24-channel layers or rows of fewer than 32 pixels: the switches must leave these programs as they are)
FORMS[("small_x", "planes")] = FORMS[("small_x", "default")]
FORMS[("odd_x", "planes")] = FORMS[("odd_x", "default")]
_F128 = [r"^kvctx C=128 N=2048 ", r"^ctxf C=128 N=2048 ", (r"^conv 1x1 s1 128->128 out 32x64 ", r" pre .*\+res$"), r"^kvctx C=64 N=8192 "] + _FINAL
_F192 = [r"^kstats C=192 N=3072 ", r"^ctxp C=192 N=3072 ", r"^ctxf C=192 N=3072 ", (r"^conv 1x1 s1 192->384 out 48x64 ", _PRE),
         (r"^conv 1x1 s1 192->192 out 48x64 ", r" pre .*\+res$"), r"^kvctx C=64 N=12288 "] + _FINAL
FORMS[("fold128", "default")] = (_F128, [r"^pfunpack$"])
FORMS[("fold192", "default")] = (_F192, [r"^pfunpack$"])
FORMS[("fold128", "exact")] = (_F128 + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"])
FORMS[("fold192", "exact")] = (_F192 + [r" SPLIT2( |$)"], _NO_PLANES + [r"SPLIT2H", r" WS"])
FORMS[("fold128", "planes")] = (_F128 + _PLANE_FORMS, [r"^pfunpack$", r"^unfold$"],
                                {3: [(r"^conv 2x2 s1 64->64 out 32x64 ", _TZ4), (r"^conv 1x1 s1 128->128 out 32x64 ", r" PW pre \+pf \+res$")],
                                 1: [(r"^conv 1x1 s1 128->128 out 32x64 ", r" WS1 pre perimg \+res$")]})
FORMS[("fold192", "planes")] = (_F192 + [f for f in _PLANE_FORMS if "64->64" not in str(f)] +
                                [(r"^conv 3x3 s2 64->64 out 48x64 ", r" PF \+pf$")], [r"^pfunpack$", r"^unfold$"],
                                {3: [(r"^conv 2x2 s1 64->64 out 48x64 ", _TZ4), (r"^conv 1x1 s1 192->192 out 48x64 ", r" PW pre \+pf \+res$")],
                                 1: [(r"^conv 1x1 s1 192->192 out 48x64 ", r" WS1 pre perimg \+res$")]})
assert set(FORMS) == set(RUNS)


def check_forms(labels, forms, batch):
    """(the entries that must be present and that no label matches, the (expression, label) pairs of the absent ones that match)."""
    present, absent = list(forms[0]) + list(forms[2].get(batch, []) if len(forms) > 2 else []), forms[1]
    labels = [re.sub(r"\s+", " ", l).strip() for l in labels]
    def hit(f, l):
        return all(re.search(e, l) for e in ((f,) if isinstance(f, str) else f))
    return [f for f in present if not any(hit(f, l) for l in labels)], [(f, l) for f in absent for l in labels if hit(f, l)]
