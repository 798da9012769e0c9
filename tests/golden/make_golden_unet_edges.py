#!/usr/bin/env python3
"""Golden digests of the denoising U-Net's stages from the REAL reference on the edge cases of tests/unet_ref.py.

Same rules as make_golden.py, whose `import_reference` this uses: the reference's own `Unet` runs on the PyTorch CPU path and only data
is stored.

    python tests/golden/make_golden_unet_edges.py          # ~3 min; rewrites unet_edges.npz byte for byte

unet_edges.npz, per entry `<configuration>|<case>` of unet_ref.entries():
    <entry>/val      [taps, NSAMPLE]  the reference's float64 run (the model after .double(), forward hooks on its modules) at the sampled
                                      flat indices unet_ref.sample_idx(size), one row per name of unet_ref.tap_names(cfg)
    <entry>/sum      [taps]           the float64 sum of each whole tap
    <entry>/amax     [taps]           max |tap|
    <entry>/e32      [stages]         per name of unet_ref.stage_names(cfg): the reference module in float32, fed the float32 rounding of
                                      its float64 input, against its float64 output: max |y32 - y64| / max(1, max |y64|)
    <entry>/e32_end  the same for the whole float32 forward
    <entry>/sha      sha256 of the regenerated inputs and parameters (unet_ref.checksum); they are not stored
worst_bound: the largest max(5e-6, 3 e32) of any stage or forward of any entry; a case whose bound leaves unet_ref.TOL_DEC is made
milder in unet_ref (and the change recorded there), the bound is never raised.  The statistics taps are those of ln_ref.ln_f64 over the
float64 `downs.<i>.1` (the reference has no such module output).  Written with fixed member dates, uncompressed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: unet_ref
from make_golden import import_reference  # noqa: E402
from make_golden_attention import write_npz  # noqa: E402
import unet_ref as U  # noqa: E402

OUT = os.path.join(HERE, "unet_edges.npz")


def module_of(net, name):
    m = net
    for part in name.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def load(ref, cfg, sd, double):
    net = ref.unet.Unet(**cfg.kw)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == cfg.manifest, cfg.name
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    return net.double() if double else net


def shift_table(net, cfg, time):
    """The library's `temb` tap from the reference's own time_mlp and ResnetBlock.mlp modules."""
    lay, bs = cfg.shift_layout()
    t = net.time_mlp(time)
    out = torch.zeros(time.shape[0], 1, 1, bs, dtype=time.dtype)
    for p, (off, c) in lay.items():
        out[:, 0, 0, off:off + c] = module_of(net, p).mlp(t)
    return out.numpy()


def run_entry(ref, config_name, case):
    args = U.build(case, config_name)
    cfg, sd, x, time, ctx = args
    net64, net32 = load(ref, cfg, sd, True), load(ref, cfg, sd, False)
    io = {}

    def hook(key):
        def fn(m, i, o):
            io[key] = ([t.detach().clone() for t in i], o.detach().clone())
        return fn
    modules = [s for s, _, _ in U.wiring(cfg) if s not in ("temb", "final")] + ["final_conv", "final_conv.0", "final_conv.1"]
    hooks = [module_of(net64, s).register_forward_hook(hook(s)) for s in modules]
    tx, tt, tc = torch.from_numpy(x), torch.from_numpy(time), [torch.from_numpy(c) for c in ctx]
    with torch.no_grad():
        y64 = net64(tx.double(), tt.double(), [c.double() for c in tc]).numpy()
        y32 = net32(tx, tt, tc).numpy()
        taps = {"temb": shift_table(net64, cfg, tt.double()), "y": y64}
        e32 = {"temb": U.relerr(shift_table(net32, cfg, tt), taps["temb"])}
        for s in modules:
            ins, o = io[s]
            taps[s] = o.numpy()
            e32[s] = U.relerr(module_of(net32, s)(*[t.float() for t in ins]).numpy(), o.numpy())
        n = cfg.n
        up = f"ups.{n - 2}.3"
        both = net32.final_conv[0](module_of(net32, up)(io[up][0][0].float())).numpy()
        e32[up + "+final_conv.0"] = U.relerr(both, taps["final_conv.0"])
        e32["final"] = e32.pop("final_conv")
    for h in hooks:
        h.remove()
    for i in range(n - 1):
        taps[f"ups.{i}"] = taps[f"ups.{i}.3"]
    for i in range(n):
        v = taps[f"downs.{i}.1"]
        B, C, H, W = v.shape
        st = U.ln_ref.ln_f64(v.reshape(1, B, C, 1, H * W))
        taps[f"downs.{i}.1.stat_mean"], taps[f"downs.{i}.1.stat_rstd"] = st["mean"].reshape(B, 1, H, W), st["rstd"].reshape(B, 1, H, W)
    assert y32.dtype == np.float32 and all(taps[k].dtype == np.float64 for k in U.tap_names(cfg))
    key = U.entry_key(config_name, case)
    rec = {f"{key}/val": np.stack([taps[k].reshape(-1)[U.sample_idx(taps[k].size)] for k in U.tap_names(cfg)]),
           f"{key}/sum": np.array([taps[k].sum(dtype=np.float64) for k in U.tap_names(cfg)]),
           f"{key}/amax": np.array([np.abs(taps[k]).max() for k in U.tap_names(cfg)]),
           f"{key}/e32": np.array([e32[s] for s in U.stage_names(cfg)]),
           f"{key}/e32_end": np.array(U.relerr(y32, y64)),
           f"{key}/sha": U.checksum(args)}
    mine = U.forward(sd, cfg, x, time, ctx)[1]
    worst = max(max(e32.values()), float(rec[f"{key}/e32_end"]))
    ws = max(e32, key=e32.get)
    print(f"{key:28s} max|tap| {float(rec[f'{key}/amax'].max()):8.2f}  e32_end {float(rec[f'{key}/e32_end']):.3g}  worst stage e32 {e32[ws]:.3g} "
          f"({ws})  |restatement - f64| {max(U.relerr(mine[k], taps[k]) for k in U.tap_names(cfg)):.2g}", flush=True)
    return rec, worst


def main():
    torch.set_num_threads(8)
    rec = {"nsample": np.array(U.NSAMPLE)}
    refs, worst = {}, 0.0
    for config_name, case in U.entries():
        tree = "epsilonparam" if "eps" in config_name else "xparam"
        if tree not in refs:
            refs[tree] = import_reference(tree)
        r, w = run_entry(refs[tree], config_name, case)
        rec.update(r)
        worst = max(worst, w)
    rec["worst_bound"] = np.array(max(U.OP_BOUND, 3 * worst))
    write_npz(OUT, rec)
    print("unet_edges ok:", len(U.entries()), "entries,", os.path.getsize(OUT), "bytes, worst bound", float(rec["worst_bound"]))
    assert float(rec["worst_bound"]) <= U.TOL_DEC, "a case leaves TOL_DEC: make it milder in unet_ref (never raise the bound)"


if __name__ == "__main__":
    main()
