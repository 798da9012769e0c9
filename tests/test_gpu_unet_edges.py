"""The U-Net's stages on the GPU against the float64 statement of tests/unet_ref.py (which tests/test_unet_ref_host.py pins to the real
reference's float64 run), STAGE-LOCALLY: for every stage of unet_ref.wiring() the library's own tap at the stage's input (cdc_unet_tap;
a planes-only tensor is unpacked to h + l 2^-11, what its reader consumes) goes through unet_ref.stage() on the CPU and is compared with
the library's tap at the stage's output.  Nothing propagates, so a failure names the stage, and the forms that exist only inside a network
program -- folded PreNorm, per-image weights and shifts, hoisted partial sums, planes-only tensors, the unfolded first layer, the
row-folded final convolution and its combine, temb_kernel, the plane unpack behind a tap -- are held to the operator tests' bound.

Bound, per stage, in the project's measure max |got - ref64| / max(1, max |ref64|), taken per image (the worst row is asserted and named):
max(5e-6, 3 e32).  5e-6 is the operator bound of tests/test_gpu_parity.py; e32 (tests/golden/unet_edges.npz, from
tests/golden/make_golden_unet_edges.py) is what the reference's own float32 module loses on that stage against float64 when fed the
float32 rounding of the same input, and 3x is the project's margin over a measured figure: the kernels' operands carry 22-23 significant
bits, so they are granted what float32 is and no more (the wording and the reasoning of tests/test_gpu_attention_edges.py).  The whole
forward is held to max(5e-6, 3 e32_end) against unet_ref.forward.  No bound exceeds 2.7e-5 (`worst_bound` of the fixture, asserted
below TOL_DEC = 5e-5 on the CPU); the bounds come from the reference alone, never from a GPU run.  The PreNorm statistics
(downs.<i>.1.stat_mean / .stat_rstd) are compared with float64 statistics of the GPU's own downs.<i>.1 under ln_ref's element-wise bound
for statistics.

Exact relations: rows 0 and 2 of `rows` are bit-equal at every tap; `dead` is finite at every tap; status() shows the arithmetic the
switch set names, no range fault and no non-finite result (a faulted call is repeated in bf16x3 and would pass on other arithmetic).

Forms are proven: the program's labels must hold every fragment unet_ref.FORMS lists for the configuration and switch set (and none it
excludes), so a case cannot silently stop reaching the form it is named for.  Kernels are chosen only through switches that
test_unet_forward_alternate_kernel_modes (tests/test_gpu_parity.py) already runs.

The new taps: `ups.<i>.0/.1/.2`, `temb` and `final_conv.0` are separate allocations of the program (Builder::new_act / dalloc never
reuse a buffer and no later op writes them in place), so each is tapped and no two stages had to be checked as one -- except that
where the last Upsample's epilogue applied the final LayerNorm, `ups.<n-2>` does not exist and Upsample + LayerNorm is one stage
(`ups.<n-2>.3+final_conv.0`), the 7 x 7 convolution (`final_conv.1`) the next.

Not every case runs under every switch set (unet_ref.RUNS says which and why): the default program and the plane forms take every
case, a switch that replaces one form takes `normal` and the cases aimed at that form.  Every figure is printed before it is asserted
and, with CDC_TEST_OBS=<file>, appended there; the worst fraction of the bound per stage kind and switch set on an MI355X, the forms
seen and the module's wall time are in profiles/unet_edges.md."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import ln_ref
import unet_ref as U
import cdc_compression_amd as cdc
from cdc_compression_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(U.GOLDEN, "unet_edges.npz")


def _obs(what, err, bound):
    print(f"[unet-edges] {what}: {err:.3g} (bound {bound:.3g}, {err / bound:.2f} of it)")
    obs = os.environ.get("CDC_TEST_OBS")
    if obs:
        with open(obs, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "what": what, "relerr": err, "bound": bound}) + "\n")
    return err


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=2)          # the switch sets of a (configuration, case) follow each other below: inputs and forward are computed once
def _case(config_name, case):
    args = U.build(case, config_name)
    assert np.array_equal(U.checksum(args), _golden()[f"{U.entry_key(config_name, case)}/sha"]), "the builder gives other inputs on this host"
    cfg, sd, x, time, ctx = args
    y = U.forward(sd, cfg, x, time, ctx)[0]
    y.setflags(write=False)
    return args, y


def _labels(un):
    L, out = _lib.lib(), []
    for i in range(L.cdc_prof_num_ops(un._h)):
        lab = ctypes.c_char_p()
        L.cdc_prof_op(un._h, i, ctypes.byref(lab), None, None, None)
        out.append(lab.value.decode())
    return out


def _params():
    out = []
    for config_name in U.CONFIGS:
        for case in U.CONFIGS[config_name][3]:
            for sw in U.SWITCHES:
                if case in U.RUNS.get((config_name, sw), ()):
                    out.append(pytest.param(config_name, sw, case, id=f"{config_name}-{sw}-{case}"))
    return out


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("config_name,sw,case", _params())
def test_unet_stage_edge_case(config_name, sw, case, monkeypatch):
    for k, v in U.SWITCHES[sw].items():
        monkeypatch.setenv(k, v)                # (the arithmetic and the switches are read when the handle is created)
    (cfg, sd, x, time, ctx), y_ref = _case(config_name, case)
    g, key = _golden(), U.entry_key(config_name, case)
    un = cdc.Unet(**cfg.kw)
    assert [(n, tuple(s)) for n, s in un.manifest()] == cfg.manifest
    un.load_state_dict(sd)
    arith = 0 if U.SWITCHES[sw].get("CDC_ARITH") == "0" else 1
    assert un.status()["arith"] == arith
    y = un(x, time, ctx)
    st = un.status()
    assert st["nonfinite_results"] == 0 and st["range_faults"] == 0 and st["arith"] == arith, st
    assert y.shape == y_ref.shape and y.dtype == np.float32

    # ---- the forms this switch set is named for are in the program
    labels = _labels(un)
    missing, unwanted = U.check_forms(labels, U.FORMS[(config_name, sw)], x.shape[0])
    print(f"[unet-edges] {config_name} {sw} B={x.shape[0]}: {len(labels)} ops, missing forms {missing}, unwanted {unwanted}")
    assert not missing and not unwanted, (missing, unwanted, labels)

    # ---- every tap of the program
    try:
        un.tap("final_conv.0")
        ln_done = True
    except _lib.CdcError:
        ln_done = False
    wiring = U.wiring(cfg, ln_done)
    taps = {"x": x, "time": time, "y": y, **{f"ctx{l}": c for l, c in enumerate(ctx)}}
    for _, tap, _ in wiring:
        if tap != "y":
            taps[tap] = un.tap(tap)
    mask = U.table_mask(cfg)
    lay, bs = cfg.shift_layout()
    assert taps["temb"].shape == (x.shape[0], 1, 1, bs)
    table = taps["temb"][:, 0, 0, :]

    # ---- stage-local: the GPU's input taps through the float64 stage against the GPU's output tap
    stages, failures = U.stage_names(cfg), []
    for name, tap, ins in wiring:
        inputs = {"x": [taps[i] for i in ins]}
        if name in lay:
            inputs["shift"] = table[:, lay[name][0]:lay[name][0] + lay[name][1]]
        ref, got = U.stage(sd, cfg, name, inputs), taps[tap]
        assert got.shape == ref.shape and got.dtype == np.float32, (name, got.shape, ref.shape)
        if name == "temb":
            ref, got = ref[..., mask], got[..., mask]
        bound = max(U.OP_BOUND, 3 * float(g[f"{key}/e32"][stages.index(name)]))
        assert bound <= U.TOL_DEC
        rows = U.row_errors(got, ref) if np.isfinite(got).all() else np.full(x.shape[0], np.inf)
        err = _obs(f"{config_name} {sw} {case} stage {name}", float(rows.max()), bound)
        if not err <= bound:
            failures.append((name, err, bound, "worst image", int(rows.argmax())))

    # ---- the PreNorm statistics of the convolution epilogue against float64 statistics of the GPU's own tensor
    for i in range(cfg.n):
        v = taps[f"downs.{i}.1"]
        B, C, H, W = v.shape
        mean, rstd, bm, br = ln_ref.final_stats_f64(v.reshape(B, C, 1, H * W))
        for what, want, bnd in (("stat_mean", mean, bm), ("stat_rstd", rstd, br)):
            got = un.tap(f"downs.{i}.1.{what}")
            assert got.shape == (B, 1, H, W) and got.dtype == np.float32
            f = ln_ref.fraction(got.reshape(B, 1, H * W), want, bnd) if np.isfinite(got).all() else np.inf
            print(f"[unet-edges] {config_name} {sw} {case} downs.{i}.1.{what}: worst error {f:.3f} of ln_ref's bound")
            if not f <= 1.0:
                failures.append((f"downs.{i}.1.{what}", f, 1.0))
            taps[f"downs.{i}.1.{what}"] = got

    # ---- end to end
    bound = max(U.OP_BOUND, 3 * float(g[f"{key}/e32_end"]))
    assert bound <= U.TOL_DEC
    rows = U.row_errors(y, y_ref) if np.isfinite(y).all() else np.full(x.shape[0], np.inf)
    err = _obs(f"{config_name} {sw} {case} forward", float(rows.max()), bound)
    if not err <= bound:
        failures.append(("forward", err, bound, "worst image", int(rows.argmax())))

    # ---- exact relations
    outs = {k: (v[..., mask] if k == "temb" else v) for k, v in taps.items() if k not in ("x", "time") and not k.startswith("ctx")}
    if case == "rows":
        failures += [(k, "rows 0 and 2 differ") for k, v in outs.items() if not _bits_equal(v[0], v[2])]
        assert not _bits_equal(y[0], y[1])
    if case == "dead":
        failures += [(k, "not finite") for k, v in outs.items() if not np.isfinite(v).all()]
    st = un.status()
    assert st["nonfinite_results"] == 0 and st["range_faults"] == 0, st
    assert not failures, (config_name, sw, case, failures)
