"""Every convolution family behind Ops.conv2d / Ops.conv_transpose2d on the MI355X against the float64 statement of tests/conv_ref.py:
the exact classes (`planes`, `wplanes`, `wsmall`, `lround`) bit for bit, the bound classes (`normal`, `tiny`, `top`, `wide_w`) inside the
derived element-wise bound and inside the rms limit (2 x the CPU's serial-order restatement of the same case), and `planes` behind
LayerNorm + ReLU + shift + resid inside ln_ref.ln_bound.  The preconditions are tests/test_conv_ref_host.py's.

Every call is held to the kernel family it names: the labels of the ops the call planned are read back (Ops.last_labels) and the family
is asserted from them, and status() must show the arithmetic the form names, no range fault (a faulted call would be repeated in bf16x3
and pass on the wrong arithmetic) and no non-finite result.  conv_ref.FORMS lists, per switch set and shape, the family that runs each
epilogue; every shape and switch set is one that tests/test_gpu_parity.py or tests/test_gpu_determinism.py runs, and no kernel is forced
any other way.  Where a shape the forms were listed for runs another family than expected (conv_ref.FORMS says which), it stays, under
the family it runs, and the nearest shape of the suite that does run the named family is added.

The forms that exist only inside a network program -- folded PreNorm (`pre`), per-image weights (`perimg`), hoisted partial sums
(`pre_add` / HOIST), planes-only outputs, the unfolded first layer and the row-folded 1 x 7 final convolution -- are checked stage by
stage against float64 in tests/test_gpu_unet_edges.py.

Every figure is printed before it is asserted (run with -s): per call the worst element with its error, bound, S and binade, and
r = rms(err / S) against its limit; per family, at the end, the worst fraction of the bound and of the rms limit, whether every exact
call was bit-equal, and the module's wall time.  The MI355X figures are in profiles/conv_edges.md."""
import functools
import time

import numpy as np
import pytest

import conv_ref as C
from cdc_compression_amd.ops import Ops

pytestmark = pytest.mark.gpu

SUMMARY = {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    t0 = time.time()
    yield
    for fam in sorted(SUMMARY):
        s = SUMMARY[fam]
        print(f"[conv-edges] summary {fam} ({C.ARITH_OF[fam]}): {s['calls']} calls; exact classes {s['exact']} bit-equal of {s['exact_calls']}; worst fraction of the "
              f"bound {s['bound']:.3f}, of the LayerNorm bound {s['ln']:.3f}; worst rms {s['rms']:.3f} of its limit"
              + "".join(f"; {c} {s[c][0]:.3f} of the bound, rms {s[c][1]:.3f} of the limit" for c in C.BOUND_CLASSES if c in s))
    print(f"[conv-edges] summary wall time of the module {time.time() - t0:.1f} s")


def note(fam, **kw):
    s = SUMMARY.setdefault(fam, {"calls": 0, "exact": 0, "exact_calls": 0, "bound": 0.0, "ln": 0.0, "rms": 0.0})
    for k, v in kw.items():
        if isinstance(v, tuple):
            s[k] = tuple(max(a, b) for a, b in zip(s.get(k, (0.0, 0.0)), v))
        else:
            s[k] = s[k] + v if k in ("calls", "exact", "exact_calls") else max(s[k], v)


@functools.lru_cache(maxsize=10)                 # the forms of one shape follow each other: a reference is computed once
def _case(cls, shape):
    case = C.make_case(cls, shape)
    ref = C.conv_f64(case, shape)
    if cls in ("planes", "wsmall"):
        assert C.budget(ref, case) < 2.0 ** 20
    if cls == "wplanes":
        assert C.budget(ref, case) < 2.0 ** 12
    return case, ref


@functools.lru_cache(maxsize=4)
def _rounded_conv(shape):
    """The statement of class `lround` in f16x2: the convolution of xq = h + l' 2^-11."""
    case, _ = _case("lround", shape)
    out = C._conv(C.lround_input(case["x"]), case["w"], shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _limit(cls, shape, arith, ep):
    return 2.0 * C.serial_figure(_case(cls, shape)[0], shape, arith, ep)


def _params():
    out = []
    for form in C.FORMS:
        pf3 = "pf3" in form[2].values()
        for cls in C.EXACT_CLASSES + C.BOUND_CLASSES:
            if not pf3 or cls in C.PF3_CLASSES:
                out.append(pytest.param(form, cls, id=f"{C.form_id(form)}-{cls}"))
    return out


def _call(G, case, shape, ep):
    if len(shape) == 5:
        return G.conv_transpose2d(case["x"], case["w"], case["bias"])
    kw = {}
    if ep in ("sr", "ln"):
        kw["shift"] = case["shift"]
    if ep in ("sr", "r", "ln"):
        kw["resid"] = case["resid"]
    if ep == "ln":
        kw.update(ln_g=case["g"], ln_b=case["b"], relu=True)
    return G.conv2d(case["x"], case["w"], case["bias"], shape[6], shape[7], **kw)


@pytest.mark.parametrize("form,cls", _params())
def test_convolution_against_float64(form, cls, monkeypatch):
    env, shape, eps = form
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    G = Ops(0)                                   # (the arithmetic and the switches are read when the handle is created)
    clean = {"arith": 0 if env.get("CDC_ARITH") == "0" else 1, "range_faults": 0, "nonfinite_results": 0}
    assert G.status() == clean, G.status()
    case, ref = _case(cls, shape)
    for ep, family in eps.items():
        if ep == "ln" and cls != "planes":
            continue                             # behind LayerNorm only the exact convolution result has a bound (ln_ref.ln_bound)
        if cls in C.BOUND_CLASSES and cls != "normal" and ep != "bias" and "bias" in eps:
            continue                             # the edge classes once per form; `normal` with every epilogue
        arith = C.ARITH_OF[family]
        tag = f"{C.form_id(form)} {cls} {ep}"
        got = _call(G, case, shape, ep)
        labels = G.last_labels()
        ran = [C.family_of(l) for l in labels if C.family_of(l)]
        print(f"[conv-edges] {tag}: {labels}")
        assert ran == [family], (tag, family, labels)
        if ep == "r" and family == "split2h":    # the stride-2 form at 8 x 8: K in slices and the sum pass behind them
            assert "copy" in labels and " ks1 " not in labels[0], labels
        st = G.status()
        assert st == clean, (tag, st)
        assert got.dtype == np.float32 and got.shape == ref["conv"].shape
        note(family, calls=1)
        if ep == "ln":
            want, bnd = C.statement(ref, case, "ln"), C.bound(ref, case, "ln", arith)
            f, _, line = C.worst(got, want, bnd)
            print(f"[conv-edges] {tag}: {f:.3f} of the LayerNorm bound; {line}")
            note(family, ln=f)
            assert f <= 1.0, (tag, f, line)
        elif cls in C.EXACT_CLASSES:
            conv = _rounded_conv(shape) if cls == "lround" and arith == "f16x2" else ref["conv"]
            want = C.statement({"conv": conv}, case, ep)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
            differ = C.bits(got) != C.bits(want.astype(np.float32))
            differ &= ~((got == 0) & (want == 0))                        # (+0 and -0 are the same result)
            n = int(differ.sum())
            line = "" if not n else "; " + C.worst(got, want, np.where(differ, C.TINY, np.inf), ref["S"])[2]
            print(f"[conv-edges] {tag}: {'bit-equal' if not n else 'NOT bit-equal in %d of %d elements' % (n, differ.size)}{line}")
            note(family, exact_calls=1, exact=int(not n))
            assert not n, (tag, n, line)
        else:
            want, bnd = C.statement(ref, case, ep), C.bound(ref, case, ep, arith)
            f, _, line = C.worst(got, want, bnd, ref["S"])
            r, limit = C.rms_ratio(got, want, np.broadcast_to(ref["S"], want.shape)), _limit(cls, shape, arith, ep)
            with np.errstate(invalid="ignore", divide="ignore"):
                m = float(np.nanmax(np.abs(got - want) / ref["S"]))
            print(f"[conv-edges] {tag}: {f:.3f} of the bound; {line}; largest err / S {m:.3e}; rms(err / S) {r:.3e} = {r / limit:.3f} of the limit {limit:.3e}")
            note(family, bound=f, rms=r / limit)
            note(family, **{cls: (f, r / limit)})
            assert np.isfinite(got).all(), tag
            assert f <= 1.0, (tag, f, line)
            assert r <= limit, (tag, r, limit)
