"""The preconditions of tests/test_gpu_conv_edges.py, on the CPU (tests/conv_ref.py): the float64 statement against the independent numpy
oracle; the budgets and plane identities that make the exact classes exact, for every shape of conv_ref.FORMS; the float32 restatements of
the three arithmetics in three summation orders -- bit-exact on the exact classes, inside the element-wise bound and the rms limit on the
bound classes; and the wrong kernels (conv_ref.MUTANTS), each of which must LEAVE the check that conv_ref's docstring names for it.  Every
figure is printed (run with -s)."""
import numpy as np
import pytest

import conv_ref as C
from oracle import ops as oops

SHAPES = tuple(dict.fromkeys(shape for _, shape, _ in C.FORMS))
LARGE = 2e9          # multiply-adds of one float64 convolution above which a shape's budget is taken from its worst case alone
ORDERS = ("serial", "blocks", "split8")


def _macs(shape):
    B, Ci, H, W, Co, k, s, p, T, Ho, Wo, Kmax, win = C.geometry(shape)
    return B * Co * Ho * Wo * Kmax


def _ariths(shape):
    return tuple(dict.fromkeys(C.ARITH_OF[f] for _, sh, eps in C.FORMS if sh == shape for f in eps.values()))


def test_family_of_reads_the_per_op_labels():
    labels = {
        "conv 3x3 s1    5->7    out   9x11  MB1 NPW1 WN4 g1 tg0 ipw1 ks1": "mfma",
        "conv 3x3 s1   64->64   out  32x32  MB2 NPW1 WN4 g1 tg1 ipw1 ks1 SPLIT2H LN +res": "split2h",
        "conv 3x3 s1   64->64   out  32x32  MB1 NPW1 WN4 g2 tg3 ipw1 ks1 SPLIT2": "split2",
        "conv 3x3 s2  320->320  out   8x8   MB1 NPW1 WN2 g10 tg3 ipw1 ks1 SPLIT +res": "split",
        "conv 3x3 s1  192->192  out  36x32  MB3 NPW2 WM2 WP4 g1 R5 PF LN +res": "pf",
        "conv 3x3 s2   32->192  out  32x32  MB3 NPW1 WM2 WP4 g1 R5 PF": "pf s2",
        "conv 2x2 s1   32->64   out   8x32  MB2 NPW1 WM1 WP4 g1 R4 PF TZ4": "pf tz4",
        "conv 3x3 s1   64->64   out 128x256 MB2 NPW2 WM1 WP4 g1 R5 PF3 LN +res": "pf3",
        "conv 1x1 s1   64->64   out  36x64  MB2 NPW2 WM1 WP4 g1 R6 PW +res": "pw",
        "conv 3x3 s1   48->32   out   8x8   NPB2 waves3 tiles2 g1 WS": "ws",
        "conv 1x1 s1   48->32   out   8x8   NPB4 waves3 tiles1 g1 WS1 +res": "ws1",
        "ln C=32 HW=64": None, "pfpack": None, "copy": None}
    for label, family in labels.items():
        assert C.family_of(label) == family, label
    assert set(f for _, _, eps in C.FORMS for f in eps.values()) <= set(C.ARITH_OF)
    ids = [C.form_id(f) for f in C.FORMS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("shape", [(2, 5, 9, 11, 7, 3, 1, 1), (1, 4, 12, 10, 6, 3, 2, 1), (1, 3, 10, 9, 4, 7, 1, 3), (2, 6, 5, 5, 9, 1, 1, 0), (2, 5, 6, 7, 4)],
                         ids=C.shape_id)
def test_statement_equals_the_numpy_oracle(shape):
    """conv, S, X1, W1 and K of conv_f64 (torch, float64) against oracle.ops.NumpyOps, an independent float64 restatement; and the
    sampled rows against the full tensors."""
    N = oops.NumpyOps()
    case = C.make_case("normal", shape)
    ref = C.conv_f64(case, shape)
    B, Ci, H, W, Co, k, s, p, T = C.geometry(shape)[:9]
    x, w = case["x"].astype(np.float64), case["w"].astype(np.float64)

    def oracle(xx, ww):
        return np.asarray(N.conv_transpose2d(xx, ww, None, 2, 1) if T else N.conv2d(xx, ww, None, s, p), np.float64)
    one_w = np.ones((w.shape[0], 1) + w.shape[2:]) if T else np.ones((1,) + w.shape[1:])
    for key, xx, ww in (("conv", x, w), ("S", np.abs(x), np.abs(w)), ("X1", np.abs(x), one_w), ("W1", np.ones_like(x[:1]), np.abs(w)),
                        ("K", np.ones_like(x[:1]), one_w)):
        want = oracle(xx, ww)
        err = float(np.abs(ref[key] - want).max() / max(1.0, np.abs(want).max()))
        print(f"[conv-ref] {C.shape_id(shape)} {key}: {err:.2e} from the numpy oracle")
        assert ref[key].shape == want.shape and err < 2e-7, (key, err)            # (the oracle returns float32)
    assert ref["K"].max() == C.geometry(shape)[11] and ref["K"].min() >= 1
    rows = C.sample_rows(case, shape, 256)
    b, co, oy, ox = rows["idx"]
    for ep in ("bias", "sr", "r"):
        y, S = C.rows_f64(rows, ep)
        full = C.statement(ref, case, ep)[b, co, oy, ox]
        assert np.abs(y - full).max() <= 1e-13 * max(1.0, np.abs(full).max()), ep
    assert np.allclose(S, np.broadcast_to(ref["S"], ref["conv"].shape)[b, co, oy, ox], rtol=1e-13)
    assert np.array_equal((rows["a"] != 0).sum(1), np.broadcast_to(ref["K"], ref["conv"].shape)[b, co, oy, ox])


@pytest.mark.parametrize("shape", SHAPES, ids=C.shape_id)
def test_exact_classes_meet_their_budgets_and_plane_identities(shape):
    B, Ci, H, W, Co, k, s, p, T, Ho, Wo, Kmax, win = C.geometry(shape)
    big = _macs(shape) > LARGE
    for cls in C.EXACT_CLASSES:
        case = C.make_case(cls, shape)
        x, w = case["x"], case["w"]
        sc = C.weight_scale(w)
        assert sc == 12, (cls, sc)                                                  # the weight-scale rule on the exact classes
        h, l = (t.astype(np.float64) for t in C.act_planes(x))
        WH, WL, WH2 = (t.astype(np.float64) for t in C.weight_planes(w, sc))
        assert np.array_equal(h + l * 2.0 ** -11, x.astype(np.float64)) or cls == "lround"
        assert np.array_equal(WH2 * 2048.0, WH) and ((np.abs(WH2[WH2 != 0]) >= 2.0 ** -14).all() or cls == "wsmall")      # WH2 exact and normal
        assert np.array_equal((WH + WL) * 2.0 ** -12, w.astype(np.float64))
        a1, a2, a3 = C.split3(x)
        assert np.array_equal(a1.astype(np.float64) + a2 + a3, x.astype(np.float64))
        extras = float(np.abs(case["bias"]).max() + np.abs(case["shift"]).max() + np.abs(case["resid"]).max())
        if cls == "wsmall":
            sub = (WH2 != 0) & (np.abs(WH2) < 2.0 ** -14)
            chan = np.arange(Co) % 4 == 1
            assert sub.any() == (Co > 1) and np.array_equal(np.moveaxis(sub, 1 if T else 0, 0).reshape(Co, -1).any(1), chan & (Co > 1)), "WH2 subnormal in the scaled channels"
            plain = C.make_case("planes", shape)
            assert np.array_equal(plain["x"], x) and np.array_equal(np.moveaxis(w, 1 if T else 0, 0)[~chan], np.moveaxis(plain["w"], 1 if T else 0, 0)[~chan])
            assert np.array_equal(np.moveaxis(w, 1 if T else 0, 0)[chan] * 2.0 ** 18, np.moveaxis(plain["w"], 1 if T else 0, 0)[chan])
            assert np.array_equal(case["resid"][:, chan] * 2.0 ** 18, plain["resid"][:, chan]) and np.array_equal(case["bias"][chan] * 2.0 ** 18, plain["bias"][chan])
            if not big:                        # every statement of the scaled channels is the `planes` one times 2^-18: the same budget
                ra, rb = C.conv_f64(case, shape), C.conv_f64(plain, shape)
                for ep in ("bias", "sr", "r"):
                    ya, yb = C.statement(ra, case, ep), C.statement(rb, plain, ep)
                    assert np.array_equal(ya[:, chan] * 2.0 ** 18, yb[:, chan]) and np.array_equal(ya[:, ~chan], yb[:, ~chan])
                    assert np.array_equal(ya.astype(np.float32).astype(np.float64), ya)
            continue
        if cls == "planes":
            I = C.planes_I(Kmax)
            assert I == (7 if Kmax <= 780 else I) and 3 <= I <= 7 and np.abs(w).max() == 3
            assert set(np.unique(l)) == {-128.0, 0.0, 128.0} and np.array_equal(h % 64, np.zeros_like(h))             # h = 64 i, l' = 128 j
            assert np.abs(h).max() == 64 * I and np.abs(h[h != 0]).min() == 192 and not l[h == 0].any() and not WL.any()
            nnz = Kmax if Kmax <= 1819 else Ci * win * -(-win // C.thin_m(Ci, win, 1819))
            worst = 3 * nnz * (64 * I + 1 / 16) + extras
            assert worst < 2.0 ** 20, worst
            limit = 2.0 ** 20
        elif cls == "wplanes":
            assert np.array_equal(h, x.astype(np.float64)) and not l.any() and set(np.unique(x)) <= {-1.0, 0.0, 1.0}
            assert set(np.unique(WL)) == {-1.0, 0.0, 1.0} and np.abs(w).max() >= 3
            i = np.round(w.astype(np.float64))
            assert np.array_equal(WL[i != 0], ((w - i) * 4096.0)[i != 0])           # WL = j wherever i != 0
            limit = 2.0 ** 12
        else:
            xq = C.lround_input(x)
            assert np.array_equal(xq.astype(np.float32).astype(np.float64), xq) and not WL.any() and np.abs(w).max() == 2
            frac = float((xq != x)[x != 0].mean())
            assert frac > 0.1, frac                                                 # a fifth of the values lose bits to the two planes
            nz = C._conv((x != 0).astype(np.float64), np.ones((w.shape[0], 1) + w.shape[2:]) if T else np.ones((1,) + w.shape[1:]), shape)
            assert nz.max() == 1, nz.max()                                          # one non-zero value per receptive field
            continue
        if not big:
            ref = C.conv_f64(case, shape)
            got = C.budget(ref, case)
            print(f"[conv-ref] {C.shape_id(shape)} {cls}: largest S + |bias| + |shift| + |resid| = {got:.6g} of {limit:g}")
            assert got < limit, (cls, got)
            for ep in ("bias", "sr", "r"):
                y = C.statement(ref, case, ep)
                assert np.array_equal(y.astype(np.float32).astype(np.float64), y), (cls, ep)


@pytest.mark.parametrize("shape", SHAPES, ids=C.shape_id)
def test_restatements_are_bit_exact_on_the_exact_classes(shape):
    """All three arithmetics in all three orders, on 256 sampled output elements (every element of a small output)."""
    for cls in C.EXACT_CLASSES:
        case = C.make_case(cls, shape)
        rows = C.with_scale(C.sample_rows(case, shape, 256, every=512), case)
        for ep in ("bias", "sr"):
            plain = C.rows_f64(rows, ep)[0]
            rounded = C.rows_f64(rows, ep, a=C.lround_input(rows["a"]))[0]
            for arith in C.ARITHS:
                want = rounded if cls == "lround" and arith == "f16x2" else plain
                for order in ORDERS:
                    got = C.emulate(rows, arith, order, ep)
                    assert np.array_equal(got.astype(np.float64), want), (cls, ep, arith, order, int((got != want).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=C.shape_id)
def test_restatements_stay_inside_the_bound_and_the_rms_limit(shape):
    """The bound classes, in the arithmetics this shape's forms run: every order inside the element-wise bound, the blocked orders inside
    2 x the serial figure (the kernels' limit)."""
    for cls in C.BOUND_CLASSES:
        case = C.make_case(cls, shape)
        rows = C.with_scale(C.sample_rows(case, shape, 512), case)
        for arith in _ariths(shape):
            for ep in ("bias", "sr"):
                want, S = C.rows_f64(rows, ep)
                bnd = C.rows_bound(rows, ep, arith, rows["s"])
                fig = {}
                for order in ORDERS:
                    got = C.emulate(rows, arith, order, ep, block=2 if arith == "f32" else 16)
                    fig[order] = (float((np.abs(got - want) / bnd).max()), C.rms_ratio(got, want, S))
                print(f"[conv-ref] {C.shape_id(shape)} {cls} {arith} {ep}: " + ", ".join(f"{o} {f:.3f} of the bound, rms {r:.2e}" for o, (f, r) in fig.items()))
                for order in ORDERS:
                    assert fig[order][0] <= 1.0, (cls, arith, ep, order, fig[order])
                    assert fig[order][1] <= 2 * fig["serial"][1], (cls, arith, ep, order, fig)


# ---- the wrong kernels --------------------------------------------------------------------------------------------------------------
W384 = (2, 384, 32, 32, 128, 1, 1, 0)          # Cin = 384: 24 chunks of 16 channels
W3X3 = (1, 64, 33, 48, 64, 3, 1, 1)


def _exact_misses(cls, shape, mutant, quantum):
    """(elements that differ from the statement, the smallest non-zero error in quanta) of a mutant on an exact class."""
    case = C.make_case(cls, shape)
    rows = C.with_scale(C.sample_rows(case, shape, 512), case)
    want = C.rows_f64(rows, "bias", a=C.lround_input(rows["a"]) if cls == "lround" else None)[0]
    assert np.array_equal(C.emulate(rows, "f16x2", "blocks").astype(np.float64), want)
    err = np.abs(C.emulate(rows, "f16x2", "blocks", mutant=mutant).astype(np.float64) - want)
    n = int((err != 0).sum())
    return n, float(err[err != 0].min() / quantum) if n else 0.0


def _bound_figures(cls, shape, mutant):
    """(worst fraction of the bound, rms / limit) of a mutant in blocked order on a bound class."""
    case = C.make_case(cls, shape)
    rows = C.with_scale(C.sample_rows(case, shape, 512), case)
    want, S = C.rows_f64(rows)
    bnd = C.rows_bound(rows, "bias", "f16x2", rows["s"])
    limit = 2 * C.rms_ratio(C.emulate(rows, "f16x2", "serial"), want, S)
    got = C.emulate(rows, "f16x2", "blocks", mutant=mutant)
    return float((np.abs(got - want) / bnd).max()), C.rms_ratio(got, want, S) / limit


CATCHES = {          # mutant: (the check that must catch it, shape)
    "lp_zero_chunk": ("planes", W384), "acc2_unscaled": ("planes", W384), "drop_hWL": ("wplanes", W384), "lp_trunc": ("lround", W384),
    "wh2_flush": ("wsmall", W384), "ftz": ("tiny", W384)}


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("shape", (W384, W3X3), ids=C.shape_id)
def test_wrong_kernels_leave(mutant, shape):
    """Each restated wrong kernel fails the check conv_ref's docstring names for it, by at least one quantum on an exact class or by
    leaving the element-wise bound; what every OTHER check makes of it is printed (a figure)."""
    assert set(CATCHES) == set(C.MUTANTS)
    by = CATCHES[mutant][0]
    seen = {}
    for cls, quantum in (("planes", 2.0 ** -4), ("wplanes", 2.0 ** -12), ("wsmall", 2.0 ** -22), ("lround", C.TINY)):
        seen[cls] = _exact_misses(cls, shape, mutant, quantum)
    for cls in C.BOUND_CLASSES:
        seen[cls] = _bound_figures(cls, shape, mutant)
    print(f"[conv-ref] {mutant} on {C.shape_id(shape)}: " + ", ".join(f"{c} {n} of 512 differ (least {q:.3g} quanta)" for c, (n, q) in list(seen.items())[:4])
          + "; " + ", ".join(f"{c} {f:.3g} of the bound, rms {r:.3g} of the limit" for c, (f, r) in list(seen.items())[4:]) + f"; caught by {by}")
    if by in C.EXACT_CLASSES:
        n, q = seen[by]
        assert n > 0 and q >= 1.0, (mutant, by, n, q)
    else:
        assert seen[by][0] > 1.0, (mutant, by, seen[by])
    if mutant == "ftz":
        assert seen["tiny"][1] > 1.0, seen["tiny"]
    if mutant == "wh2_flush":
        assert seen["wide_w"][1] > 1.0, seen["wide_w"]
    if mutant == "lp_trunc":                   # the statement of conv_ref's docstring: the rms measure on `normal` does not see it
        assert seen["normal"][1] <= 1.0 and seen["normal"][0] <= 1.0
