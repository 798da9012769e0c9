#!/usr/bin/env python3
"""Golden digests of Residual(PreNorm(dim, LinearAttention(dim))) from the REAL reference on the edge cases of tests/attention_ref.py.

Same rules as make_golden.py, whose `import_reference` this uses: the reference's own modules run on the PyTorch CPU path and only data
is stored.

    python tests/golden/make_golden_attention.py          # ~1 min; rewrites attention_edges.npz byte for byte

attention_edges.npz, per entry `<case>|<B>x<C>x<H>x<W>` of attention_ref.fixture_entries() (every case on every shape that
tests/test_gpu_attention_edges.py runs):
    <entry>/val     the reference's float64 output (the module after .double()) at the sampled flat indices `idx/<shape>`
    <entry>/sum     the float64 sum of that whole output
    <entry>/amax    max |y64|
    <entry>/e32     max |y32 - y64| / max(1, max |y64|) of the reference's own float32 run: what plain float32 arithmetic loses
    <entry>/sha     sha256 of the regenerated inputs (attention_ref.checksum); the inputs themselves are not stored
NSAMPLE sampled values per entry, not the 4096 of the model goldens: 90 entries of float64 have to stay below the size limit of a
committed file; the sum covers the elements in between.  The archive is written with fixed member dates, uncompressed."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: attention_ref
from make_golden import import_reference  # noqa: E402
import attention_ref as A  # noqa: E402

NSAMPLE = 1024
OUT = os.path.join(HERE, "attention_edges.npz")


def shape_key(shape):
    return "x".join(str(v) for v in shape)


def reference_module(nc, args, double):
    x, g, b, wq, wo, bo = args
    C = x.shape[1]
    m = nc.Residual(nc.PreNorm(C, nc.LinearAttention(C)))
    with torch.no_grad():
        m.fn.norm.g.copy_(torch.from_numpy(g))
        m.fn.norm.b.copy_(torch.from_numpy(b))
        m.fn.fn.to_qkv.weight.copy_(torch.from_numpy(wq))
        m.fn.fn.to_out.weight.copy_(torch.from_numpy(wo))
        m.fn.fn.to_out.bias.copy_(torch.from_numpy(bo))
    m.eval()
    return m.double() if double else m


def write_npz(path, rec):
    """np.savez without the clock: members in the order given, dated 1980-01-01, stored."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(8)
    nc = import_reference("xparam").nc
    rec = {"nsample": np.array(NSAMPLE)}
    worst = 0.0
    for case, shape in A.fixture_entries():
        args = A.build(case, shape)
        x = torch.from_numpy(args[0])
        with torch.no_grad():
            y32 = reference_module(nc, args, False)(x).numpy()
            y64 = reference_module(nc, args, True)(x.double()).numpy()
        assert y32.dtype == np.float32 and y64.dtype == np.float64 and y64.shape == tuple(shape)
        sk, key = shape_key(shape), A.entry_key(case, shape)
        if f"idx/{sk}" not in rec:
            rec[f"idx/{sk}"] = A.sample_idx(NSAMPLE, y64.size).astype(np.int32)
        e32 = A.relerr(y32, y64)
        rec[f"{key}/val"] = y64.reshape(-1)[rec[f"idx/{sk}"]].copy()
        rec[f"{key}/sum"] = np.array(y64.sum(dtype=np.float64))
        rec[f"{key}/amax"] = np.array(np.abs(y64).max())
        rec[f"{key}/e32"] = np.array(e32)
        rec[f"{key}/sha"] = A.checksum(args)
        worst = max(worst, e32)
        print(f"{key:36s} max|y64| {float(np.abs(y64).max()):9.3f}  e32 {e32:.3g}  |restatement - y64| {A.relerr(A.linear_attention(*args), y64):.2g}")
    write_npz(OUT, rec)
    print("attention_edges ok:", len(A.fixture_entries()), "entries,", os.path.getsize(OUT), "bytes, worst e32", worst)


if __name__ == "__main__":
    main()
