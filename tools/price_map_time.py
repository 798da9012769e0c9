"""Timings of region-of-interest coding: the map forms of the RDO kernels beside the scalar forms, and cdc_price_cells, on the shapes of
tools/rdo_time.py.  usage:
    python tools/price_map_time.py run SHAPE [rounds] [out.txt]     SHAPE: b32 (a batch of 32 256 x 256 images) or mp (one 2048 x 2048 image)
    python tools/price_map_time.py trace KERNEL_TRACE.csv [out.txt] the kernel times of a `rocprofv3 --kernel-trace` run of `run`
(profiles/price_map.md holds a run.)

`run` alternates, round by round, the same call without a map and with one -- cdc_entropy_rate_sweep (L = 17), cdc_entropy_encode with
cdc_set_rdo, cdc_op_rdo_quantize -- so that both forms of a kernel see the same state of a shared machine, and prints host-clock call
times.  The kernels alone come from a kernel trace of `run`, taken in a run of its own and summarised by `trace`: per kernel the median
over all dispatches and the medians of four consecutive quarters of them (the spread between repeats of one kernel in one session: the
margin a difference between two kernels has to exceed)."""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def host_timed(f, reps):
    import torch
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        v.append((time.perf_counter() - t0) * 1e6)
    return v


def run(shape, rounds):
    import torch
    import cdc_compression_amd as cdc
    import rate_ref as R
    from cdc_compression_amd import compressor as C
    B, H, W = {"b32": (32, 256, 256), "mp": (1, 2048, 2048)}[shape]
    say(f"device: {torch.cuda.get_device_name(0)}")
    m = cdc.ResnetCompressor(dim=64)                       # the published x-param sizes: CH = CL = 256 (the operands of tools/rdo_time.py)
    dims = tuple(m.reversed_hyper_dims)
    CH, CL = dims[0], dims[-1] // 2
    rng = np.random.default_rng(B * 1000 + H)
    mean_bias = (2.0 * rng.standard_normal(CL)).astype(np.float32)
    m.load_hyper_state_dict({**R.zero_weight_hyper_sd(mean_bias, np.full(CL, 3.0, np.float32), dims=dims), **R.prior_sd(C=CH),
                             "prior._medians": R.medians(CH)})
    hh, wh = H // 64, W // 64
    gh, gw = 4 * hh, 4 * wh
    hyper = (R.medians(CH)[None, :, None, None] + rng.standard_normal((B, CH, hh, wh))).astype(np.float32)
    latent = (mean_bias[None, :, None, None] + 3.0 * rng.standard_normal((B, CL, gh, gw))).astype(np.float32)
    dl, dh = torch.from_numpy(latent).cuda(), torch.from_numpy(hyper).cuda()
    pm = np.exp2(rng.uniform(-3.0, 2.0, (B, H, W))).astype(np.float32)          # one map per image, log-uniform in [1/8, 4]
    dpm = torch.from_numpy(pm).cuda()
    mus = C.RDO_LADDER
    say(f"batch {B} at {H} x {W}: latent {CL} x {gh} x {gw} ({latent[0].size} symbols an image), a price map of {B} x {gh} x {gw} cells")
    cells = m.price_cells(dpm, (H, W), (H, W))
    mean, scale = m.hyper_decode(m.decompress_from_bytes(m.latents_to_bytes(dl, dh), like=dl, return_hyper=True)[1])
    t0, t1 = m._sweep(dl, dh, mus), m._sweep(dl, dh, mus, cells=cells)
    say(f"    the ladder 2^-8 .. 2^8: bits / symbol {t0['bits'][0, 0] / latent[0].size:.3f} -> {t0['bits'][0, -1] / latent[0].size:.3f} without a map, "
        f"-> {t1['bits'][0, -1] / latent[0].size:.3f} under the map; moved at mu = 1: {t0['moved'][0, 8]} / {t1['moved'][0, 8]}")
    ones = m._sweep(dl, dh, mus, cells=np.ones((1, gh, gw), np.float32))
    say(f"    an all-ones map gives the bits of the sweep without one: {all(np.array_equal(ones[k].view(np.int64), t0[k].view(np.int64)) for k in t0)}")
    calls = {"cdc_entropy_rate_sweep L = 17": (lambda: m._sweep(dl, dh, mus), lambda: m._sweep(dl, dh, mus, cells=cells)),
             "latents_to_bytes rdo = 1": (lambda: m.latents_to_bytes(dl, dh, rdo=1.0), lambda: m.latents_to_bytes(dl, dh, rdo=1.0, price_cells=cells)),
             "cdc_op_rdo_quantize": (lambda: m.rdo_quantize(dl, mean, scale, 1.0), lambda: m.rdo_quantize(dl, mean, scale, 1.0, price_cells=cells))}
    times = {k: ([], []) for k in calls}
    cell_times = []
    per = 4
    for _ in range(rounds + 1):                            # (the first round warms up and is dropped)
        for k, (plain, mapped) in calls.items():
            a, b = host_timed(plain, per), host_timed(mapped, per)
            times[k][0].append(a)
            times[k][1].append(b)
        cell_times.append(host_timed(lambda: m.price_cells(dpm, (H, W), (H, W)), per))
    for k, (a, b) in times.items():
        a, b = np.array(a[1:]), np.array(b[1:])
        say(f"    {k:32s} without a map: median {np.median(a):10.1f} us (round medians {np.min(np.median(a, 1)):.1f} .. {np.max(np.median(a, 1)):.1f}); "
            f"with: {np.median(b):10.1f} us ({np.min(np.median(b, 1)):.1f} .. {np.max(np.median(b, 1)):.1f})   whole calls, host clock")
    c = np.array(cell_times[1:])
    say(f"    {'cdc_price_cells':32s} median {np.median(c):10.1f} us ({np.min(np.median(c, 1)):.1f} .. {np.max(np.median(c, 1)):.1f})   "
        f"device map in, {B * gh * gw} cells out (flag read back, copy to a host array)")


def trace(path):
    """Kernel_Name / Start_Timestamp / End_Timestamp of a rocprofv3 kernel trace -> per kernel of interest the medians."""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("kernel_name")
            t = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
            rows.setdefault(name, []).append((float(r["Start_Timestamp"]), t))
    keys = ("latent_symbols_rdo_kernel", "rdo_sweep_kernel", "rdo_quantize_kernel", "price_cells_kernel", "rdo_map_check_kernel",
            "latent_symbols_kernel", "rdo_sweep_sum_kernel")
    say(f"{'kernel':70s} {'n':>5s} {'median us':>10s} {'p10':>8s} {'p90':>8s}   medians of the four quarters of the dispatches")
    for name in sorted(rows):
        if not any(k in name for k in keys):
            continue
        v = np.array([t for _, t in sorted(rows[name])])
        short = name.replace("cdc::(anonymous namespace)::", "").replace("void ", "")
        short = short.split("(")[0][:70]
        q = [np.median(c) for c in np.array_split(v, 4) if c.size]
        say(f"{short:70s} {v.size:5d} {np.median(v):10.1f} {np.percentile(v, 10):8.1f} {np.percentile(v, 90):8.1f}   " + "  ".join(f"{x:.1f}" for x in q))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "run"
    if mode == "trace":
        trace(sys.argv[2])
        out = sys.argv[3] if len(sys.argv) > 3 else None
    else:
        run(sys.argv[2] if len(sys.argv) > 2 else "b32", int(sys.argv[3]) if len(sys.argv) > 3 else 6)
        out = sys.argv[4] if len(sys.argv) > 4 else None
    if out:
        open(out, "w").write("\n".join(lines) + "\n")
