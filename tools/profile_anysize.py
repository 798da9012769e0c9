#!/usr/bin/env python3
"""The frame kernels of an any-size compress() beside the part's copy rate and the decode they frame (profiles/anysize.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o anysize -- python tools/profile_anysize.py run
    python tools/profile_anysize.py report DIR > profiles/anysize.txt

`run`: a batch-32 compress() of 500 x 333 uint8 images (full x-param model, synthetic parameters, 65 steps: the reference script's
default), once to warm up (launch plans, graph capture) and once more; then cdc_probe_hbm_copy of the same box.
`report`: per frame kernel of the LAST compress() its duration, the bytes it moves and GB/s, the copy rate, and the sum of all
kernel time between the frame-in and the frame-out launches (the decode and the context model)."""
import csv
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W, STEPS = 32, 500, 333, 65


def run():
    import numpy as np
    import torch
    import cdc_compression_amd as cdc
    from cdc_compression_amd import _lib, synth
    G = os.path.join(ROOT, "tests", "golden")
    um = json.load(open(os.path.join(G, "manifest_full_x.json")))
    un = cdc.Unet(**um["unet_kwargs"])
    un.load_state_dict(synth.unet_state_dict([(a, tuple(b)) for a, b in um["manifest"]], seed=0))
    cm = json.load(open(os.path.join(G, "manifest_encoder_full_x.json")))
    comp = cdc.ResnetCompressor(**cm["kwargs"])
    comp.load_state_dict(synth.unet_state_dict([(k, tuple(v)) for k, v in cm["manifest"]], seed=15))
    diff = cdc.GaussianDiffusionX(un, comp, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    one = np.load(os.path.join(G, "anysize_images.npz"))["w500x333"]
    x = torch.from_numpy(np.repeat(one, B, axis=0)).cuda()
    init = torch.from_numpy(synth.normal("init", (B, 3, H, W), seed=1, std=0.8)).cuda()
    for _ in range(2):
        rec, bpp = diff.compress(x, sample_steps=STEPS, bpp_return_mean=False, init=init)
        torch.cuda.synchronize()
    assert tuple(rec.shape) == (B, 3, H, W)
    gbs = ctypes.c_double()
    assert _lib.lib().cdc_probe_hbm_copy(0, 256 << 20, 5, ctypes.byref(gbs)) == 0
    Hp, Wp = diff.padded_size(H, W)
    print(json.dumps({"hbm_copy_gbs": gbs.value, "B": B, "H": H, "W": W, "Hp": Hp, "Wp": Wp, "steps": STEPS, "bpp0": float(bpp[0]),
                      "status": un.status()}), flush=True)


def report(d):
    trace = [f for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)]
    assert trace, f"no *kernel_trace.csv under {d}"
    rows = []
    for f in trace:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    fin = [i for i, r in enumerate(rows) if "frame_in_kernel" in r[2]]
    fout = [i for i, r in enumerate(rows) if "frame_out_kernel" in r[2]]
    meta = json.loads([line for line in open(os.path.join(d, "run.log")) if line.startswith("{")][-1])
    Hp, Wp = meta["Hp"], meta["Wp"]
    P = 3 * B
    # the last compress(): frame-in of the uint8 images, frame-in (zero fill) of the init, ..., frame-out of the reconstruction
    i_img, i_init, i_out = fin[-2], fin[-1], fout[-1]
    moved = {i_img: P * H * W * 1 + P * Hp * Wp * 4, i_init: P * H * W * 4 + P * Hp * Wp * 4,
             i_out: P * H * ((W + 3) // 4) * 16 + P * H * W * 4}
    what = {i_img: "frame-in  uint8 [32,3,500,333] -> f32 [32,3,512,384], edge", i_init: "frame-in  f32 init -> [32,3,512,384], zero fill",
            i_out: "frame-out f32 [32,3,512,384] -> [32,3,500,333]"}
    print(f"batch-{B} compress() of {H} x {W} uint8 images, full x-param model, {meta['steps']} steps (frame {Hp} x {Wp}); rocprofv3 --kernel-trace")
    print(f"cdc_probe_hbm_copy of the same box (256 MiB float4 copy, read + write): {meta['hbm_copy_gbs']:.0f} GB/s")
    for i in (i_img, i_init, i_out):
        us = (rows[i][1] - rows[i][0]) / 1e3
        print(f"  {what[i]:62s} {us:8.1f} us  {moved[i] / 1e6:7.1f} MB  {moved[i] / us / 1e3:7.0f} GB/s   {rows[i][2][:60]}")
    between = sum(r[1] - r[0] for r in rows[i_init + 1:i_out]) / 1e6
    wall = (rows[i_out][1] - rows[i_img][0]) / 1e6
    frame_ms = sum(rows[i][1] - rows[i][0] for i in (i_img, i_init, i_out)) / 1e6
    print(f"kernel time between them (context model + {meta['steps']}-step decode): {between:.1f} ms in {i_out - i_init - 1} launches; "
          f"first frame launch to last: {wall:.1f} ms; the three frame launches: {frame_ms:.3f} ms = {100 * frame_ms / wall:.3f} % of it")
    print(f"handle status after the run: {meta['status']}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2])
