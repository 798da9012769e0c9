#!/usr/bin/env python3
"""Split decode: ms per DDIM iteration of one chain against two half-batch chains on two streams, over a grid of
batches and frame sizes -- the measurement the default of cdc_set_decode_chains(h, 0) rests on (profiles/split_decode.md).  The full
x-param network, synthetic weights, device tensors; per shape the minimum and the median of `--rounds` decodes of `--steps`
iterations for each setting.  tools/gpu_two_streams.py is the two-handle, two-thread baseline of the same idea.

    timeout -k 10 600 python tools/split_time.py --out profiles/split_time.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cdc_compression_amd as cdc  # noqa: E402
from cdc_compression_amd import synth  # noqa: E402

KW = dict(dim=64, channels=3, context_channels=64, dim_mults=(1, 2, 3, 4, 5, 6), context_dim_mults=(1, 2, 3, 4))
SHAPES = [(2, 256), (4, 256), (8, 256), (16, 256), (24, 256), (32, 256), (48, 256), (32, 128), (64, 128), (4, 512), (8, 512), (16, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    un = cdc.Unet(**KW, device=0)
    un.load_state_dict(synth.unet_state_dict(un.manifest(), seed=0))
    diff = cdc.GaussianDiffusionX(un, None, None, num_timesteps=8193, pred_mode="x", var_schedule="cosine")
    lines = [f"# steps={a.steps} rounds={a.rounds}: B, size, rule, ms/iter one chain (min, median), two chains (min, median), min ratio"]
    for B, S in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * 1000 + S)
        init = torch.randn((B, 3, S, S), generator=g, device=dev) * 0.8
        ctx = [torch.randn((B, c, S >> l, S >> l), generator=g, device=dev) * 0.5 for l, c in enumerate([64, 64, 128, 192])]
        un.set_decode_chains(0)
        rule, res = un.decode_chains(B, S, S), {}
        for chains in (1, 2):
            un.set_decode_chains(chains)
            diff.decompress(ctx, (B, 3, S, S), sample_steps=2, init=init)
            ts = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                diff.decompress(ctx, (B, 3, S, S), sample_steps=a.steps, init=init)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / a.steps)
            res[chains] = (min(ts), statistics.median(ts))
        lines.append(f"B={B:3d} {S}x{S} rule={rule}  one {res[1][0]:7.3f} {res[1][1]:7.3f}   two {res[2][0]:7.3f} {res[2][1]:7.3f}   two/one {res[2][0] / res[1][0]:.4f}")
        print(lines[-1], flush=True)
        del init, ctx
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
