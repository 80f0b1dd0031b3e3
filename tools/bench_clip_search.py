#!/usr/bin/env python3
"""Time the clip search (csrc/clip_search.hip) beside the same search in plain torch on the GPU, g = 128, W4 asymmetric, AWQ's ten
candidates: wanq_clip_search (mse), wanq_clip_search_blocks (hessian) and their torch forms, interleaved in one process after a
warm-up of every shape, device events around `reps` back-to-back calls.  Prints one line per shape; profiles/clip_search.txt keeps
a run.  The torch forms evaluate one candidate at a time (the [R, S, g] tensor of all ten does not fit at the large shapes)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wan2.1-quantization_amd"))
from qdiff.base import base_quantizer as bq  # noqa: E402
from viditq_extension import fused  # noqa: E402

G, BITS, STEPS, S = 128, 4, 20, 10
SHAPES = [(1536, 1536), (8960, 1536), (1536, 8960), (5120, 5120), (13824, 5120), (5120, 13824)]


def torch_search(w, Hb=None):
    rows = w.view(-1, G)
    lo, hi = rows.amin(1, keepdim=True), rows.amax(1, keepdim=True)
    best = None
    for r in bq.clip_ratios(STEPS, S, w.device):
        d, z = bq.clip_params(lo, hi, r, BITS, False)
        e = rows - (torch.clamp(torch.round(rows / d) - z, -8, 7) + z) * d
        if Hb is None:
            obj = (e * e).sum(1)
        else:
            eb = e.view(w.shape[0], -1, G).transpose(0, 1)  # [K / g, N, g]
            obj = (torch.bmm(eb, Hb) * eb).sum(2).t().reshape(-1)
        if best is None:
            best, bd, bz = obj, d[:, 0].clone(), z[:, 0].clone()
        else:
            take = obj < best
            best, bd, bz = torch.where(take, obj, best), torch.where(take, d[:, 0], bd), torch.where(take, z[:, 0], bz)
    return bd, bz


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    for N, K in SHAPES:
        w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
        x = torch.randn(K // G, 256, G, device="cuda", generator=g)
        Hb = torch.bmm(x.transpose(1, 2), x).contiguous()
        forms = {"hip mse": lambda: fused.clip_search(w.view(-1, G), BITS, False, -8, 7, STEPS, S),
                 "torch mse": lambda: torch_search(w),
                 "hip hessian": lambda: fused.clip_search_blocks(w, Hb, BITS, False, -8, 7, STEPS, S),
                 "torch hessian": lambda: torch_search(w, Hb)}
        for fn in forms.values():
            fn()
        d_h, d_t = forms["hip hessian"]()[0], forms["torch hessian"]()[0]
        same = (d_h == d_t).float().mean().item()  # (torch sums in another order: near-ties may choose differently)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn, a.reps))
        print(f"N={N:6d} K={K:6d}  " + "  ".join(f"{k} {min(v):8.3f} ms" for k, v in ms.items()) +
              f"  | mse x{min(ms['torch mse']) / min(ms['hip mse']):.1f}  hessian x{min(ms['torch hessian']) / min(ms['hip hessian']):.1f}"
              f"  same delta as torch on {100 * same:.2f} % of the groups", flush=True)
