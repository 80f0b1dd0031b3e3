#!/usr/bin/env python3
"""Attention kernel timing at cfg-B (L=32760, 12 heads, d=128): bf16 HIP kernel vs the int8 Q.K^T form (interleaved rounds in
ONE process, median and minimum) vs torch SDPA, plus the quantisation error of the int8 form against the bf16 kernel.

    python tools/bench_attn.py [quick] [--dtype {bf16,fp16}] [--window LEFT RIGHT]...

--dtype fp16 adds the fp16 forms of both kernels to the SAME interleaved rounds (the bf16 ones stay in as the baseline) and prints
the fp16 / bf16 time ratios.

--window LEFT RIGHT (repeatable) times sliding-window self-attention instead: at the cfg-B self-attention shape the dense launch and
one banded launch per window run interleaved in the same rounds on the same operands, and every window prints its time, its ratio
to the dense time beside it and the share of the key tiles a 256-query block walks (the ratio to expect, plus prologue)."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
from wan import ops  # noqa: E402


def attention_sdpa(q, k, v, num_heads):
    """The same contraction through torch SDPA -- a timing reference only."""
    Lq, C = q.shape
    d = C // num_heads
    qh = q.view(1, Lq, num_heads, d).transpose(1, 2)
    kh = k.view(1, k.shape[0], num_heads, d).transpose(1, 2)
    vh = v.view(1, v.shape[0], num_heads, d).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, scale=1.0 / math.sqrt(d))
    return o.transpose(1, 2).reshape(Lq, C)


def time_once(fn, iters=3):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def ab(fns, rounds=7):
    for f in fns.values():
        f()
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            ts[n].append(time_once(f))
    return {n: (sorted(v)[len(v) // 2], min(v)) for n, v in ts.items()}


ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", choices=["quick"], help="quick: the cfg-B self-attention shape only")
ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16", help="fp16: time the fp16 forms against the bf16 ones, interleaved")
ap.add_argument("--window", nargs=2, type=int, action="append", metavar=("LEFT", "RIGHT"),
                help="time ops.attention(window=(LEFT, RIGHT)) against the dense call, interleaved; repeatable")
args = ap.parse_args()
if args.window:
    Lq = Lk = 32760
    H = 12
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.ones(H * 128, device="cuda")
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    q, k = (ops.rmsnorm_rope_(torch.randn(Lq, H * 128, device="cuda", generator=g), w, None, 128).to(dt) for _ in range(2))
    v = torch.randn(Lk, H * 128, device="cuda", generator=g).to(dt)
    fns = {"dense": lambda: ops.attention(q, k, v, H, splits=1)}
    for left, right in args.window:
        fns[f"window({left},{right})"] = lambda left=left, right=right: ops.attention(q, k, v, H, window=(left, right))
    r = ab(fns)
    nt = -(-Lk // 64)
    print(f"{args.dtype} self-attention Lq={Lq} Lk={Lk} H={H}, {nt} key tiles, dense and banded launches interleaved (median / min of 7 rounds x 3)")
    for n, (med, mn) in r.items():
        line = f"{n:22s} median {med*1e3:8.3f} ms  min {mn*1e3:8.3f} ms"
        if n != "dense":
            left, right = (int(x) for x in n[7:-1].split(","))
            span = (left if left >= 0 else Lk) + (right if right >= 0 else Lk) + 256
            tiles = min(nt, span // 64 + 2)  # tiles an interior 256-query block touches (an unaligned band adds one at each end)
            fl = 4.0 * ops.window_pairs(Lq, Lk, (left, right)) * 128 * H
            line += (f"  {fl/med/1e12:7.1f} TFLOP/s over visible pairs  time / dense {med / r['dense'][0]:.3f} (median) "
                     f"{mn / r['dense'][1]:.3f} (min)  band tiles / all tiles <= {tiles / nt:.3f}")
        else:
            line += f"  {4.0 * Lq * Lk * 128 * H / med / 1e12:7.1f} TFLOP/s"
        print(line)
    sys.exit(0)
shapes = [(32760, 32760, 12), (32760, 512, 12), (9450, 75600, 5)]
if args.mode == "quick":
    shapes = shapes[:1]
for (Lq, Lk, H) in shapes:
    g = torch.Generator(device="cuda").manual_seed(0)
    xq = torch.randn(Lq, H * 128, device="cuda", generator=g)
    xk = torch.randn(Lk, H * 128, device="cuda", generator=g)
    v = torch.randn(Lk, H * 128, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.ones(H * 128, device="cuda")
    q, k = ops.rmsnorm_rope_(xq.clone(), w, None, 128).to(torch.bfloat16), ops.rmsnorm_rope_(xk.clone(), w, None, 128).to(torch.bfloat16)
    q8, k8 = ops.rmsnorm_rope_q8(xq, w, None, 128, False), ops.rmsnorm_rope_q8(xk, w, None, 128, True)
    fl = 4.0 * Lq * Lk * 128 * H
    fns = {"bf16": lambda: ops.attention(q, k, v, H), "qk8": lambda: ops.attention_qk8(q8, k8, v, H)}
    if args.dtype == "fp16":
        qh, kh, vh = q.half(), k.half(), v.half()
        fns["fp16"] = lambda: ops.attention(qh, kh, vh, H)
        fns["qk8-fp16"] = lambda: ops.attention_qk8(q8, k8, vh, H)
    r = ab(fns)
    for n, (med, mn) in r.items():
        print(f"{n:5s} attention Lq={Lq} Lk={Lk} H={H}: median {med*1e3:8.3f} ms  min {mn*1e3:8.3f} ms  {fl/med/1e12:7.1f} TFLOP/s "
              f"({fl/med/2.5e15*100:.1f}% of the bf16 MFMA peak)")
    print(f"      qk8 / bf16 time ratio {r['qk8'][0] / r['bf16'][0]:.3f}")
    if args.dtype == "fp16":
        print(f"      fp16 / bf16 time ratio {r['fp16'][0] / r['bf16'][0]:.3f} (median)  {r['fp16'][1] / r['bf16'][1]:.3f} (min)   "
              f"qk8-fp16 / qk8 {r['qk8-fp16'][0] / r['qk8'][0]:.3f} (median)  {r['qk8-fp16'][1] / r['qk8'][1]:.3f} (min)")
        oh = ops.attention(qh, kh, vh, H).float()
        o16_ = ops.attention(q, k, v, H).float()
        print(f"      fp16 vs bf16 kernel: rel L2 {((oh - o16_).norm() / o16_.norm()).item():.3e}")
    o16, o8 = ops.attention(q, k, v, H).float(), ops.attention_qk8(q8, k8, v, H).float()
    print(f"      int8 Q.K^T vs bf16 kernel: rel L2 {((o8 - o16).norm() / o16.norm()).item():.3e}  max abs {(o8 - o16).abs().max().item():.3e}")
    if Lq * Lk <= 32760 * 32760:
        t = time_once(lambda: attention_sdpa(q, k, v, H))
        print(f"sdpa  attention Lq={Lq} Lk={Lk} H={H}: {t*1e3:8.3f} ms {fl/t/1e12:7.1f} TFLOP/s")

if args.mode == "quick":
    sys.exit(0)
# the per-rank shape under 4-way sequence parallelism (3 of 12 heads, all 32760 tokens): 384 workgroups on 256 CUs
Lq = Lk = 32760
for H in (3, 1):
    q = torch.randn(Lq, H * 128, device="cuda").to(torch.bfloat16)
    k = torch.randn(Lk, H * 128, device="cuda").to(torch.bfloat16)
    v = torch.randn(Lk, H * 128, device="cuda").to(torch.bfloat16)
    fl = 4.0 * Lq * Lk * 128 * H
    for s in (1, 2):
        t = time_once(lambda: ops.attention(q, k, v, H, splits=s), 5)
        print(f"hip  attention Lq={Lq} Lk={Lk} H={H} splits={s}: {t*1e3:8.3f} ms {fl/t/1e12:7.1f} TFLOPS")
