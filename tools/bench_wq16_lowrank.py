#!/usr/bin/env python3
"""Time the weight-only GEMM with its low-rank branch (wanq_gemm_wq16_lowrank, R = 64 and 128) and the small GEMM in front of it
(t = x A^T, wanq_gemm_bf16 with N = R) against the entry without the branch, W4, bf16 activations and output, bias, at the six Wan Linear shapes of profiles/gemm_mx.txt:
the group-wise form (groups of 128, against wanq_gemm_wq16_grouped) and the per-channel form (against wanq_gemm_wq16), whose
LOWRANK instantiation holds a second accumulator set that the plain kernel does not (224 VGPRs against 166: two waves per SIMD
instead of three).

One process, the kernels interleaved round by round so that clock and temperature drift hit all alike; each sample is one launch
between two events after a warm-up; the table gives the median and the spread (max - min) / median of the samples, the ratio of the
branch kernel's median to the base kernel's, and the ratio with the t GEMM added (what a layer pays).  The rough expectation is one
more K-tile per 64 ranks, (K + R) / K, plus one more read of x for t.

    python tools/bench_wq16_lowrank.py [--rounds 30] [--out profiles/wq16_lowrank.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from viditq_extension import qgemm  # noqa: E402

TOKENS, GROUP, RANKS = 32760, 128, (64, 128)
SHAPES = [(TOKENS, 1536, 1536), (TOKENS, 8960, 1536), (TOKENS, 1536, 8960),        # 1.3B: q/k/v/o, ffn.0, ffn.2
          (TOKENS, 5120, 5120), (TOKENS, 13824, 5120), (TOKENS, 5120, 13824)]      # 14B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wq16_lowrank.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_wq16_lowrank.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, W4 g{GROUP}, bf16 activations "
             "and output, bias; interleaved launches, one event pair per launch; median us, spread = (max - min) / median; "
             "x base = median / median of wanq_gemm_wq16_grouped (x per-channel: of wanq_gemm_wq16, the per-channel form of both); "
             "layer = (branch GEMM + t GEMM) / base; expect = (K + R) / K"]
    for M, N, K in SHAPES:
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        c4 = qgemm.pack_w4(torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8), bias=8)
        swg = (torch.rand(K // GROUP, N, device=dev, generator=g) * 1e-3).contiguous()
        zpg = torch.randint(-8, 8, (K // GROUP, N), device=dev, generator=g).float().contiguous()
        bias = torch.randn(N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        sw1, zp1 = swg[0].contiguous(), zpg[0].contiguous()
        runs = {"base": lambda: qgemm.wq16_grouped_linear(x, c4, swg, zpg, GROUP, bias, out=out, w4=True),
                "pc": lambda: qgemm.wq16_linear(x, c4, sw1, zp1, bias, out=out, w4=True)}
        for R in RANKS:
            fa = (torch.randn(R, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            fb = (torch.randn(N, R, device=dev, generator=g) * R ** -0.5).to(torch.bfloat16)
            t = qgemm.fp_linear(x, fa)
            runs[f"t{R}"] = lambda fa=fa, t=t: qgemm.fp_linear(x, fa, out=t)
            runs[f"lr{R}"] = lambda t=t, fb=fb: qgemm.wq16_lowrank_linear(x, c4, swg, zpg, GROUP, t, fb, bias, out=out, w4=True)
            runs[f"pclr{R}"] = lambda t=t, fb=fb: qgemm.wq16_lowrank_linear(x, c4, sw1, zp1, None, t, fb, bias, out=out, w4=True)
        times = {k: [] for k in runs}
        for r in range(a.warmup + a.rounds):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        spr = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        lines.append(f"M={M:>6} N={N:>6} K={K:>6} | base          {med['base']:>8.1f} us  spread {spr['base']:.2f}")
        for R in RANKS:
            lines.append(f"M={M:>6} N={N:>6} K={K:>6} | lowrank R={R:<3} {med[f'lr{R}']:>8.1f} us  spread {spr[f'lr{R}']:.2f}  x base "
                         f"{med[f'lr{R}'] / med['base']:.3f}  expect {(K + R) / K:.3f} | t GEMM {med[f't{R}']:>7.1f} us  spread "
                         f"{spr[f't{R}']:.2f} | layer {(med[f'lr{R}'] + med[f't{R}']) / med['base']:.3f}")
        lines.append(f"M={M:>6} N={N:>6} K={K:>6} | per-channel   {med['pc']:>8.1f} us  spread {spr['pc']:.2f}")
        for R in RANKS:
            lines.append(f"M={M:>6} N={N:>6} K={K:>6} | per-ch. R={R:<3}  {med[f'pclr{R}']:>8.1f} us  spread {spr[f'pclr{R}']:.2f}  x per-channel "
                         f"{med[f'pclr{R}'] / med['pc']:.3f}  expect {(K + R) / K:.3f} | layer {(med[f'pclr{R}'] + med[f't{R}']) / med['pc']:.3f}")
        print("\n".join(lines[-2 - 2 * len(RANKS):]), flush=True)
        del x, c4, out, runs
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
