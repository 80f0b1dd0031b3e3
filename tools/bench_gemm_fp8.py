#!/usr/bin/env python3
"""Time the fp8 GEMM (wanq_gemm_fp8: e4m3 activations x e4m3 weights, per-token and per-channel fp32 scales) against the int8 GEMM
(wanq_gemm_w8a8 under automatic kernel selection, symmetric weights) and the bf16 GEMM (wanq_gemm_bf16) at the FFN shapes of the 1.3B
model, plus the row-wise quantisers in front of the two 8-bit products (wanq_quant_rows_fp8 / wanq_quant_rows on the bf16 activation).

One process, the kernels interleaved round by round, so that clock and temperature drift hit all alike; each sample is one launch
between two events after a warm-up; the table gives the median and the spread of the samples.  bf16 output, bias, no GELU.

    python tools/bench_gemm_fp8.py [--rounds 30] [--out profiles/gemm_fp8.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from viditq_extension import fused, qgemm  # noqa: E402

SHAPES = [(32760, 8960, 1536), (32760, 1536, 8960)]


def interleaved(runs, warmup, rounds):
    """{name: [us per launch]} of the callables in `runs`, called in turn round by round"""
    times = {k: [] for k in runs}
    for r in range(warmup + rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def operands(M, N, K, dev, g):
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    return x, w, torch.randn(N, device=dev, generator=g)


def main(extra_runs=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_fp8.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_gemm_fp8.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 output, bias; interleaved "
             "launches, one event pair per launch; median us, T(FL)OP/s = 2 M N K / median, spread = (max - min) / median"]
    for M, N, K in SHAPES:
        x, w, bias = operands(M, N, K, dev, g)
        a8, s8 = fused.quant_rows_fp8(x)
        w8, sw8 = fused.quant_rows_fp8(w)
        qs = torch.empty(2, M, device=dev)
        ai = fused.quant_sum(x, qs[1], qs[0])
        wq = torch.empty(2, N, device=dev)
        wi = fused.quant_sum(w, wq[1], wq[0])
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        bias16 = bias.to(torch.bfloat16)
        runs = {"fp8": lambda: qgemm.fp8_linear(a8, w8, s8, sw8, bias, torch.bfloat16, out=out),
                "w8a8": lambda: qgemm.w8a8_linear(ai, wi, qs[0], wq[0], bias, out_dtype=torch.bfloat16, out=out),
                "bf16": lambda: qgemm.fp_linear(x, w, bias16, torch.bfloat16, out=out),
                "quant fp8": lambda: fused.quant_rows_fp8(x),
                "quant int8": lambda: fused.quant_sum(x, qs[1], qs[0])}
        if extra_runs is not None:
            runs.update(extra_runs(a8, w8, s8, sw8, bias, out))
        times = interleaved(runs, a.warmup, a.rounds)
        for k, v in times.items():
            med = statistics.median(v)
            rate = f"{2 * M * N * K / med * 1e-6:>7.1f} T(FL)OP/s" if not k.startswith("quant") else f"{M * K * 3 / med * 1e-3:>7.1f} GB/s     "
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {k:<12} {med:>9.1f} us  {rate}  spread {(max(v) - min(v)) / med:.2f}")
            print(lines[-1], flush=True)
        del x, w, a8, w8, ai, wi, out, runs
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
