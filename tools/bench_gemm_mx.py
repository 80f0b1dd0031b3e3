#!/usr/bin/env python3
"""Time the MX GEMM (wanq_gemm_mx: MXFP8 activations x MXFP8 / MXFP4 weights, E8M0 block scales applied by the matrix cores) against the
fp8 GEMM (wanq_gemm_fp8: the same instruction, tile and LDS image with unit scales and fp32 row / channel scales in the epilogue) on the
per-layer Linear shapes of the 1.3B and the 14B model, and measure the accumulation error of the block-scaled instruction against the
float64 product in units of the plain-fp32 bound (1.01 K + 3) u S of tests/test_gpu_fp8.py::bound_case.

One process, the kernels interleaved round by round, so that clock and temperature drift hit all alike; each sample is one launch
between two events after a warm-up; the table gives the median, the spread of the samples and the ratio to the fp8 GEMM.  bf16 output,
bias, no GELU.

    python tools/bench_gemm_mx.py [--rounds 20] [--out profiles/gemm_mx.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_gemm_fp8 import interleaved, operands  # noqa: E402
from viditq_extension import fused, qgemm  # noqa: E402

TOKENS = 32760
SHAPES = [(TOKENS, 1536, 1536), (TOKENS, 8960, 1536), (TOKENS, 1536, 8960),        # 1.3B: q/k/v/o, ffn.0, ffn.2
          (TOKENS, 5120, 5120), (TOKENS, 13824, 5120), (TOKENS, 5120, 13824)]      # 14B
ERR_SHAPES = [(130, 136, 256), (300, 264, 1536), (257, 128, 8960)]
FP8, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"


def accumulation_error(M, N, K, w_fmt, g):
    """worst |y - y64| / ((1.01 K + 3) 2^-24 S) over the outputs, fp32 output, no bias: random finite codes, random scale bytes"""
    from qdiff.base.base_quantizer import mx_decode

    dev = "cuda"
    a = torch.randint(0, 256, (M, K), device=dev, generator=g, dtype=torch.uint8)
    a[(a & 0x7f) == 0x7f] = 0x3c
    w = torch.randint(0, 256, (N, K if w_fmt == FP8 else K // 2), device=dev, generator=g, dtype=torch.uint8)
    if w_fmt == FP8:
        w[(w & 0x7f) == 0x7f] = 0xbc
    sa = torch.randint(117, 124, (M, K // 32), device=dev, generator=g, dtype=torch.uint8)
    sw = torch.randint(116, 123, (N, K // 32), device=dev, generator=g, dtype=torch.uint8)
    a64, w64 = mx_decode(a, sa, FP8, torch.float64), mx_decode(w, sw, w_fmt, torch.float64)
    y = qgemm.mx_linear(a, w, sa, sw, w_fmt, None, torch.float32)
    err = (y.double() - a64 @ w64.T).abs()
    return (err / ((1.01 * K + 3) * 2.0 ** -24 * (a64.abs() @ w64.abs().T))).max().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_mx.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_gemm_mx.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 output, bias; interleaved "
             "launches, one event pair per launch; median us, T(FL)OP/s = 2 M N K / median, spread = (max - min) / median, ratio = median / "
             "median of wanq_gemm_fp8"]
    for M, N, K in SHAPES:
        x, w, bias = operands(M, N, K, dev, g)
        a8, s8 = fused.quant_rows_fp8(x)
        w8, sw8 = fused.quant_rows_fp8(w)
        ax, sx = fused.quant_rows_mx(x, FP8)
        wx8, swx8 = fused.quant_rows_mx(w, FP8)
        wx4, swx4 = fused.quant_rows_mx(w, FP4)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        runs = {"fp8": lambda: qgemm.fp8_linear(a8, w8, s8, sw8, bias, torch.bfloat16, out=out),
                "mxfp8": lambda: qgemm.mx_linear(ax, wx8, sx, swx8, FP8, bias, torch.bfloat16, out=out),
                "mxfp4 w": lambda: qgemm.mx_linear(ax, wx4, sx, swx4, FP4, bias, torch.bfloat16, out=out),
                "quant fp8": lambda: fused.quant_rows_fp8(x),
                "quant mxfp8": lambda: fused.quant_rows_mx(x, FP8)}
        times = interleaved(runs, a.warmup, a.rounds)
        ref = statistics.median(times["fp8"])
        for k, v in times.items():
            med = statistics.median(v)
            quant = k.startswith("quant")
            rate = f"{M * K * 3 / med * 1e-3:>7.1f} GB/s     " if quant else f"{2 * M * N * K / med * 1e-6:>7.1f} T(FL)OP/s"
            ratio = "" if quant else f"  ratio {med / ref:.3f}"
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {k:<12} {med:>9.1f} us  {rate}  spread {(max(v) - min(v)) / med:.2f}{ratio}")
            print(lines[-1], flush=True)
        del x, w, a8, w8, ax, wx8, wx4, out, runs
    lines.append("# accumulation error of the block-scaled MFMA: worst |y - y64| / ((1.01 K + 3) 2^-24 S), fp32 output, random finite codes and "
                 "random scale bytes (tests/test_gpu_mx.py::random_operands)")
    for M, N, K in ERR_SHAPES:
        for w_fmt in (FP8, FP4):
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {w_fmt:<12} err / bound {accumulation_error(M, N, K, w_fmt, g):.4f}")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
