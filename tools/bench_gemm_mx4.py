#!/usr/bin/env python3
"""Time the W4A4 MX GEMM (wanq_gemm_mx4: MXFP4 activations x MXFP4 weights) against the W4A8 MX GEMM (wanq_gemm_mx, e2m1 weights) and the
fp8 GEMM (wanq_gemm_fp8) on the per-layer Linear shapes of the 1.3B and the 14B model, the two e2m1 activation quantisers (plain and
behind the 32-point block Hadamard rotation) against the e4m3 one, and measure the accumulation error of the block-scaled instruction
with both operands e2m1 against the float64 product, in units of the plain-fp32 bound (1.01 K + 3) u S.

One process, the kernels interleaved round by round (tools/bench_gemm_mx.py, tools/bench_gemm_fp8.py); bf16 output, bias, no GELU.

    python tools/bench_gemm_mx4.py [--rounds 20] [--out profiles/gemm_mx4.txt]
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
from bench_gemm_mx import ERR_SHAPES, FP4, FP8, SHAPES  # noqa: E402
from viditq_extension import fused, qgemm  # noqa: E402


def accumulation_error(M, N, K, g):
    """worst |y - y64| / ((1.01 K + 3) 2^-24 S) over the outputs, fp32 output, no bias: random e2m1 codes on both sides, random scale
    bytes (the ranges of tests/test_gpu_mx.py::random_operands)"""
    from qdiff.base.base_quantizer import mx_decode

    dev = "cuda"
    a = torch.randint(0, 256, (M, K // 2), device=dev, generator=g, dtype=torch.uint8)
    w = torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8)
    sa = torch.randint(117, 124, (M, K // 32), device=dev, generator=g, dtype=torch.uint8)
    sw = torch.randint(116, 123, (N, K // 32), device=dev, generator=g, dtype=torch.uint8)
    a64, w64 = mx_decode(a, sa, FP4, torch.float64), mx_decode(w, sw, FP4, torch.float64)
    y = qgemm.mx4_linear(a, w, sa, sw, None, torch.float32)
    err = (y.double() - a64 @ w64.T).abs()
    return (err / ((1.01 * K + 3) * 2.0 ** -24 * (a64.abs() @ w64.abs().T))).max().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_mx4.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_gemm_mx4.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 output, bias; interleaved "
             "launches, one event pair per launch; median us, T(FL)OP/s = 2 M N K / median, spread = (max - min) / median, ratio = median / "
             "median of wanq_gemm_fp8 (GEMMs) or of the e4m3 MX quantiser (quantisers)"]
    for M, N, K in SHAPES:
        x, w, bias = operands(M, N, K, dev, g)
        a8, s8 = fused.quant_rows_fp8(x)
        w8, sw8 = fused.quant_rows_fp8(w)
        ax, sx = fused.quant_rows_mx(x, FP8)
        a4, s4 = fused.quant_rows_mx(x, FP4)
        wx4, swx4 = fused.quant_rows_mx(w, FP4)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        runs = {"fp8": lambda: qgemm.fp8_linear(a8, w8, s8, sw8, bias, torch.bfloat16, out=out),
                "mx w4a8": lambda: qgemm.mx_linear(ax, wx4, sx, swx4, FP4, bias, torch.bfloat16, out=out),
                "mx4 w4a4": lambda: qgemm.mx4_linear(a4, wx4, s4, swx4, bias, torch.bfloat16, out=out),
                "quant mxfp8": lambda: fused.quant_rows_mx(x, FP8),
                "quant mxfp4": lambda: fused.quant_rows_mx(x, FP4),
                "quant mxfp4 h32": lambda: fused.quant_rows_mx(x, FP4, had32=True)}
        times = interleaved(runs, a.warmup, a.rounds)
        ref, qref = statistics.median(times["fp8"]), statistics.median(times["quant mxfp8"])
        for k, v in times.items():
            med = statistics.median(v)
            quant = k.startswith("quant")
            rate = f"{M * K * (3 if k == 'quant mxfp8' else 2.5) / med * 1e-3:>7.1f} GB/s     " if quant else f"{2 * M * N * K / med * 1e-6:>7.1f} T(FL)OP/s"
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {k:<16} {med:>9.1f} us  {rate}  spread {(max(v) - min(v)) / med:.2f}  "
                         f"ratio {med / (qref if quant else ref):.3f}")
            print(lines[-1], flush=True)
        del x, w, a8, w8, ax, a4, wx4, out, runs
    lines.append("# accumulation error of the block-scaled MFMA, e2m1 x e2m1: worst |y - y64| / ((1.01 K + 3) 2^-24 S), fp32 output, random codes "
                 "and random scale bytes")
    for M, N, K in ERR_SHAPES:
        lines.append(f"M={M:>6} N={N:>5} K={K:>5} | e2m1 x e2m1     err / bound {accumulation_error(M, N, K, g):.3e}")
        print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
