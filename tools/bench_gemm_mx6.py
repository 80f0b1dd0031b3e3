#!/usr/bin/env python3
"""Time the MXFP6 GEMM (wanq_gemm_mx6: e2m3 activations against e2m3 weights, W6A6, or against e2m1 weights, W4A6) against the W4A4
GEMM (wanq_gemm_mx4) and the MX GEMM with e4m3 activations (wanq_gemm_mx, e4m3 and e2m1 weights) on the per-layer Linear shapes of the
1.3B and the 14B model, the e2m3 activation quantiser against the e4m3 and e2m1 ones, and measure the accumulation error of the
block-scaled instruction with 6-bit operands against the float64 product, in units of the plain-fp32 bound (1.01 K + 3) u S.  On the
same values recoded as e4m3 bytes it records whether wanq_gemm_mx returns the same bits (recorded, not required).

One process, the kernels interleaved round by round (tools/bench_gemm_mx4.py, tools/bench_gemm_fp8.py); bf16 output, bias, no GELU.

    python tools/bench_gemm_mx6.py [--rounds 20] [--out profiles/gemm_mx6.txt]
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

FP6 = "mxfp6_e2m3fn"


def accumulation_error(M, N, K, w_fmt, g):
    """(worst |y - y64| / ((1.01 K + 3) 2^-24 S) over the outputs, whether wanq_gemm_mx gives the same bits on the e2m3 values recoded as
    e4m3 bytes): fp32 output, no bias, random e2m3 codes (every byte pattern is four finite codes), random e2m3 / e2m1 weight codes,
    random scale bytes (the ranges of tests/test_gpu_mx.py::random_operands)"""
    from qdiff.base.base_quantizer import mx_decode

    dev = "cuda"
    a = torch.randint(0, 256, (M, K // 4 * 3), device=dev, generator=g, dtype=torch.uint8)
    w = torch.randint(0, 256, (N, K // 4 * 3 if w_fmt == FP6 else K // 2), device=dev, generator=g, dtype=torch.uint8)
    sa = torch.randint(117, 124, (M, K // 32), device=dev, generator=g, dtype=torch.uint8)
    sw = torch.randint(116, 123, (N, K // 32), device=dev, generator=g, dtype=torch.uint8)
    a64, w64 = mx_decode(a, sa, FP6, torch.float64), mx_decode(w, sw, w_fmt, torch.float64)
    y = qgemm.mx6_linear(a, w, sa, sw, w_fmt, None, torch.float32)
    err = (y.double() - a64 @ w64.T).abs()
    ratio = (err / ((1.01 * K + 3) * 2.0 ** -24 * (a64.abs() @ w64.abs().T))).max().item()
    unit = torch.full_like(sa, 127), torch.full_like(sw, 127)
    as8 = lambda c, s, f: mx_decode(c, s, f, torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)  # noqa: E731 (exact: a subset of e4m3)
    y8 = qgemm.mx_linear(as8(a, unit[0], FP6), as8(w, unit[1], FP6) if w_fmt == FP6 else w, sa, sw, FP8 if w_fmt == FP6 else FP4, None,
                         torch.float32)
    return ratio, torch.equal(y8, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_mx6.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_gemm_mx6.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 output, bias; interleaved "
             "launches, one event pair per launch; median us, T(FL)OP/s = 2 M N K / median, spread = (max - min) / median, ratio = median / "
             "median of wanq_gemm_mx with e4m3 weights (GEMMs) or of the e4m3 MX quantiser (quantisers)"]
    for M, N, K in SHAPES:
        x, w, bias = operands(M, N, K, dev, g)
        a8, s8 = fused.quant_rows_mx(x, FP8)
        a6, s6 = fused.quant_rows_mx(x, FP6)
        a4, s4 = fused.quant_rows_mx(x, FP4)
        w8, sw8 = fused.quant_rows_mx(w, FP8)
        w6, sw6 = fused.quant_rows_mx(w, FP6)
        w4, sw4 = fused.quant_rows_mx(w, FP4)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        runs = {"mx w8a8": lambda: qgemm.mx_linear(a8, w8, s8, sw8, FP8, bias, torch.bfloat16, out=out),
                "mx w4a8": lambda: qgemm.mx_linear(a8, w4, s8, sw4, FP4, bias, torch.bfloat16, out=out),
                "mx4 w4a4": lambda: qgemm.mx4_linear(a4, w4, s4, sw4, bias, torch.bfloat16, out=out),
                "mx6 w6a6": lambda: qgemm.mx6_linear(a6, w6, s6, sw6, FP6, bias, torch.bfloat16, out=out),
                "mx6 w4a6": lambda: qgemm.mx6_linear(a6, w4, s6, sw4, FP4, bias, torch.bfloat16, out=out),
                "quant mxfp8": lambda: fused.quant_rows_mx(x, FP8),
                "quant mxfp6": lambda: fused.quant_rows_mx(x, FP6),
                "quant mxfp4": lambda: fused.quant_rows_mx(x, FP4)}
        times = interleaved(runs, a.warmup, a.rounds)
        ref, qref = statistics.median(times["mx w8a8"]), statistics.median(times["quant mxfp8"])
        nbytes = {"quant mxfp8": 3.0, "quant mxfp6": 2.75, "quant mxfp4": 2.5}   # bf16 in, codes out, per element
        for k, v in times.items():
            med = statistics.median(v)
            quant = k.startswith("quant")
            rate = f"{M * K * nbytes[k] / med * 1e-3:>7.1f} GB/s     " if quant else f"{2 * M * N * K / med * 1e-6:>7.1f} T(FL)OP/s"
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {k:<16} {med:>9.1f} us  {rate}  spread {(max(v) - min(v)) / med:.2f}  "
                         f"ratio {med / (qref if quant else ref):.3f}")
            print(lines[-1], flush=True)
        del x, w, a8, a6, a4, w8, w6, w4, out, runs
    lines.append("# accumulation error of the block-scaled MFMA with 6-bit operands: worst |y - y64| / ((1.01 K + 3) 2^-24 S), fp32 output, random "
                 "codes and random scale bytes; and whether wanq_gemm_mx returns the same bits on the same values recoded as e4m3")
    for M, N, K in ERR_SHAPES:
        for w_fmt, what in ((FP6, "e2m3 x e2m3"), (FP4, "e2m3 x e2m1")):
            ratio, same = accumulation_error(M, N, K, w_fmt, g)
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {what}     err / bound {ratio:.3e}   same bits as wanq_gemm_mx on e4m3 bytes: {same}")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
