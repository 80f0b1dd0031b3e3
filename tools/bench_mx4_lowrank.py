#!/usr/bin/env python3
"""Time the W4A4 MX GEMM with its low-rank branch (wanq_gemm_mx4_lowrank, R = 64 / 128) against the plain one (wanq_gemm_mx4) on the same
operands, and the fused quantise + project producer (wanq_quant_rows_mx4_project, fp32 and bf16 rows, R = 64 / 192) against the plain
e2m1 quantiser and against the unfused route it replaces -- a 16-bit copy of the row, wanq_gemm_bf16 with N = R, the plain quantiser --
on the per-layer Linear shapes of the 1.3B and the 14B model.

One process, the kernels interleaved round by round (tools/bench_gemm_mx4.py); bf16 output, bias, no GELU.

    python tools/bench_mx4_lowrank.py [--rounds 20] [--out profiles/gemm_mx4_lowrank_times.txt]
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
from bench_gemm_mx import FP4, SHAPES  # noqa: E402
from viditq_extension import fused, qgemm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_mx4_lowrank_times.txt"))
    a = ap.parse_args()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_mx4_lowrank.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 output, bias; "
             "interleaved launches, one event pair per launch; median us, spread = (max - min) / median, ratio = median / median of "
             "wanq_gemm_mx4 (GEMMs) or of the plain e2m1 quantiser on the same rows (producers); `unfused` = 16-bit copy of the row (fp32 "
             "rows only) + wanq_gemm_bf16 with N = R + the plain quantiser, timed as one unit"]
    for M, N, K in SHAPES:
        x, w, bias = operands(M, N, K, dev, g)
        x32, xb = x.float(), x.to(bf)
        a4, s4 = fused.quant_rows_mx(x, FP4)
        w4, sw4 = fused.quant_rows_mx(w, FP4)
        out = torch.empty(M, N, device=dev, dtype=bf)
        A = {R: (torch.randn(R, K, device=dev, generator=g) * K ** -0.5).to(bf) for R in (64, 128, 192)}
        B = {R: (torch.randn(N, R, device=dev, generator=g) * R ** -0.5).to(bf) for R in (64, 128)}
        t = {R: qgemm.fp_linear(xb, A[R]) for R in (64, 128)}

        def unfused(rows, R):
            x16 = rows if rows.dtype == bf else rows.to(bf)
            qgemm.fp_linear(x16, A[R])
            fused.quant_rows_mx(rows, FP4)

        runs = {"mx4": lambda: qgemm.mx4_linear(a4, w4, s4, sw4, bias, bf, out=out),
                "mx4 + lr R=64": lambda: qgemm.mx4_lowrank_linear(a4, w4, s4, sw4, t[64], B[64], bias, bf, out=out),
                "mx4 + lr R=128": lambda: qgemm.mx4_lowrank_linear(a4, w4, s4, sw4, t[128], B[128], bias, bf, out=out)}
        for name, rows in (("f32", x32), ("bf16", xb)):
            runs[f"quant {name}"] = lambda rows=rows: fused.quant_rows_mx(rows, FP4)
            for R in (64, 192):
                runs[f"quant+project {name} R={R}"] = lambda rows=rows, R=R: fused.quant_rows_mxfp4_project(rows, A[R])
                runs[f"unfused {name} R={R}"] = lambda rows=rows, R=R: unfused(rows, R)
        times = interleaved(runs, a.warmup, a.rounds)
        for k, v in times.items():
            med = statistics.median(v)
            ref = "mx4" if k.startswith("mx4") else "quant " + k.split()[1]
            lines.append(f"M={M:>6} N={N:>5} K={K:>5} | {k:<28} {med:>9.1f} us  spread {(max(v) - min(v)) / med:.2f}  "
                         f"ratio {med / statistics.median(times[ref]):.3f}")
            print(lines[-1], flush=True)
        del x, w, x32, xb, a4, w4, out, runs, A, B, t
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
