#!/usr/bin/env python3
"""Time the W4A16 MXFP4 GEMM (wanq_gemm_wq16_mx, bf16 and fp16 activations) next to the bf16 GEMM (wanq_gemm_bf16), the integer W4A16
GEMM (wanq_gemm_wq16) and its group-wise form with groups of 64 (wanq_gemm_wq16_grouped) at the 1.3B block's Linear shapes.

tools/bench_wq16.py's method: one process, the kernels interleaved round by round so that clock and temperature drift hit all
alike; each sample is one launch between two events after a warm-up; the table gives the median, the spread of the samples and the
ratio of medians.  16-bit output, bias, no GELU (the plain Linear).  The MXFP4 weight is a Gaussian matrix through the block quantiser.

    python tools/bench_wq16_mx.py [--rounds 30] [--out profiles/gemm_wq16_mx_times.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from qdiff.base.base_quantizer import mx_quant_rows  # noqa: E402
from viditq_extension import qgemm  # noqa: E402

SHAPES = [(32760, 1536, 1536), (32760, 8960, 1536), (32760, 1536, 8960)]
ORDER = ("bf16", "w4", "w4g64", "mx_bf16", "mx_fp16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_wq16_mx_times.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_wq16_mx.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, 16-bit output, bias; interleaved "
             "launches, one event pair per launch; median us (spread = (max - min) / median)",
             f"{'M':>6} {'N':>6} {'K':>6} | " + " | ".join(f"{k + ' us':>18}" for k in ORDER) + " | mx_bf16 / bf16, / w4, / w4g64 | mx_fp16 / w4"]
    for M, N, K in SHAPES:
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        xh = x.to(torch.float16)
        w = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
        c4 = qgemm.pack_w4(torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8), bias=8)
        zp4 = torch.randint(-8, 8, (N,), device=dev, generator=g).float()
        sw = torch.rand(N, device=dev, generator=g) * 1e-3
        swg = (torch.rand(K // 64, N, device=dev, generator=g) * 1e-3).contiguous()
        zpg = zp4[torch.randint(0, N, (K // 64, N), device=dev, generator=g)].contiguous()
        cm, sm = mx_quant_rows(w, "mxfp4_e2m1")
        row_exp = qgemm.wq16_mx_row_exp(sm)
        bias = torch.randn(N, device=dev, generator=g)
        w16 = w.to(torch.bfloat16)
        out, outh = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N, device=dev, dtype=torch.float16)
        runs = {"bf16": lambda: qgemm.fp_linear(x, w16, bias, out=out),
                "w4": lambda: qgemm.wq16_linear(x, c4, sw, zp4, bias, out=out, w4=True),
                "w4g64": lambda: qgemm.wq16_grouped_linear(x, c4, swg, zpg, 64, bias, out=out, w4=True),
                "mx_bf16": lambda: qgemm.wq16_mx_linear(x, cm, sm, row_exp, bias, out=out),
                "mx_fp16": lambda: qgemm.wq16_mx_linear(xh, cm, sm, row_exp, bias, out=outh)}
        times = {k: [] for k in ORDER}
        for r in range(a.warmup + a.rounds):
            for k in ORDER:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                runs[k]()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        spr = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        lines.append(f"{M:>6} {N:>6} {K:>6} | " + " | ".join(f"{med[k]:>11.1f} ({spr[k]:.2f})" for k in ORDER) +
                     f" | {med['mx_bf16'] / med['bf16']:.2f}, {med['mx_bf16'] / med['w4']:.3f}, {med['mx_bf16'] / med['w4g64']:.3f} | "
                     f"{med['mx_fp16'] / med['w4']:.3f}")
        print(lines[-1], flush=True)
        del x, xh, w, c4, cm, sm, out, outh, runs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
