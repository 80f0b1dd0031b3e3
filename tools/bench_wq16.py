#!/usr/bin/env python3
"""Time the weight-only GEMM (wanq_gemm_wq16, 8 and 4 bit) against the bf16 GEMM (wanq_gemm_bf16) at the Wan Linear shapes, and the
group-wise form (wanq_gemm_wq16_grouped: W4 with groups of 128 and of 64, W8 with groups of 128) against the per-channel kernel
of the same width.

One process, the kernels interleaved round by round (bf16, W8, W4, W4 g128, W4 g64, W8 g128, bf16, ...), so that clock and
temperature drift hit all alike; each sample is one launch between two events after a warm-up; the table gives the median and the spread of the
samples and the ratio of medians to the bf16 GEMM.  bf16 activations, bf16 output, bias, no GELU (the plain Linear).

    python tools/bench_wq16.py [--rounds 30] [--out profiles/wq16_vs_bf16.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from viditq_extension import qgemm  # noqa: E402

SHAPES = [(32760, 1536, 1536), (32760, 8960, 1536), (32760, 1536, 8960), (9450, 5120, 5120), (9450, 13824, 5120)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wq16_vs_bf16.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_wq16.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 activations and output, bias; "
             "interleaved launches, one event pair per launch",
             f"{'M':>6} {'N':>6} {'K':>6} | {'bf16 us':>9} {'TFLOP/s':>8} | {'W8A16 us':>9} {'x bf16':>7} | {'W4A16 us':>9} {'x bf16':>7} | spread (max-min)/median bf16 / W8 / W4 | "
             f"{'W4 g128 us':>10} {'x W4':>6} | {'W4 g64 us':>10} {'x W4':>6} | {'W8 g128 us':>10} {'x W8':>6} | spread g128 / g64 / W8 g128"]
    for M, N, K in SHAPES:
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        c8 = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
        c4 = qgemm.pack_w4(torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8), bias=8)
        zp = torch.randint(-100, 100, (N,), device=dev, generator=g).float()
        zp4 = torch.randint(-8, 8, (N,), device=dev, generator=g).float()
        sw = torch.rand(N, device=dev, generator=g) * 1e-3
        w = ((c8.float() + zp[:, None]) * sw[:, None]).to(torch.bfloat16)
        bias = torch.randn(N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        runs = {"bf16": lambda: qgemm.fp_linear(x, w, bias, out=out),
                "w8": lambda: qgemm.wq16_linear(x, c8, sw, zp, bias, out=out),
                "w4": lambda: qgemm.wq16_linear(x, c4, sw, zp4, bias, out=out, w4=True)}
        for name, codes, gs, z in (("w4g128", c4, 128, zp4), ("w4g64", c4, 64, zp4), ("w8g128", c8, 128, zp)):
            swg = (torch.rand(K // gs, N, device=dev, generator=g) * 1e-3).contiguous()
            zpg = z[torch.randint(0, N, (K // gs, N), device=dev, generator=g)].contiguous()  # integers of the per-channel range
            runs[name] = lambda codes=codes, gs=gs, swg=swg, zpg=zpg: qgemm.wq16_grouped_linear(
                x, codes, swg, zpg, gs, bias, out=out, w4=codes.dtype == torch.uint8)
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
        lines.append(f"{M:>6} {N:>6} {K:>6} | {med['bf16']:>9.1f} {2 * M * N * K / med['bf16'] * 1e-6:>8.1f} | {med['w8']:>9.1f} {med['w8'] / med['bf16']:>7.2f} | "
                     f"{med['w4']:>9.1f} {med['w4'] / med['bf16']:>7.2f} | {spr['bf16']:.2f} / {spr['w8']:.2f} / {spr['w4']:.2f} | "
                     f"{med['w4g128']:>10.1f} {med['w4g128'] / med['w4']:>6.3f} | {med['w4g64']:>10.1f} {med['w4g64'] / med['w4']:>6.3f} | "
                     f"{med['w8g128']:>10.1f} {med['w8g128'] / med['w8']:>6.3f} | {spr['w4g128']:.2f} / {spr['w4g64']:.2f} / {spr['w8g128']:.2f}")
        print(lines[-1], flush=True)
        del x, c8, c4, w, out, runs
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
