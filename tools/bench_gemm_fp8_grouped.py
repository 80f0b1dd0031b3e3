#!/usr/bin/env python3
"""Time the fine-grained fp8 GEMM (wanq_gemm_fp8_grouped: one fp32 scale per 128 input channels on both sides, folded into the fp32
accumulator once per K-tile) against the per-channel one (wanq_gemm_fp8), and the grouped row quantiser (wanq_quant_rows_fp8_grouped)
against the per-row one (wanq_quant_rows_fp8), at 32760 rows on the Linear shapes of the 1.3B and the 14B model.

One process, the kernels interleaved round by round, so that clock and temperature drift hit all alike; each sample is one launch
between two events after a warm-up; the table gives the median, the spread of the samples and the ratio grouped / per-channel.  bf16
output, bias, no GELU.

Then, on the host only (no GPU needed: --host-only), what the format buys: the squared quantisation error of an activation and the
output error of a layer, grouped against per-row fp8, for plain Gaussian activations and for activations with a few channels scaled
by 30-100x.  Synthetic tensors; the effect on a trained checkpoint is not measured here.

    python tools/bench_gemm_fp8_grouped.py [--rounds 25] [--host-only] [--out profiles/gemm_fp8_grouped.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

M = 32760
SHAPES = [(1536, 1536), (8960, 1536), (1536, 8960), (5120, 5120), (13824, 5120), (5120, 13824)]  # (N, K): q/k/v/o, ffn.0, ffn.2


def timed(lines):
    from bench_gemm_fp8 import interleaved
    from viditq_extension import fused, qgemm

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines.append(f"# {torch.cuda.get_device_name(0)}, M = {M}, bf16 output, bias; interleaved launches, one event pair per launch; median us, "
                 "T(FL)OP/s = 2 M N K / median (GB/s = 3 M K / median for the quantisers: bf16 in, codes out), spread = (max - min) / median")
    for N, K in SHAPES:
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
        bias = torch.randn(N, device=dev, generator=g)
        a8, s8 = fused.quant_rows_fp8(x)
        w8, sw8 = fused.quant_rows_fp8(w)
        ag, sg = fused.quant_rows_fp8_grouped(x)
        wg, swg = fused.quant_rows_fp8_grouped(w)
        swg = swg.t().contiguous()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        runs = {"fp8": lambda: qgemm.fp8_linear(a8, w8, s8, sw8, bias, torch.bfloat16, out=out),
                "fp8 g128": lambda: qgemm.fp8_grouped_linear(ag, wg, sg, swg, 128, bias, torch.bfloat16, out=out),
                "quant fp8": lambda: fused.quant_rows_fp8(x),
                "quant fp8 g128": lambda: fused.quant_rows_fp8_grouped(x)}
        med = {}
        for k, v in interleaved(runs, A.warmup, A.rounds).items():
            med[k] = statistics.median(v)
            rate = f"{2 * M * N * K / med[k] * 1e-6:>7.1f} T(FL)OP/s" if not k.startswith("quant") else f"{M * K * 3 / med[k] * 1e-3:>7.1f} GB/s     "
            lines.append(f"N={N:>5} K={K:>5} | {k:<15} {med[k]:>9.1f} us  {rate}  spread {(max(v) - min(v)) / med[k]:.2f}")
            print(lines[-1], flush=True)
        lines.append(f"N={N:>5} K={K:>5} | ratio grouped / per-channel: GEMM {med['fp8 g128'] / med['fp8']:.3f}, quantiser "
                     f"{med['quant fp8 g128'] / med['quant fp8']:.3f}")
        print(lines[-1], flush=True)
        del x, w, a8, w8, ag, wg, out, runs


def host(lines):
    """quantisation error on the host: relative squared error of the decoded activation, and of y = x w^T with both sides quantised"""
    from qdiff.base.base_quantizer import fp8_decode, fp8_group_expand, fp8_quant_rows, fp8_quant_rows_grouped

    def fq(t, grouped):
        if grouped:
            c, s = fp8_quant_rows_grouped(t)
            return fp8_decode(c).double() * fp8_group_expand(s, 128, t.shape[-1]).double()
        c, s = fp8_quant_rows(t)
        return fp8_decode(c).double() * s.double()[:, None]

    g = torch.Generator().manual_seed(0)
    rows, K, N = 512, 1536, 1536
    lines.append(f"# host: x [{rows}, {K}] Gaussian, w [{N}, {K}] Gaussian / sqrt(K); relative squared error ||q - t||^2 / ||t||^2 of the "
                 "decoded activation and of the layer output with both operands quantised; synthetic tensors, no trained checkpoint")
    w = torch.randn(N, K, generator=g) * K ** -0.5
    for name, n_out in (("gaussian", 0), ("8 channels x 30-100", 8)):
        x = torch.randn(rows, K, generator=g)
        if n_out:
            idx = torch.randperm(K, generator=g)[:n_out]
            x[:, idx] *= 30 + 70 * torch.rand(n_out, generator=g)
        y = x.double() @ w.double().t()
        for label, grouped in (("per-row / per-channel", False), ("g128 both sides", True)):
            xq, wq = fq(x, grouped), fq(w, grouped)
            ex = ((xq - x.double()).pow(2).sum() / x.double().pow(2).sum()).item()
            ey = ((xq @ wq.t() - y).pow(2).sum() / y.pow(2).sum()).item()
            lines.append(f"host | {name:<20} {label:<22} activation {ex:.3e}   layer output {ey:.3e}")
            print(lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_fp8_grouped.txt"))
    A = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    out_lines = [f"# tools/bench_gemm_fp8_grouped.py --rounds {A.rounds} --warmup {A.warmup}" + (" --host-only" if A.host_only else "")]
    if not A.host_only:
        timed(out_lines)
    host(out_lines)
    with open(A.out, "w") as f:
        f.write("\n".join(out_lines) + "\n")
