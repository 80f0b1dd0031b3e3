#!/usr/bin/env python3
"""Time the e2m1 row quantiser under the block-scale rule `search` (wanq_quant_rows_mx4_search) against the OCP-rule quantisers
(wanq_quant_rows_mx with fmt e2m1, wanq_quant_rows_mx_had32) and a plain device copy of the same bytes, at the 1.3B block's row-wise
shapes: 32760 rows of K = 1536 and K = 8960, bf16 input.  One process, the kernels interleaved round by round, one event pair per
launch; the copy moves what the quantiser must move (rows x K x 2 bytes in, rows x K x 17 / 32 bytes out) and stands for the ceiling.

    python tools/bench_quant_mx4_search.py [--rounds 30] [--out profiles/mx4_scale_search_times.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_gemm_fp8 import interleaved  # noqa: E402
from viditq_extension import fused  # noqa: E402

FP4 = "mxfp4_e2m1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=32760)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_scale_search_times.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_quant_mx4_search.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, bf16 rows, "
             "interleaved launches, one event pair per launch; median us, GB/s = (2 + 17 / 32) rows K / median, spread = (max - min) / "
             "median, of copy = half the copy's median / median (copying the quantiser's bytes reads and writes each of them: twice its traffic; at K = 1536 the copy's 127 MB may stay in the Infinity Cache, which raises this ceiling and lowers every 'of copy' there: compare the column within one K only), ratio = median / median of the OCP-rule entry"]
    for K in (1536, 8960):
        x = torch.randn(a.rows, K, device=dev, generator=g).to(torch.bfloat16)
        n_in, n_out = x.numel(), a.rows * K * 17 // 32 // 2      # in bf16 elements
        dst_in, dst_out = torch.empty(n_in, device=dev, dtype=torch.bfloat16), torch.empty(n_out, device=dev, dtype=torch.bfloat16)
        src_out = x.view(-1)[:n_out]

        def copy():
            dst_in.copy_(x.view(-1))
            dst_out.copy_(src_out)

        runs = {"copy (2 launches; read + write both)": copy}
        for gelu in (False, True):
            for had in (False, True):
                tag = f"{'gelu ' if gelu else ''}{'had32 ' if had else ''}".strip() or "plain"
                runs[f"ocp    {tag}"] = lambda gelu=gelu, had=had: fused.quant_rows_mx(x, FP4, gelu, had)
                runs[f"search {tag}"] = lambda gelu=gelu, had=had: fused.quant_rows_mx4_search(x, gelu, had)
        t = interleaved(runs, a.warmup, a.rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        nbytes = a.rows * K * (2 + 17 / 32)
        lines.append(f"rows {a.rows} K {K}")
        for k, v in t.items():
            base = med["ocp   " + k[6:]] if k.startswith("search") else None
            # the copy reads and writes each byte: its traffic is twice the quantiser's, so its time is halved for the comparison
            ceil = med["copy (2 launches; read + write both)"] / 2
            lines.append(f"  {k:40s} {med[k]:9.1f} us  {nbytes / med[k] / 1e3:8.1f} GB/s  spread {(max(v) - min(v)) / med[k]:.3f}  "
                         f"of copy {ceil / med[k]:.3f}" + (f"  ratio {med[k] / base:.3f}" if base else ""))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
