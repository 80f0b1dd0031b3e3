#!/usr/bin/env python3
"""What profiles/gptq.txt holds: for the Linear kinds of the 1.3B block (K = 1536 and K = 8960) and both shipped GPTQ configs' weight
sections (W4 asymmetric, g = 128; the `act:` section does not enter the weight solve), the layer objective GPTQ / round-to-nearest
on synthetic xavier weights and correlated Gaussian inputs, the solver's wall time (gptq_prepare + gptq_solve) against the
round-to-nearest `_requantize` of the same layer, and the time of one Gram accumulation of a calibration pass (3120-token and
32760-token inputs) against the column-absmax hook's.

    python tools/bench_gptq.py [--rows 4] > profiles/gptq.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wan2.1-quantization_amd")]
import torch  # noqa: E402

from qdiff import config as qcfg  # noqa: E402
from qdiff.base import gptq  # noqa: E402
from qdiff.base.base_quantizer import StaticQuantizer  # noqa: E402
from viditq_extension import fused  # noqa: E402

DEV = "cuda:0"
KINDS = [("self_attn.q/k/v/o, cross_attn.*", 1536, 1536), ("ffn.0", 8960, 1536), ("ffn.2", 1536, 8960)]


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4, help="calibration rows per input channel of the synthetic Hessian")
    a = ap.parse_args()
    print(f"# tools/bench_gptq.py on {torch.cuda.get_device_name(0)}; W4 asymmetric g = 128 (the weight section of both shipped GPTQ configs),")
    print(f"# xavier-uniform weights, inputs x = z (I + M / sqrt(K)) with z, M standard normal, {a.rows} K rows; damp 0.01, block 128")
    for kind, N, K in KINDS:
        g = torch.Generator(device=DEV).manual_seed(K + N)
        w = (torch.rand(N, K, generator=g, device=DEV) * 2 - 1) * (6.0 / (N + K)) ** 0.5
        mix = torch.eye(K, device=DEV) + torch.randn(K, K, generator=g, device=DEV) / K ** 0.5
        H = torch.zeros(K, K, device=DEV)
        for _ in range(a.rows):  # K rows at a time through the calibration hook's own accumulation
            fused.gram_accumulate_(H, (torch.randn(K, K, generator=g, device=DEV) @ mix).to(torch.bfloat16))
        q = StaticQuantizer(qcfg.create({"n_bits": 4, "sym": False, "group_size": 128}))
        (_, rtn), t_rtn = timed(lambda: q.codes_and_dequant(w))
        q.init_done = True
        (_, rtn), t_rtn = timed(lambda: q.codes_and_dequant(w), 3)
        (U, w0), t_prep = timed(lambda: gptq.gptq_prepare(H, w, 0.01))
        (codes, deq), t_solve = timed(lambda: gptq.gptq_solve(w0, U, q, 128))
        (codes, deq), t_solve = timed(lambda: gptq.gptq_solve(w0, U, q, 128))
        o_g, o_r = gptq.objective(w, deq, H), gptq.objective(w, rtn, H)
        print(f"{kind:34s} N={N:5d} K={K:5d}  objective GPTQ / RTN {(o_g.sum() / o_r.sum()).item():.4f}  rows improved {int((o_g < o_r).sum())}/{N}  "
              f"worst row {(o_g / o_r).max().item():.4f}  |  RTN _requantize {t_rtn * 1e3:8.2f} ms   GPTQ prepare (fp64 Cholesky) {t_prep * 1e3:9.1f} ms"
              f" + solve {t_solve * 1e3:8.1f} ms")
        del H, U, mix
    print("# calibration: one hook call, H += x^T x (fused.gram_accumulate_) against the column-absmax hook (fused.col_absmax_)")
    for rows in (3120, 32760):
        for C in (1536, 8960):
            x = torch.randn(rows, C, device=DEV).to(torch.bfloat16)
            H, m = torch.zeros(C, C, device=DEV), torch.zeros(C, device=DEV)
            timed(lambda: fused.gram_accumulate_(H, x))
            _, t_g = timed(lambda: fused.gram_accumulate_(H, x), 3)
            _, t_m = timed(lambda: fused.col_absmax_(m, x), 3)
            print(f"rows={rows:6d} C={C:5d}  gram_accumulate_ {t_g * 1e3:8.2f} ms   col_absmax_ {t_m * 1e3:7.3f} ms   H is {C * C * 4 / 1e6:.0f} MB")
            del H, x


if __name__ == "__main__":
    main()
