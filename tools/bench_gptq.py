#!/usr/bin/env python3
"""What profiles/gptq.txt holds: for the Linear kinds of the 1.3B block (K = 1536 and K = 8960) and both shipped GPTQ configs' weight
sections (W4 asymmetric, g = 128; the `act:` section does not enter the weight solve), the layer objective GPTQ / round-to-nearest
on synthetic xavier weights and correlated Gaussian inputs, the solver's wall time (gptq_prepare + gptq_solve) against the
round-to-nearest `_requantize` of the same layer, and the time of one Gram accumulation of a calibration pass (3120-token and
32760-token inputs) against the column-absmax hook's; then the one-pass Gram kernel against the two-sided one (interleaved launches),
and act_order against plain GPTQ on inputs with a lognormal channel scale, with the time of wanq_gptq_block_gidx against
wanq_gptq_block on the identity map.

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
    ap.add_argument("--rounds", type=int, default=20, help="rounds of the interleaved A/B timings")
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
    gram_ab(a.rounds)
    act_order(a.rows, a.rounds)


def _events(fns, rounds, warmup=3):
    """{name: [ms per round]}: the variants launched in turn inside every round, one event pair per launch"""
    ms = {k: [] for k in fns}
    for r in range(warmup + rounds):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            if r >= warmup:
                ms[k].append(s.elapsed_time(e))
    return ms


def _med_min(v):
    v = sorted(v)
    return v[len(v) // 2], v[0]


def gram_ab(rounds):
    print("# one hook call, H += x^T x: the one-pass kernel (fused.gram_accumulate_onepass_, upper tile pairs, x read as it lies) against the")
    print(f"# two-sided GEMM on a transposed copy (fused.gram_accumulate_); launches interleaved in one process, {rounds} rounds, median (min) per call")
    for rows in (3120, 32760):
        for C in (1536, 8960):
            x = torch.randn(rows, C, device=DEV).to(torch.bfloat16)
            H1, H2 = torch.zeros(C, C, device=DEV), torch.zeros(C, C, device=DEV)
            ms = _events({"two": lambda: fused.gram_accumulate_(H2, x), "one": lambda: fused.gram_accumulate_onepass_(H1, x)}, rounds)
            (m2, n2), (m1, n1) = _med_min(ms["two"]), _med_min(ms["one"])
            print(f"rows={rows:6d} C={C:5d}  gram_accumulate_ {m2:8.3f} ({n2:8.3f}) ms   gram_accumulate_onepass_ {m1:8.3f} ({n1:8.3f}) ms   "
                  f"one-pass / two-sided {m1 / m2:.3f}")
            del H1, H2, x


def act_order(rows, rounds):
    print("# act_order against plain GPTQ: xavier-uniform weights, inputs x = z (I + M / sqrt(K)) diag(s) with a lognormal channel scale")
    print(f"# s = exp(n), n standard normal (seeded), {rows} K rows; W4 asymmetric g = 128, damp 0.01, block 128; objective in float64")
    for kind, N, K in KINDS:
        g = torch.Generator(device=DEV).manual_seed(K + N + 1)
        w = (torch.rand(N, K, generator=g, device=DEV) * 2 - 1) * (6.0 / (N + K)) ** 0.5
        mix = (torch.eye(K, device=DEV) + torch.randn(K, K, generator=g, device=DEV) / K ** 0.5) * torch.exp(torch.randn(K, generator=g, device=DEV))[None, :]
        H = torch.zeros(K, K, device=DEV)
        for _ in range(rows):
            fused.gram_accumulate_onepass_(H, (torch.randn(K, K, generator=g, device=DEV) @ mix).to(torch.bfloat16))
        d = torch.diagonal(H)
        q = StaticQuantizer(qcfg.create({"n_bits": 4, "sym": False, "group_size": 128}))
        rtn = q.codes_and_dequant(w)[1]
        q.init_done = True
        U, w0 = gptq.gptq_prepare(H, w, 0.01)
        _, plain = gptq.gptq_solve(w0, U, q, 128)
        Up, wp, perm = gptq.gptq_prepare(H, w, 0.01, act_order=True)
        _, ao = gptq.gptq_solve(wp, Up, q, 128, act_order=True, perm=perm)
        o_a, o_p, o_r = (gptq.objective(w, t, H).sum().item() for t in (ao, plain, rtn))
        # the two block kernels on the same problem (the plain order; the identity map), the propagate launches left out
        delta, zp = q.delta.reshape(N, K // 128).contiguous(), q.zero_point.reshape(N, K // 128).contiguous()
        g_idx = (torch.arange(K, device=DEV) // 128).to(torch.int32)
        codes, err = torch.empty(N, K, dtype=torch.int8, device=DEV), torch.empty(N, 128, device=DEV)

        def blocks(gidx):
            ww = w0.clone()
            for c0 in range(0, K, 128):
                if gidx:
                    fused.gptq_block_gidx_(ww, U, delta, zp, g_idx, -8, 7, codes, err, c0, 128)
                else:
                    fused.gptq_block_(ww, U, delta, zp, 128, -8, 7, codes, err, c0, 128)

        ms = _events({"plain": lambda: blocks(False), "gidx": lambda: blocks(True)}, rounds)
        (mp, _), (mg, _) = _med_min(ms["plain"]), _med_min(ms["gidx"])
        print(f"{kind:34s} N={N:5d} K={K:5d}  diag H over {torch.log10(d.max() / d.min()).item():.1f} decades  objective act_order / plain {o_a / o_p:.4f}  "
              f"plain / RTN {o_p / o_r:.4f}  act_order / RTN {o_a / o_r:.4f}  |  {K // 128} block launches: wanq_gptq_block {mp:7.3f} ms  "
              f"wanq_gptq_block_gidx (identity map) {mg:7.3f} ms  ratio {mg / mp:.3f}")
        del H, U, Up, mix


if __name__ == "__main__":
    main()
