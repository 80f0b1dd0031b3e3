#!/usr/bin/env python3
"""Time the group-wise int8 GEMM (wanq_gemm_w8a8_grouped, g = 128: 4-bit asymmetric and 8-bit symmetric weights) against the
per-channel int8 GEMMs of the same width (wanq_gemm_w4a8 / wanq_gemm_w8a8) at the Wan Linear shapes, in two settings of the
per-channel side: automatic kernel selection as qgemm.w8a8_linear makes it (at these M: packed 4-bit codes expanded once per launch,
then the persistent ping-pong kernel) and wanq_gemm_select_kernel(1), the 128 x 128 kernel the grouped one is a sibling of (4 bit:
wanq_gemm_w4a8 itself, nibbles expanded at staging time).

One process, the kernels interleaved round by round, so that clock and temperature drift hit all alike; each sample is one launch
between two events after a warm-up; the table gives the median and the spread of the samples.  bf16 output, bias, no GELU.

    python tools/bench_w8a8_grouped.py [--rounds 30] [--out profiles/w8a8_grouped.txt]

--quality prints instead the 4-bit weight error of StaticQuantizer with and without groups of 128 on a weight with three outlier
columns (the latent PSNR of the shipped configs comes from bench.py --full --quant-config, see profiles/w8a8_grouped_psnr.txt).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from viditq_extension import _C, qgemm  # noqa: E402

SHAPES = [(32760, 1536, 1536), (32760, 8960, 1536), (32760, 1536, 8960), (9450, 5120, 5120), (9450, 13824, 5120), (9450, 5120, 13824)]
GS = 128


def quality():
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer

    w = torch.randn(64, 512, generator=torch.Generator().manual_seed(0)) * 0.02
    w[:, [17, 200, 461]] *= 20.0
    w = w.to("cuda")
    for gs in (None, GS):
        cfg = {"n_bits": 4, "sym": False}
        if gs:
            cfg["group_size"] = gs
        err = ((StaticQuantizer(qcfg.create(cfg))(w) - w).norm() / w.norm()).item()
        print(f"4-bit asymmetric weight error (relative Frobenius), [64, 512] N(0, 0.02^2) with three columns x 20: "
              f"{'groups of %d' % gs if gs else 'per output channel'} {err:.3f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w8a8_grouped.txt"))
    a = ap.parse_args()
    if a.quality:
        return quality()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_w8a8_grouped.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, int8 activations, bf16 output, "
             f"bias; groups of {GS}; interleaved launches, one event pair per launch; TOP/s = 2 M N K / median",
             f"{'M':>6} {'N':>6} {'K':>6} | {'W4 g128 us':>10} {'TOP/s':>7} | {'W4 auto us':>10} {'g / auto':>8} | {'W4 128x128 us':>13} {'g / 128':>7} | "
             f"{'W8 g128 us':>10} {'TOP/s':>7} | {'W8 auto us':>10} {'g / auto':>8} | {'W8 128x128 us':>13} {'g / 128':>7} | "
             "spread (max-min)/median W4 g, auto, 128 / W8 g, auto, 128"]
    for M, N, K in SHAPES:
        x = torch.randint(-127, 128, (M, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
        sa = torch.rand(M, device=dev, generator=g) * 1e-2
        asum = x.float().sum(dim=1) * sa
        c8 = torch.randint(-127, 128, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
        c4 = qgemm.pack_w4(torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8), bias=8)
        sw = torch.rand(N, device=dev, generator=g) * 1e-3
        zp4 = -torch.randint(0, 16, (N,), device=dev, generator=g).float()          # zero_point - 8: u + zp in [-15, 15]
        swg = (torch.rand(K // GS, N, device=dev, generator=g) * 1e-3).contiguous()
        zpg = (-torch.randint(0, 16, (K // GS, N), device=dev, generator=g).float()).contiguous()
        bias = torch.randn(N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

        def v1(name, codes, zp):  # the 128 x 128 kernel on the codes as they are
            prev = _C.lib.wanq_gemm_select_kernel(1)
            try:
                _C.call(name, _C.ptr(x), _C.ptr(codes), _C.ptr(out), _C.BF16, _C.ptr(sa), _C.ptr(asum) if zp is not None else None, _C.F32,
                        _C.ptr(sw), _C.ptr(bias), _C.F32, _C.ptr(zp), _C.F32, None, None, 0, M, N, K, _C.stream())
            finally:
                _C.lib.wanq_gemm_select_kernel(prev)

        runs = {"w4g": lambda: qgemm.w8a8_grouped_linear(x, c4, sa, swg, zpg, GS, bias, torch.bfloat16, out=out, w4=True),
                "w4auto": lambda: qgemm.w8a8_linear(x, c4, sa, sw, bias, asum, zp4, torch.bfloat16, out=out, w4=True),
                "w4v1": lambda: v1("wanq_gemm_w4a8", c4, zp4),
                "w8g": lambda: qgemm.w8a8_grouped_linear(x, c8, sa, swg, None, GS, bias, torch.bfloat16, out=out),
                "w8auto": lambda: qgemm.w8a8_linear(x, c8, sa, sw, bias, out_dtype=torch.bfloat16, out=out),
                "w8v1": lambda: v1("wanq_gemm_w8a8", c8, None)}
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
        tops = lambda k: 2 * M * N * K / med[k] * 1e-6  # noqa: E731
        lines.append(f"{M:>6} {N:>6} {K:>6} | {med['w4g']:>10.1f} {tops('w4g'):>7.1f} | {med['w4auto']:>10.1f} {med['w4g'] / med['w4auto']:>8.2f} | "
                     f"{med['w4v1']:>13.1f} {med['w4g'] / med['w4v1']:>7.2f} | {med['w8g']:>10.1f} {tops('w8g'):>7.1f} | "
                     f"{med['w8auto']:>10.1f} {med['w8g'] / med['w8auto']:>8.2f} | {med['w8v1']:>13.1f} {med['w8g'] / med['w8v1']:>7.2f} | "
                     f"{spr['w4g']:.2f} {spr['w4auto']:.2f} {spr['w4v1']:.2f} / {spr['w8g']:.2f} {spr['w8auto']:.2f} {spr['w8v1']:.2f}")
        print(lines[-1], flush=True)
        del x, c8, c4, out, runs
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
