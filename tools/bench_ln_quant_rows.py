#!/usr/bin/env python3
"""Time the fused LayerNorm + modulate + fp8 / MX row quantisers (fused.layernorm_quant_rows_*) against the two launches they replace
(fused.layernorm_nobias_t2i_fuse into an fp32 tensor, then fused.quant_rows_*) on the fp32 residual stream of a block.

One process, the candidates interleaved round by round (fused fp8, two-launch fp8, fused MXFP8, ...), so that clock and temperature
drift hit all alike; each sample is one event pair around one candidate (one launch, or the two launches back to back) after a
warm-up; the table gives the medians, their ratio and the spread (max - min) / median of the samples.  Outputs are compared bit for
bit before anything is timed.

    python tools/bench_ln_quant_rows.py [--rounds 50] [--out profiles/ln_quant_rows.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
import torch  # noqa: E402

from viditq_extension import fused  # noqa: E402

ROWS, WIDTHS, EPS = 32760, (1536, 5120), 1e-6
FORMS = {"fp8": ("fp8", {}), "mxfp8": ("mx", {"fmt": "mxfp8_e4m3"}), "mxfp4": ("mx", {"fmt": "mxfp4_e2m1"}), "mxfp4_s": ("mx4_search", {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ln_quant_rows.txt"))
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/bench_ln_quant_rows.py --rounds {a.rounds} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, rows {ROWS}, fp32 x, shift + scale "
             "(norm1 / norm2); interleaved candidates, one event pair per candidate; bytes: x read + codes and scales written",
             f"{'cols':>6} {'form':>8} | {'two-launch us':>13} {'fused us':>9} {'fused / two':>11} {'fused GB/s':>10} | spread (max-min)/median two / fused | bits"]
    for cols in WIDTHS:
        x = torch.randn(ROWS, cols, device=dev, generator=g)
        e = torch.randn(1, 6, cols, device=dev, generator=g) * 0.3
        y = torch.empty_like(x)

        def two(name, args):
            fused.layernorm_nobias_t2i_fuse(y, x, None, e[:, 0], e[:, 1], EPS)
            return getattr(fused, "quant_rows_" + name)(y, **args)

        runs, same, nbytes = {}, {}, {}
        for form, (name, args) in FORMS.items():
            runs[form, "two"] = lambda name=name, args=args: two(name, args)
            runs[form, "fused"] = lambda name=name, args=args: getattr(fused, "layernorm_quant_rows_" + name)(x, None, e[:, 0], e[:, 1], EPS, **args)
            (c, s), (c2, s2) = runs[form, "fused"](), runs[form, "two"]()
            same[form] = bool(torch.equal(c, c2) and torch.equal(s, s2))
            nbytes[form] = x.numel() * 4 + c.numel() + s.numel() * s.element_size()
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
        for form in FORMS:
            t2, tf = med[form, "two"], med[form, "fused"]
            lines.append(f"{cols:>6} {form:>8} | {t2:>13.1f} {tf:>9.1f} {tf / t2:>11.3f} {nbytes[form] / tf * 1e-3:>10.0f} | "
                         f"{spr[form, 'two']:.2f} / {spr[form, 'fused']:.2f} | {'equal' if same[form] else 'DIFFER'}")
            print(lines[-1], flush=True)
        del x, y, runs
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
