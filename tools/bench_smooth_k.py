#!/usr/bin/env python3
"""What K smoothing (attn.qk.smooth_k) costs: the plain int8 k prep (wanq_rmsnorm_rope_q8) against column sums + centred prep
(wanq_rmsnorm_rope_colsum + the division + wanq_rmsnorm_rope_q8_centered) at the 1.3B self-attention shape and at the 14B per-rank
shape of 8-way Ulysses, as interleaved launches with one event pair each (medians reported); and, with --step, bench.py's headline
step on quant_configs/w8a8_all_linears_qk8.yaml with and without the key, alternating in fresh processes on one box.

    python tools/bench_smooth_k.py [--iters 30]
    python tools/bench_smooth_k.py --step [--rounds 2] [--steps 2] [--warmup 1]

The key ships in no YAML (tests/test_linear_dispatch.py pins that directory), so the step child sets it on the loaded config in
memory and then runs bench.py's own main()."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
SHAPES = ((32760, 1536), (75600, 640))


def kernels(iters):
    import torch

    from wan import ops

    for rows, cols in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        k = (torch.randn(rows, cols, device="cuda", generator=g) + 3.0 * torch.randn(cols, device="cuda", generator=g)).to(torch.bfloat16)
        w = torch.rand(cols, device="cuda", generator=g) + 0.5
        rope = torch.randn(rows, 64, 2, device="cuda", generator=g)

        def plain():
            return ops.rmsnorm_rope_q8(k, w, rope, 128, True)

        def colsum():
            return ops.rmsnorm_rope_colsum(k, w, rope, 128)

        def smooth():
            return ops.rmsnorm_rope_q8(k, w, rope, 128, True, center=ops.center_of(ops.rmsnorm_rope_colsum(k, w, rope, 128), rows))

        times = {"plain": [], "colsum": [], "smooth": []}
        for fn in (plain, colsum, smooth):
            fn()
        torch.cuda.synchronize()
        for _ in range(iters):  # interleaved: every launch of one form sits between launches of the others
            for name, fn in (("plain", plain), ("colsum", colsum), ("smooth", smooth)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e) * 1e3)
        # the same launches back to back, 20 inside one event pair: what a launch costs when the GPU never waits for the host
        # (a single launch between two events also counts the host's time to issue it, two kernels and two allocations for colsum)
        b2b = {}
        for name, fn in (("plain", plain), ("colsum", colsum), ("smooth", smooth)):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                fn()
            e.record()
            e.synchronize()
            b2b[name] = s.elapsed_time(e) * 1e3 / 20
        med = {n: statistics.median(t) for n, t in times.items()}
        lo = {n: min(t) for n, t in times.items()}
        mb = rows * cols * 2 / 1e6
        print(f"k prep {rows} x {cols} bf16 ({mb:.0f} MB per read of k), {iters} interleaved launches each, us median (min): "
              f"plain q8 {med['plain']:.1f} ({lo['plain']:.1f}) | colsum alone {med['colsum']:.1f} ({lo['colsum']:.1f}) | "
              f"colsum + division + centred q8 {med['smooth']:.1f} ({lo['smooth']:.1f}) = {med['smooth'] / med['plain']:.2f}x plain, "
              f"+{med['smooth'] - med['plain']:.1f} us per attention || 20 launches back to back in one event pair, us per launch: "
              f"plain q8 {b2b['plain']:.1f} | colsum alone {b2b['colsum']:.1f} | colsum + division + centred q8 {b2b['smooth']:.1f}", flush=True)


def step_child(on, rest):
    from qdiff import config as qcfg

    load = qcfg.load

    def patched(path):
        cfg = load(path)
        if on and cfg.get("attn", None) is not None and cfg["attn"].get("qk", None) is not None:
            cfg["attn"]["qk"]["smooth_k"] = True
        return cfg

    qcfg.load = patched
    import atexit

    from wan import ops

    n, colsum = [0], ops.rmsnorm_rope_colsum
    ops.rmsnorm_rope_colsum = lambda *a, **kw: (n.__setitem__(0, n[0] + 1), colsum(*a, **kw))[1]
    atexit.register(lambda: print(f"smooth_k child: {n[0]} column-sum launches", file=sys.stderr, flush=True))
    sys.path.insert(0, ROOT)
    sys.argv = ["bench.py", "--quant-config", "w8a8_all_linears_qk8.yaml", *rest]
    import bench

    bench.main()


def step(rounds, rest):
    for r in range(rounds):
        for on in (0, 1):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-child", str(on), *rest], capture_output=True, text=True)
            line = next((ln for ln in reversed(out.stdout.splitlines()) if ln.startswith("{")), None)
            if out.returncode != 0 or line is None:
                print(f"round {r} smooth_k={on}: bench.py failed ({out.returncode})\n{out.stderr[-2000:]}", flush=True)
                sys.exit(1)
            res = json.loads(line)
            print(next((ln for ln in out.stderr.splitlines() if ln.startswith("smooth_k child")), "smooth_k child: no count"), flush=True)
            print(f"round {r} smooth_k={on}: " + json.dumps({k: v for k, v in res.items() if not isinstance(v, (dict, list))})[:1200], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-child", dest="step_child", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=2)
    a, rest = ap.parse_known_args()
    if a.step_child is not None:
        step_child(bool(a.step_child), rest)
    elif a.step:
        step(a.rounds, rest or ["--gpus", "1", "--steps", "2", "--warmup", "1"])
    else:
        kernels(a.iters)
