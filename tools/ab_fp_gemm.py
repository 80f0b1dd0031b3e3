#!/usr/bin/env python3
"""A/B of kernel mode's fp_gemm="torch" (torch linear = hipBLASLt, GELU and gate + residual as separate passes) against fp_gemm="hip"
(qgemm.fp_linear: csrc/gemm_bf16.hip with both fused), INTERLEAVED in one process (boxes differ by several per cent).

  1. per shape of the 1.3B block at L = 32760, the cross-attention k / v on the 512-token context and the 14B per-rank shapes:
     the plain product (+ bias) in us and as a fraction of the 2.5 PFLOP/s bf16 dense nominal, then the fused sequences
     (ffn.0 + GELU; ffn.2 / o + gate + residual into the fp32 stream) against torch's linear + the separate pass;
  2. one kernel-mode block of the shipped configuration (ViDiT W8A8 on self_attn q / k / v, the other seven Linears FP) at
     L = 32760, ms per block.
Each number is the median over rounds of (device-event time of REPS back-to-back calls) / REPS, the arms alternating inside a round.
usage: python tools/ab_fp_gemm.py [--rounds 7] [--no-block]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wan2.1-quantization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from viditq_extension import fused, qgemm  # noqa: E402

DEV = "cuda"
PEAK = 2.5e15
# (label, M, N, K, kind): kind 'plain' = + bias; 'gelu' = + bias, GELU, bf16 out; 'gres' = + bias, gate + residual into fp32
SHAPES = [
    ("1.3B q/o  [32760,1536]x1536", 32760, 1536, 1536, "gres"),
    ("1.3B ffn0 [32760,1536]x8960", 32760, 8960, 1536, "gelu"),
    ("1.3B ffn2 [32760,8960]x1536", 32760, 1536, 8960, "gres"),
    ("1.3B cross k/v [512,1536]x1536", 512, 1536, 1536, "plain"),
    ("14B  o    [9450,5120]x5120", 9450, 5120, 5120, "gres"),
    ("14B  ffn0 [9450,5120]x13824", 9450, 13824, 5120, "gelu"),
    ("14B  ffn2 [9450,13824]x5120", 9450, 5120, 13824, "gres"),
    ("14B  o    [75600,5120]x5120", 75600, 5120, 5120, "gres"),
    ("14B  ffn0 [75600,5120]x13824", 75600, 13824, 5120, "gelu"),
    ("14B  ffn2 [75600,13824]x5120", 75600, 5120, 13824, "gres"),
]


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps  # us


def ab(arms, rounds, reps):
    """arms: {name: fn}; warm each, then `rounds` rounds alternating the arms -> {name: median us}"""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for r in range(rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            t[k].append(timed(arms[k], reps))
    return {k: statistics.median(v) for k, v in t.items()}


def gemm_section(rounds):
    print("## 1. products (median us per call; fraction of the 2.5 PFLOP/s bf16 nominal)")
    print(f"{'shape':34s} {'torch lin':>10s} {'hip':>10s} {'hip/pk':>7s} {'torch/pk':>8s} | {'fused kind':10s} {'torch seq':>10s} {'hip fused':>10s} {'speedup':>7s}")
    for label, M, N, K, kind in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(M + N + K)
        x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
        b = (torch.randn(N, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
        flop = 2.0 * M * N * K
        reps = max(2, min(50, int(2e13 / flop)))
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        plain = ab({"torch": lambda: torch.nn.functional.linear(x, w, b), "hip": lambda: qgemm.fp_linear(x, w, b, out=y)}, rounds, reps)
        line = (f"{label:34s} {plain['torch']:10.1f} {plain['hip']:10.1f} {flop / plain['hip'] * 1e6 / PEAK:7.3f} "
                f"{flop / plain['torch'] * 1e6 / PEAK:8.3f} | ")
        if kind == "gelu":
            seq = ab({"torch": lambda: torch.nn.functional.gelu(torch.nn.functional.linear(x, w, b), approximate="tanh"),
                      "hip": lambda: qgemm.fp_linear(x, w, b, gelu=True, out=y)}, rounds, reps)
            line += f"{'+GELU':10s} {seq['torch']:10.1f} {seq['hip']:10.1f} {seq['torch'] / seq['hip']:7.3f}"
        elif kind == "gres":
            res = torch.randn(M, N, device=DEV, generator=g)
            gate = torch.rand(N, device=DEV, generator=g) * 0.01  # small: the stream stays bounded over many in-place calls

            def torch_seq():
                fused.gate_residual_into_(res, torch.nn.functional.linear(x, w, b), gate.view(1, -1))

            seq = ab({"torch": torch_seq, "hip": lambda: qgemm.fp_linear(x, w, b, torch.float32, gate=gate, residual=res, out=res)},
                     rounds, reps)
            line += f"{'+gate+res':10s} {seq['torch']:10.1f} {seq['hip']:10.1f} {seq['torch'] / seq['hip']:7.3f}"
            del res
        print(line, flush=True)
        del x, w, y
        torch.cuda.empty_cache()


def block_section(rounds):
    from oracle import qdiff_ref  # noqa: F401  (the ViDiT helpers the block test uses live beside the oracle)
    from qdiff import config as qcfg
    from qdiff.base.quant_model import quant_layer_refactor_
    from qdiff.utils import apply_func_to_submodules
    from wan import calib, ops
    from wan.modules.model import WanAttentionBlock
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    from oracle import wan_ref as wr

    dim, ffn, heads, grid, lc = 1536, 8960, 12, (21, 30, 52), 512
    L = grid[0] * grid[1] * grid[2]
    torch.manual_seed(0)
    blk = WanAttentionBlock("t2v_cross_attn", dim, ffn, heads, cross_attn_norm=True)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.normal_(m.bias, std=0.05)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(L, dim, generator=g).to(DEV)
    e0 = (torch.randn(1, 6, dim, generator=g) * 0.3).to(DEV)
    ctx = torch.randn(lc, dim, generator=g).to(DEV)
    act_mask = torch.rand(dim, generator=g) * 3 + 0.2
    cfg = qcfg.create({"weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": 8, "sym": True},
                       "viditq": {"alpha": 0.5665, "layer_name_regex": ""},
                       "remain_fp_regex": r"self_attn\.(?!q$)(?!k$)(?!v$)[^.]+|ffn.*|cross_attn"})
    blk = blk.to(DEV)
    apply_func_to_submodules(blk, torch.nn.Linear, quant_layer_refactor_, name=None, parent_module=None, quant_config=cfg,
                             full_name=None, remain_fp_regex=cfg.remain_fp_regex)
    gen = torch.Generator().manual_seed(11)
    for name in ("q", "k", "v"):
        calib.init_rotation_and_channel_mask_(getattr(blk.self_attn, name), "x", {"x": act_mask[None]}, gen)
    rope = ops.rope_table(wr.rope_freqs(dim // heads), grid, DEV)
    blocks = {m: WanAttentionBlockWithHipKernel.from_float(blk, None, fp_gemm=m) for m in ("torch", "hip")}
    buf = {m: x.clone() for m in blocks}
    outs = {}

    def run(m):
        buf[m].copy_(x)
        outs[m] = blocks[m](buf[m], e0, rope, L, _FpSrc(ctx, torch.bfloat16))

    t = ab({m: (lambda m=m: run(m)) for m in blocks}, rounds, 5)
    rel = ((outs["hip"] - outs["torch"]).double().norm() / outs["torch"].double().norm()).item()
    print(f"\n## 2. shipped-configuration kernel-mode block, 1.3B, L = {L} (ms per block, incl. one [L,1536] fp32 copy per call in both arms)")
    print(f"fp_gemm=torch {t['torch'] / 1e3:8.3f} ms   fp_gemm=hip {t['hip'] / 1e3:8.3f} ms   torch/hip {t['torch'] / t['hip']:.3f}   "
          f"output rel diff {rel:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-block", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_fp_gemm.py measures on the GPU; none is visible")
    print(f"# tools/ab_fp_gemm.py on {torch.cuda.get_device_name()}, torch {torch.__version__}, rounds {a.rounds}")
    gemm_section(a.rounds)
    if not a.no_block:
        block_section(a.rounds)


if __name__ == "__main__":
    main()
