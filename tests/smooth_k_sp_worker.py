"""Worker for tests/test_gpu_smooth_k.py: two ranks on ONE GPU run a kernel-mode block with attn.qk + smooth_k under Ulysses.

As in tests/sp_rehearsal_worker.py the process group is gloo and the collectives are staged through host memory
(tools/one_gpu_rehearsal.py); everything else is the product code.  A rank holds a token shard of k, so the column sums of the two
shards are added over the group before the centred quantiser: a differently ordered sum than the single rank's, hence a bound and a
bar here where that worker asserts bit equality."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wan2.1-quantization_amd"))
sys.path.insert(0, ROOT)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", init_method="env://")
    from wan.distributed import stage_rehearsal_collectives
    stage_rehearsal_collectives()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    from oracle import wan_ref as wr
    from test_gpu_block import make_block, rel_err
    from wan import ops
    from wan.distributed.parallel import ParallelPlan
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    # ---- the block of tests/test_gpu_attn_qk8.py's block case, self-attention smoothed
    dim, ffn, heads, grid, lc = 1536, 8960, 12, (2, 6, 8), 64
    n_tok = grid[0] * grid[1] * grid[2]
    hb = WanAttentionBlockWithHipKernel.from_float(make_block(dim, ffn, heads, 0).to(dev), attn_qk8=True, cross_attn_qk8=True, attn_smooth_k=True)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_tok, dim, generator=g)
    x[:, 5] *= 12.0
    e0 = (torch.randn(1, 6, dim, generator=g) * 0.3).to(dev)
    ctx = torch.randn(lc, dim, generator=g).to(dev)
    rope = ops.rope_table(wr.rope_freqs(dim // heads), grid, dev)
    one = hb(x.to(dev).clone(), e0, rope, n_tok, _FpSrc(ctx, torch.bfloat16))

    sp = ParallelPlan(world, rank, 1, world).sp
    assert sp.size == world and n_tok % world == 0
    lp = n_tok // world
    rows = slice(rank * lp, (rank + 1) * lp)
    names, call = [], ops._C.call
    ops._C.call = lambda name, *a, **kw: (names.append(name), call(name, *a, **kw))[1]
    two = hb(x[rows].to(dev).clone(), e0, rope[rows].contiguous(), n_tok, _FpSrc(ctx, torch.bfloat16), sp=sp)
    ops._C.call = call
    assert names.count("wanq_rmsnorm_rope_colsum") == 1 and names.count("wanq_rmsnorm_rope_q8_centered") == 1, names  # k only, never q
    e_sp = rel_err(two.float().cpu(), one[rows].float().cpu())

    # ---- the all-reduced centre against the single-rank centre, under the fixed-order summation bound of the column sums
    # (tests/test_gpu_smooth_k.py, G2): |sum~ - sum| <= rows * 2^-24 * sum|y| for either order, so the two differ by at most twice that;
    # the division by rows adds half an ulp of the centre on each side
    L, C = 1000, 1536
    k = (torch.randn(L, C, generator=g) + 3.0 * torch.randn(C, generator=g)).to(torch.bfloat16).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    table = ops.rope_table(wr.rope_freqs(128), (1, 1, L), dev)
    single = ops.center_of(ops.rmsnorm_rope_colsum(k, w, table, 128), L)
    half = L // world
    mine = slice(rank * half, (rank + 1) * half)
    # (a shard's rows keep their own positions: the rope rows of the shard)
    both = sp.mean_rows(ops.rmsnorm_rope_colsum(k[mine].contiguous(), w, table[mine].contiguous(), 128), half)
    y = ops.rmsnorm_rope_(k, w, table, 128, out=torch.empty(L, C, dtype=torch.float32, device=dev))
    bound = 2.0 * L * 2.0 ** -24 * y.double().abs().sum(0) / L + 2.0 ** -24 * single.double().abs()
    diff = (both.double() - single.double()).abs()
    ok = bool((diff <= bound).all())
    torch.cuda.synchronize()
    print(f"RANK {rank} smooth_k_sp_rel={e_sp:.3e} centre_ok={ok} centre_max_ratio={(diff / bound).max().item():.3f}", flush=True)
    assert e_sp < 1e-2, e_sp
    assert ok
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
