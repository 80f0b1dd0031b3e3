"""The W4A16 MXFP4 GEMM (csrc/gemm_wq16_mx.hip, qgemm.wq16_mx_linear) against its contract (include/wanq_hip.h), and one kernel-mode
block (HipLinearWq16Mx) against the float64 oracle on the simulation-mode weights.

The bound.  Operands and products are exact (e2m1 2^r is a number of the operand type), so only the fp32 accumulation of K terms
and the one output rounding remain: |y - ref| <= K 2^-23 (|a| |w_hat|^T) + ulp_out(|ref|).  With an epilogue behind it the value
before it, fma(acc, 2^e, bias), carries an fp32 rounding of its own, 2^-23 |y0|; the sum goes through GELU times 1.13 (its largest
slope) plus 3e-6 |gelu| (gelu_tanh_fast_f32) and through gate + residual times |gate|, as tests/test_gpu_wq16.py has it."""
import os

import pytest
import torch
from oracle import wan_ref as wr
from test_gpu_wq16 import _ULP, DEV, PKG, _Lin16, _make_block, _rel, gelu64

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 64), (133, 136, 192), (256, 128, 128)]  # one and three K-tiles, a partial token tile, a partial channel tile
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def operands(M, N, K, dtype, lo, hi, row_exp=None):
    """a [M, K]; packed codes with all 16 nibbles at every position of a 64-code tile (N >= 16); scale bytes row_exp + lo .. + hi"""
    from qdiff.base.base_quantizer import mx_pack_e2m1

    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    w = mx_pack_e2m1(((n + 3 * k + k // 64) % 16).to(torch.uint8))
    e = torch.full((N,), 127, device=DEV) if row_exp is None else row_exp + torch.arange(N, device=DEV) * 7 % 20
    s = (e[:, None] + torch.randint(lo, hi + 1, (N, K // 32), device=DEV, generator=g)).to(torch.uint8)
    return a, w, s, e.to(torch.uint8), g


def op64(w, s, e, dtype):
    """the contract's operand, float64: e2m1(w) 2^(s - e), blocks below the operand type's window flushed to zero"""
    from qdiff.base.base_quantizer import mx_decode

    r = s.long() - e.long()[:, None]
    v = mx_decode(w, (r + 127).clamp(0, 254).to(torch.uint8), "mxfp4_e2m1", torch.float64)
    return v * (r >= (-13 if dtype == torch.float16 else -112)).repeat_interleave(32, dim=1)


@DTYPES
@pytest.mark.parametrize("MNK", SHAPES)
def test_bit_equal_to_the_bf16_gemm_on_the_decoded_weight(MNK, dtype):
    from viditq_extension import qgemm

    a, w, s, e, _ = operands(*MNK, dtype, -6, 6)
    want = qgemm.fp_linear(a, op64(w, s, e, dtype).to(dtype), out_dtype=torch.float32)
    assert torch.equal(qgemm.wq16_mx_linear(a, w, s, e, out_dtype=torch.float32), want)


@DTYPES
@pytest.mark.parametrize("MNK", SHAPES)
def test_row_exponent_and_flush_bit_for_bit(MNK, dtype):
    from viditq_extension import qgemm

    a, w, s, e, g = operands(*MNK, dtype, -20, 13, 100)
    bias = torch.randn(MNK[1], device=DEV, generator=g)
    assert MNK[1] == 8 or bool((s.long() - e.long()[:, None] < -13).any())  # blocks that fp16 flushes and bf16 keeps
    acc = qgemm.fp_linear(a, op64(w, s, e, dtype).to(dtype), out_dtype=torch.float32)  # (exact in dtype; the test above pins the order)
    want = acc * torch.exp2(e.float() - 127.0) + bias  # the product is exact: one rounding, the fma's
    assert torch.equal(qgemm.wq16_mx_linear(a, w, s, e, bias, out_dtype=torch.float32), want)


@pytest.mark.parametrize("out32", [True, False], ids=["f32", "out16"])
@pytest.mark.parametrize("epi", ["plain", "gelu", "gate_res"])
@DTYPES
def test_within_the_derived_bound_of_float64(dtype, epi, out32):
    from viditq_extension import qgemm

    M, N, K = SHAPES[1]
    out_dtype = torch.float32 if out32 else dtype
    a, w, s, e, g = operands(M, N, K, dtype, -20, 13, 95)  # |w_hat| <= 6
    bias, gate = torch.randn(N, device=DEV, generator=g) * 0.1, torch.rand(N, device=DEV, generator=g) * 2 - 1
    res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
    w_hat = op64(w, s, e, dtype) * torch.exp2(e.double() - 127.0)[:, None]
    y = a.double() @ w_hat.T + bias.double()
    tol = K * 2.0 ** -23 * (a.double().abs() @ w_hat.abs().T) + (0.0 if epi == "plain" else 2.0 ** -23 * y.abs())
    if epi == "gelu":
        y = gelu64(y)
        tol = tol * 1.13 + 3e-6 * y.abs()
    if epi == "gate_res":
        y, tol = res.double() + y * gate.double(), tol * gate.double().abs()
    tol = tol + y.abs() * _ULP[out_dtype] + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
    out = qgemm.wq16_mx_linear(a, w, s, e, bias, out_dtype, gelu=epi == "gelu", gate=gate if epi == "gate_res" else None,
                               residual=res.clone() if epi == "gate_res" else None)
    err = (out.double() - y).abs()
    print(f"{dtype} -> {out_dtype} {epi}: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any(), f"{int((err > tol).sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}"


def test_kernel_mode_block_vs_float64_oracle_on_the_simulation_mode_weights():
    """tests/test_gpu_wq16.py's integer W4A16 block: its dimensions, its oracle (float64 Linears on the 16-bit activation, here with
    the weights simulation mode multiplies by) and its bar, 1.5 times the FP block's error against its own oracle."""
    from qdiff import config as qcfg
    from qdiff.base.quant_model import quant_layer_refactor_
    from qdiff.utils import apply_func_to_submodules
    from wan import ops
    from wan.quant_wanx_hip import HipLinearWq16Mx, WanAttentionBlockWithHipKernel, _FpSrc

    dim, ffn, heads, grid, pad, lc, act_dtype = 256, 512, 2, (3, 6, 10), 4, 40, torch.bfloat16
    blk = _make_block(dim, ffn, heads, 0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_tok + pad, dim, generator=g)
    x[:, 5] *= 12.0
    x[n_tok:] = 0
    e0, ctx = torch.randn(1, 6, dim, generator=g) * 0.3, torch.randn(lc, dim, generator=g)
    freqs = wr.rope_freqs(dim // heads)
    norm_w = {k: sd[k + ".weight"].float() for k in ("self_attn.norm_q", "self_attn.norm_k", "cross_attn.norm_q", "cross_attn.norm_k")}
    rope = ops.rope_table(freqs, grid, DEV)

    def err(hb, weights):  # the kernel-mode block against the float64 oracle with these Linear weights
        lin = {nm: _Lin16(weights[nm], sd[nm + ".bias"], act_dtype) for nm in wr.LINEARS}
        ref = wr.BlockRef(lin, norm_w, sd["modulation"], heads, 1e-6, (sd["norm3.weight"].float(), sd["norm3.bias"].float()))(
            x, e0, grid, n_tok, ctx, freqs)[:n_tok]
        return _rel(hb(x.to(DEV).clone(), e0.to(DEV), rope, n_tok, _FpSrc(ctx.to(DEV), act_dtype)).float().cpu()[:n_tok], ref)

    blk = blk.to(DEV)
    err_fp = err(WanAttentionBlockWithHipKernel.from_float(blk, None, act_dtype=act_dtype, fp_gemm="hip"),
                 {nm: sd[nm + ".weight"].to(act_dtype) for nm in wr.LINEARS})
    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "mx", "w4a16_mxfp4_all_linears.yaml"))
    apply_func_to_submodules(blk, torch.nn.Linear, quant_layer_refactor_, name=None, parent_module=None, quant_config=cfg, full_name=None,
                             remain_fp_regex=None)
    hb = WanAttentionBlockWithHipKernel.from_float(blk, None, act_dtype=act_dtype)
    assert all(isinstance(l, HipLinearWq16Mx) for l in [getattr(a, l) for a in (hb.self_attn, hb.cross_attn) for l in "qkvo"] + [hb.ffn0, hb.ffn2])
    err_mx = err(hb, {nm: blk.get_submodule(nm).weight.data.cpu() for nm in wr.LINEARS})
    print(f"W4A16 MXFP4 block bf16 (dim {dim}): rel err vs the float64 oracle on the simulation-mode weights {err_mx:.3e}; the FP block "
          f"(fp_gemm=hip) vs its own {err_fp:.3e}; ratio {err_mx / err_fp:.2f}")
    assert err_mx <= 1.5 * err_fp
