"""Kernel mode in the reference's dtype: WanAttentionBlockWithHipKernel(act_dtype=torch.float16) -- fp16 activations between the
kernels and fp16 operands in both attentions (csrc/attention.hip, WANQ_F16) -- against the simulation oracle under the bars of the
bf16 block tests, the refusals that go with it, and quant_generate --act_dtype fp16 end to end."""
import os

import pytest
import torch

from oracle import wan_ref as wr
from test_gpu_block import make_block, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")


def _block_inputs(dim, grid, pad, lc):
    n_tok = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_tok + pad, dim, generator=g)
    x[:, 5] *= 12.0  # an outlier channel, as real DiT activations have
    x[n_tok:] = 0
    e0 = torch.randn(1, 6, dim, generator=g) * 0.3
    ctx = torch.randn(lc, dim, generator=g)
    return n_tok, x, e0, ctx


def _run_block(blk, act_dtype, x, e0, grid, n_tok, ctx, freqs, **kw):
    from wan import ops
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel, _FpSrc

    hb = WanAttentionBlockWithHipKernel.from_float(blk, act_dtype=act_dtype, **kw)
    xd = x.to(DEV).clone()
    out = hb(xd, e0.to(DEV), ops.rope_table(freqs, grid, DEV), n_tok, _FpSrc(ctx.to(DEV), act_dtype))
    assert out.data_ptr() == xd.data_ptr()  # residual stream updated in place
    return out.float().cpu()[:n_tok]


@pytest.mark.parametrize("dim,ffn,heads,grid,pad,lc", [(256, 512, 2, (3, 6, 10), 4, 40), (1536, 8960, 12, (2, 6, 8), 0, 64)])
def test_fp16_kernel_mode_block_vs_simulation_oracle(dim, ffn, heads, grid, pad, lc):
    """test_kernel_mode_block_vs_simulation_oracle with act_dtype=torch.float16: the same inputs, oracle and two assertions."""
    blk = make_block(dim, ffn, heads, 0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok, x, e0, ctx = _block_inputs(dim, grid, pad, lc)
    freqs = wr.rope_freqs(dim // heads)
    ref_q = wr.block_from_state(sd, heads, quant=True)(x, e0, grid, n_tok, ctx, freqs)
    ref_fp = wr.block_from_state(sd, heads, quant=False)(x, e0, grid, n_tok, ctx, freqs)
    blk = blk.to(DEV)
    err_q = rel_err(_run_block(blk, torch.float16, x, e0, grid, n_tok, ctx, freqs), ref_q[:n_tok])
    err_b = rel_err(_run_block(blk, torch.bfloat16, x, e0, grid, n_tok, ctx, freqs), ref_q[:n_tok])
    quant_noise = rel_err(ref_q[:n_tok], ref_fp[:n_tok])
    print(f"dim={dim}: fp16 block rel err vs fake-quant oracle {err_q:.2e} (bf16 block {err_b:.2e}); fake-quant vs fp {quant_noise:.2e}")
    assert err_q < 1e-2
    assert err_q < 0.5 * quant_noise + 5e-3


def test_fp16_kernel_mode_block_with_quantized_qk_vs_oracle():
    """test_kernel_mode_block_with_quantized_qk_vs_oracle (tests/test_gpu_attn_qk8.py) under fp16: int8 Q.K^T in both attentions, V,
    P and O in fp16; the same oracle and bar."""
    dim, ffn, heads, grid, lc = 1536, 8960, 12, (2, 6, 8), 64
    blk = make_block(dim, ffn, heads, 0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok, x, e0, ctx = _block_inputs(dim, grid, 0, lc)
    freqs = wr.rope_freqs(dim // heads)
    ref = wr.block_from_state(sd, heads, quant=True, qk_bits=8, cross_qk_bits=8)(x, e0, grid, n_tok, ctx, freqs)
    blk = blk.to(DEV)
    err = rel_err(_run_block(blk, torch.float16, x, e0, grid, n_tok, ctx, freqs, attn_qk8=True, cross_attn_qk8=True), ref)
    err_b = rel_err(_run_block(blk, torch.bfloat16, x, e0, grid, n_tok, ctx, freqs, attn_qk8=True, cross_attn_qk8=True), ref)
    print(f"fp16 block with int8 Q.K^T: rel err vs recipe oracle {err:.2e} (bf16 block {err_b:.2e})")
    assert err < 1e-2


def test_attention_map_config_is_refused_under_fp16_by_layer_name():
    """attn.attn_map together with act_dtype=float16: refused once, by hardware_forward_refactor, with the layer's name -- not from
    inside the first forward; the same config builds under bf16."""
    from qdiff import config as qcfg
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    base = {"model": {"model_id": "wan2.1", "model_type": "wanx"}, "remain_fp_regex": "text_embedding|time_embedding|time_projection|head\\.head",
            "weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": 8, "sym": True}}
    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, freq_dim=64).eval()
    for key in ("attn", "cross_attn"):
        m = QuantWanModel.from_float(fp, qcfg.create(dict(base, **{key: {"attn_map": {"n_bits": 8, "sym": False, "group": "row"}}})))
        m.quant_layer_refactor()
        m.set_init_done()
        with pytest.raises(NotImplementedError, match=rf"^{key}\.attn_map.*float16.*bf16"):
            m.hardware_forward_refactor(act_dtype=torch.float16)
        assert getattr(m, "hip_blocks", None) is None or len(m.hip_blocks) == 0 or m.hip_blocks[0].act_dtype != torch.float16
        m.hardware_forward_refactor(act_dtype=torch.bfloat16)
        assert (m.hip_blocks[0].attn_map if key == "attn" else m.hip_blocks[0].cross_attn_map) == (8, False)
    # a config without a map builds under fp16
    m = QuantWanModel.from_float(fp, qcfg.create(dict(base, attn={"qk": {"n_bits": 8, "sym": True}})))
    m.quant_layer_refactor()
    m.set_init_done()
    m.hardware_forward_refactor(act_dtype=torch.float16)
    assert m.hip_blocks[0].act_dtype == torch.float16 and m.hip_blocks[0].attn_qk8


def _qkv(dtype_q, dtype_k, dtype_v, Lq=70, Lk=130, H=2):
    g = torch.Generator().manual_seed(3)
    return ((torch.randn(Lq, H * 128, generator=g) * 1.5).to(DEV).to(dtype_q), (torch.randn(Lk, H * 128, generator=g) * 1.5).to(DEV).to(dtype_k),
            torch.randn(Lk, H * 128, generator=g).to(DEV).to(dtype_v))


def test_ops_attention_refuses_a_mixed_set_by_name():
    from wan import ops

    q, k, v = _qkv(torch.bfloat16, torch.float16, torch.float16)
    with pytest.raises(RuntimeError, match=r"q is torch\.bfloat16, k is torch\.float16, v is torch\.float16.*all be torch\.bfloat16 or all be torch\.float16"):
        ops.attention(q, k, v, 2)
    q, k, v = _qkv(torch.float16, torch.float16, torch.float32)
    with pytest.raises(RuntimeError, match=r"v is torch\.float32"):
        ops.attention(q, k, v, 2)
    q, k, v = _qkv(torch.float16, torch.float16, torch.float16)
    with pytest.raises(RuntimeError, match=r"out is torch\.bfloat16"):
        ops.attention(q, k, v, 2, out=torch.empty(q.shape, dtype=torch.bfloat16, device=DEV))
    assert ops.attention(q, k, v, 2).dtype == torch.float16


def test_ops_attention_on_fp32_operands_still_rounds_to_bf16():
    """fp32 operands (the act_dtype=float32 parity configuration) are rounded to bf16, as before fp16 existed: bit-equal to the bf16
    call on the rounded operands."""
    from wan import ops

    q, k, v = _qkv(torch.float32, torch.float32, torch.float32)
    o32 = ops.attention(q, k, v, 2)
    ob = ops.attention(q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), 2)
    assert o32.dtype == torch.bfloat16 and torch.equal(o32, ob)


def test_rmsnorm_rope_q8_float_output_follows_the_16_bit_type():
    """The optional float row of rmsnorm_rope_q8 is of the input's 16-bit type (or the requested one), and equals the plain
    rmsnorm_rope_ output in that type."""
    from wan import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(70, 256, generator=g).to(DEV)
    w = (torch.rand(256, generator=g) + 0.5).to(DEV)
    for dt in (torch.float16, torch.bfloat16):
        q8, fp = ops.rmsnorm_rope_q8(x.to(dt), w, None, 128, False, want_fp=True)
        assert fp.dtype == dt and torch.equal(fp, ops.rmsnorm_rope_(x.to(dt).clone(), w, None, 128))
        _, fp2 = ops.rmsnorm_rope_q8(x, w, None, 128, False, want_fp=True, fp_dtype=dt)
        assert fp2.dtype == dt
    _, fp3 = ops.rmsnorm_rope_q8(x, w, None, 128, False, want_fp=True)
    assert fp3.dtype == torch.bfloat16  # fp32 input, nothing requested: bf16 as before


def test_attention_map_quant_refuses_fp16_operands():
    from wan import ops

    q, k, v = _qkv(torch.float16, torch.float16, torch.float16)
    with pytest.raises(RuntimeError, match="fp16 operands are not implemented.*bf16 hi \\+ lo pair"):
        ops.attention_map_quant(q, k, v, 2)


def test_fp_model_attention_runs_in_fp16_when_the_projections_write_fp16():
    """A .half() FP model hands its attentions fp16 operands (the reference's flash_attention keeps fp16 q / k / v); any other
    model bf16, as before."""
    from wan import ops
    from wan.modules.model import WanSelfAttention

    seen = []
    real = ops.attention

    def spy(q, k, v, *a, **kw):
        seen.append((q.dtype, k.dtype, v.dtype))
        return real(q, k, v, *a, **kw)

    torch.manual_seed(0)
    sa = WanSelfAttention(256, 2).to(DEV)
    x = torch.randn(1, 60, 256, device=DEV)
    freqs = wr.rope_freqs(128)
    grid = [(3, 4, 5)]
    ops.attention = spy
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):  # (how the fp32 checkpoint runs: 16-bit projections under autocast)
            y32 = sa(x, torch.tensor([60]), grid, freqs)
        y16 = sa.half()(x.half(), torch.tensor([60]), grid, freqs)
    finally:
        ops.attention = real
    assert seen == [(torch.bfloat16,) * 3, (torch.float16,) * 3]
    # (a sanity bar only: two 16-bit runs of three GEMMs and an attention; a misread operand type is off by O(1))
    assert y16.dtype == torch.float16 and rel_err(y16.float(), y32.float()) < 5e-2


def test_quant_generate_act_dtype_fp16_end_to_end(tmp_path):
    """The toy chain of tests/test_gpu_entrypoints.py (2 blocks, 832*480, 5 frames, 2 steps) with quant_generate --act_dtype fp16:
    the latent is finite and within that file's kernel-mode distance (rel 0.03) of the bf16 run."""
    from test_gpu_entrypoints import run

    qc = os.path.join(PKG, "quant_configs", "w8a8_all_linears.yaml")
    calib = str(tmp_path / "calib.pth")
    run("get_calib_data_wanx.py", "--quant_config", qc, "--calib_data", calib, cwd=tmp_path)
    run("ptq_wanx.py", "--quant_config", qc, "--calib_data", calib, cwd=tmp_path)
    run("quant_generate.py", "--quant_config", qc, cwd=tmp_path)
    hw = torch.load(tmp_path / "quant_latent_0.pt", weights_only=True)
    run("quant_generate.py", "--quant_config", qc, "--act_dtype", "fp16", "--save_file", str(tmp_path / "fp16.pt"), cwd=tmp_path)
    h16 = torch.load(tmp_path / "fp16.pt", weights_only=True)
    assert h16.shape == hw.shape and torch.isfinite(h16).all()
    rel = ((h16 - hw).norm() / hw.norm()).item()
    print(f"quant_generate --act_dtype fp16 vs bf16: rel {rel:.3e}")
    assert rel < 0.03 and not torch.equal(h16, hw)
