"""wanq_quant_rows_mx4_project and wanq_gemm_mx4_lowrank on the GPU, from the entries up to a kernel-mode model.  Producer bound: K 2^-24
sum_k |xt a| + u_T |t64| (recursive summation plus the one rounding).  GEMM bound: (K + R) 2^-24 (sum |a w| + sum |t b|) before the
epilogue, carried through it by bound_case of tests/test_gpu_fp8.py with K + R terms, as tests/test_gpu_mx4.py carries its own."""
import os

import pytest
import torch

from test_gpu_fp8 import OUTS, _tiny_model, bound_case, gen_for, ones, rel_l2
from test_gpu_mx import deq64
from test_gpu_mx4 import FP4, random_operands
from test_gpu_wq16 import DEV, PKG
from viditq_extension import fused, qgemm

pytestmark = pytest.mark.gpu

T16 = pytest.mark.parametrize("T", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
U_T = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
YAML, YAMLH = (os.path.join(PKG, "quant_configs", "lowrank", f"w4a4_mxfp4_{h}lr32_all_linears.yaml") for h in ("", "had32_"))


def tri(shape, g, dtype):  # values in {-1, 0, 1}
    return (torch.randint(0, 3, shape, device=DEV, generator=g) - 1).to(dtype)


def window(rows, R, T, wide):  # (buffer, t): t dense, or the window at column 64 of a sentinel-filled [rows, 192] buffer
    buf = torch.full((rows, 192 if wide else R), 7.0, dtype=T, device=DEV)
    return buf, buf[:, 64:64 + R] if wide else buf


@pytest.mark.parametrize("had", [False, True], ids=["plain", "had32"])
@pytest.mark.parametrize("gelu", [False, True], ids=["id", "gelu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_codes_and_scale_bytes_equal_the_plain_quantisers(dtype, gelu, had):
    x = torch.randn(77, 384, device=DEV, generator=gen_for(1))
    x[:, [9, 130, 383]] *= 20
    q, s, _ = fused.quant_rows_mxfp4_project(x.to(dtype), torch.ones(64, 384, dtype=torch.bfloat16, device=DEV), gelu=gelu, had32=had)
    q0, s0 = fused.quant_rows_mx(x.to(dtype), FP4, gelu, had32=had)
    assert torch.equal(q, q0) and torch.equal(s, s0)


@T16
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("rows", [1, 77, 129])
def test_one_hot_factor_picks_the_named_column_and_leaves_the_rest_of_t_alone(rows, wide, T):
    K, R = 384, 64
    k_r = (7 * torch.arange(R, device=DEV)) % K          # every 64-column step, both halves, every lane group, every element slot
    a16 = torch.zeros(R, K, dtype=T, device=DEV)
    a16[torch.arange(R, device=DEV), k_r] = 1
    m, k = torch.arange(rows, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    x = ((5 * m + 3 * k) % 64 - 32).float()
    buf, t = window(rows, R, T, wide)
    fused.quant_rows_mxfp4_project(x, a16, out=t)
    assert torch.equal(t.float(), x[:, k_r])
    assert not wide or ((buf[:, :64] == 7).all() and (buf[:, 64 + R:] == 7).all())


@T16
@pytest.mark.parametrize("R", [64, 128, 256])
@pytest.mark.parametrize("K", [128, 256])
def test_integer_sums_are_exact(K, R, T):
    g = gen_for(K + R)
    x, a16 = tri((129, K), g, torch.float32), tri((R, K), g, T)
    _, _, t = fused.quant_rows_mxfp4_project(x, a16)
    assert torch.equal(t.double(), x.double() @ a16.double().T)


@T16
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_random_rows_within_the_derived_bound(dtype, T):
    K, R, g = 384, 128, gen_for(4)
    x = torch.randn(77, K, device=DEV, generator=g).to(dtype)
    a16 = (torch.randn(R, K, device=DEV, generator=g) * K ** -0.5).to(T)
    _, _, t = fused.quant_rows_mxfp4_project(x, a16)
    xt, a = x.to(T).double(), a16.double()
    t64 = xt @ a.T
    tol = K * 2.0 ** -24 * (xt.abs() @ a.abs().T) + U_T[T] * t64.abs()
    assert not ((t.double() - t64).abs() > tol).any()


@pytest.mark.parametrize("zero", ["t", "b"])
@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_zero_branch_gives_the_plain_gemms_values(out_dtype, zero):
    M, N, K, R, g = 129, 136, 384, 64, gen_for(5)
    a, w, sa, sw = random_operands(M, N, K, g)
    t = torch.randn(M, R, device=DEV, generator=g).to(torch.bfloat16) * (zero != "t")
    b = torch.randn(N, R, device=DEV, generator=g).to(torch.bfloat16) * (zero != "b")
    bias, gate = torch.randn(N, device=DEV, generator=g), torch.rand(N, device=DEV, generator=g)
    res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
    for kw in ({}, {"gelu": True}, {"gate": gate, "residual": res}):
        got = qgemm.mx4_lowrank_linear(a, w, sa, sw, t, b, bias, out_dtype, **kw)
        assert bool((got == qgemm.mx4_linear(a, w, sa, sw, bias, out_dtype, **kw)).all()), kw


@pytest.mark.parametrize("R", [64, 128, 256])
@pytest.mark.parametrize("N", [8, 136])
@pytest.mark.parametrize("M", [1, 77, 129])
def test_branch_alone_is_the_integer_product_plus_bias(M, N, R):
    K, g = 128, gen_for(M + N + R)
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)  # noqa: E731
    a, w, sa, sw = z(M, K // 2), z(N, K // 2), z(M, K // 32) + 127, z(N, K // 32) + 127
    _, t = window(M, R, torch.float16, R <= 128)   # distinct small integers, inside the wider buffer where it holds them
    t.copy_(((3 * torch.arange(M, device=DEV)[:, None] + torch.arange(R, device=DEV)[None, :]) % 128 - 64).half())
    onehot = torch.zeros(N, R, dtype=torch.float16, device=DEV)
    onehot[torch.arange(N, device=DEV), (5 * torch.arange(N, device=DEV)) % R] = 1                   # pins the (n, r) map
    bias = torch.randint(-3, 4, (N,), device=DEV, generator=g).float()
    for b in (tri((N, R), g, torch.float16), onehot):
        out = qgemm.mx4_lowrank_linear(a, w, sa, sw, t, b, bias, torch.float32)
        assert torch.equal(out.double(), t.double() @ b.double().T + bias.double())


@T16
@pytest.mark.parametrize("M,N,K,R", [(129, 136, 384, 128), (77, 8, 128, 256)])
def test_codes_and_branch_within_the_derived_bound(M, N, K, R, T):
    g = gen_for(M + K + R)
    a, w, sa, sw = random_operands(M, N, K, g)
    a64, w64 = deq64(a, sa, FP4), deq64(w, sw, FP4)
    S0 = a64.abs() @ w64.abs().T
    t = torch.randn(M, R, device=DEV, generator=g).to(T)  # (t b^T is four times the 4-bit product: behind GELU it would miss by O(1))
    b = (torch.randn(N, R, device=DEV, generator=g) * 4 * (a64 @ w64.T).std().item() * R ** -0.5).to(T)
    acc, S = a64 @ w64.T + t.double() @ b.double().T, S0 + t.double().abs() @ b.double().abs().T
    bias, gate = torch.randn(N, device=DEV, generator=g) * 0.1, torch.rand(N, device=DEV, generator=g) * 2 - 1
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True)):
            out = qgemm.mx4_lowrank_linear(a, w, sa, sw, t, b, bias, out_dtype, gelu=gelu, gate=gate if gres else None,
                                           residual=res.clone() if gres else None)
            y, tol = bound_case(S, acc, ones(M), ones(N), bias, gelu, gate if gres else None, res, out_dtype, K + R)
            worst[(str(out_dtype)[6:], gelu, gres)] = round(((out.double() - y).abs() / tol).max().item(), 4)
    print(f"MX4 low-rank GEMM ({M}, {N}, {K}, R={R}, {T}): worst err / bound {max(worst.values()):.4f} {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_rows_of_a_launch_of_129_equal_launches_of_one_row():
    M, N, K, R, g = 129, 136, 384, 128, gen_for(8)
    x = torch.randn(M, K, device=DEV, generator=g)
    a16 = torch.randn(R, K, device=DEV, generator=g).to(torch.bfloat16)
    b16 = torch.randn(N, R, device=DEV, generator=g).to(torch.bfloat16)
    _, w, _, sw = random_operands(M, N, K, g)
    q, s, t = fused.quant_rows_mxfp4_project(x, a16, gelu=True, had32=True)
    y = qgemm.mx4_lowrank_linear(q, w, s, sw, t, b16, None, torch.bfloat16, gelu=True)
    for m in (0, 77, 128):
        q1, s1, t1 = fused.quant_rows_mxfp4_project(x[m:m + 1].contiguous(), a16, gelu=True, had32=True)
        assert torch.equal(q1, q[m:m + 1]) and torch.equal(s1, s[m:m + 1]) and torch.equal(t1, t[m:m + 1])
        assert torch.equal(qgemm.mx4_lowrank_linear(q1, w, s1, sw, t1, b16, None, torch.bfloat16, gelu=True), y[m:m + 1])


@pytest.mark.parametrize("path", [YAML, YAMLH], ids=["plain", "had32"])
def test_layer_in_simulation_mode_kernel_mode_and_through_a_checkpoint(path):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from wan.quant_wanx_hip import HipLinearMx, _FpSrc

    N, K, M = 136, 384, 77
    gen = torch.Generator().manual_seed(9)
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(torch.randn(N, K, generator=gen) * K ** -0.5)
    ql = QuantizedLinear(K, N, True, DEV, qcfg.load(path), fp, module_name="blocks.0.ffn.0")
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16).to(DEV)
    out = ql(x)
    host = ql.cpu()(x.cpu())
    ql.to(DEV)
    a16, b16 = ql.low_rank_operands(torch.bfloat16, DEV)
    a_q, a_s = ql.a_quantizer.codes_and_scale(x)
    a64, w64 = deq64(a_q, a_s, FP4), ql.weight.data.double()
    # each forward against float64 on the t it multiplied (a rounding of t may fall either way): the producer's, or torch's on the host
    t_gpu = fused.quant_rows_mxfp4_project(x, a16, had32=ql.mx_had32)[2]
    t_host = (x.cpu().float() @ a16.cpu().float().t()).to(torch.bfloat16).to(DEV)
    for name, got, t in (("GPU", out, t_gpu.double()), ("host", host.to(DEV), t_host.double())):
        acc, S = a64 @ w64.T + t @ b16.double().T, a64.abs() @ w64.abs().T + t.abs() @ b16.double().abs().T
        y, tol = bound_case(S, acc, ones(M), ones(N), ql.bias.detach().float(), False, None, None, torch.bfloat16, K + 64)
        assert not ((got.double() - y).abs() > tol).any(), name
    hl = HipLinearMx.from_quantized(ql, "blocks.0.ffn.0", torch.bfloat16)
    fresh = HipLinearMx(K, N, True, FP4, "blocks.0.ffn.0", FP4, ql.mx_had32, low_rank=32).to(DEV)
    fresh.load_state_dict(hl.state_dict())
    for lin in (hl, fresh):  # kernel mode, built from the layer and restored from its checkpoint: the simulation-mode layer's bits
        src = _FpSrc(x)
        assert torch.equal(lin(*lin.operands(src), torch.bfloat16, **lin.extras(src)), out)


def test_kernel_mode_blocks_share_one_producer_launch_per_source_and_match_simulation_mode(monkeypatch):
    from qdiff import config as qcfg
    t = torch.tensor([700], device=DEV)
    model, fp, seq_len, ctx, lat0 = _tiny_model(qcfg.load(YAML))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref_fp = fp([lat0], t, [ctx], seq_len)[0].float().clone()
    sim = model([lat0], t, [ctx], seq_len)[0].float().clone()
    model.hardware_forward_refactor()
    calls, real = [], fused.quant_rows_mxfp4_project
    monkeypatch.setattr(fused, "quant_rows_mxfp4_project", lambda x, a16, **kw: calls.append(a16.shape[0]) or real(x, a16, **kw))
    monkeypatch.setattr(fused, "quant_rows_mx", lambda *a, **k: pytest.fail("a layer with a branch went to the plain quantiser"))
    hw = model([lat0], t, [ctx], seq_len)[0].float().clone()
    # per block: q + k + v (stacked, 192 ranks), self_attn.o, cross_attn.q, the context's k + v (128), cross_attn.o, ffn.0, ffn.2
    assert sorted(calls) == sorted([192, 64, 64, 128, 64, 64, 64] * 2), calls
    err, noise = rel_l2(hw, sim), rel_l2(sim, ref_fp)
    print(f"MX4 low-rank model, kernel mode vs simulation mode: rel err {err:.3e}; simulation mode vs the floating-point model {noise:.3e}")
    assert noise > 0 and err < 1e-2 and err < 0.5 * noise + 5e-3
