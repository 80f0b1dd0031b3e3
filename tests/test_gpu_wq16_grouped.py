"""The group-wise weight-only GEMM (csrc/gemm_wq16.hip, wanq_gemm_wq16_grouped / qgemm.wq16_grouped_linear) and what is built on
it: the grouped StaticQuantizer, simulation mode of a QuantizedLinear with `weight.group_size`, kernel mode's HipLinearWq16, the
integer checkpoint and the entry scripts with quant_configs/w4a16_g128_all_linears.yaml.

Contract (include/wanq_hip.h):  part_g = sum_{k in group g} a[m,k] (c[n,k] + zp[g,n]);  acc = fma(part_g, sw[g,n], acc), g ascending
from 0;  y = acc + bias;  GELU / gate + residual;  one rounding.  sw, zp fp32 [K / g, N].

The kernel tests call through the C ABI into an output window between two NaN guard regions (tests/test_gpu_wq16.py's Window).
Exact probes: integer activations |a| <= 2, integer c + zp, sw powers of two in 2^-3 .. 2^3 -- every partial and total sum is a
multiple of 2^-3 of magnitude below 2^24 units (checked from the inputs), so every fp32 intermediate is exact in any order and the
output must EQUAL the float64 evaluation.

Bound on random data (profiles/PARITY_NOTES.md, "Group-wise weight-only GEMM"), with S = sum_g |sw[g,n]| (|a| |c + zp|^T)_g[m,n]:
  |y - y64| <= (2^-14 + (K / g) 2^-24) S + 2^-23 |y|   for an fp32 output
-- the per-channel rule of tests/test_gpu_wq16.py applied to each group's partial sum, plus K / g fma roundings of at most 2^-24
of a running sum that never exceeds S -- times 1.13 plus 3e-6 |gelu(y)| through GELU, times |gate| through gate + residual; a
16-bit output one more unit of its type.

The weight quantiser has no host path, so its bit-equality with the oracle on w.view(-1, g) is tested here, on the GPU."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

import test_gpu_wq16 as W
from test_gpu_wq16 import DEV, DT, EPI_GATE_RES, EPI_GELU, PKG, Window, _ULP, gelu64

pytestmark = pytest.mark.gpu
YAML = os.path.join(PKG, "quant_configs", "w4a16_g128_all_linears.yaml")


# ---- operands ---------------------------------------------------------------------------------------------------------
def make_grouped(N, K, gs, w4, gen, scales="pow2", zp_null=False):
    """-> (codes as the kernel reads them, wint = c + zp[g(k), n] float64 [N, K], sw fp32 [K/gs, N], zp fp32 [K/gs, N] or None)"""
    from viditq_extension import qgemm

    G = K // gs
    if w4:
        q = torch.randint(-8, 8, (N, K), device=DEV, generator=gen, dtype=torch.int32).to(torch.int8)
        codes, c = qgemm.pack_w4(q.contiguous(), bias=8), q.double() + 8.0   # stored nibbles u = q + 8
        zp = torch.randint(0, 16, (G, N), device=DEV, generator=gen).float() - 8.0   # the W4 convention: zero_point - 8
    else:
        q = torch.randint(-128, 128, (N, K), device=DEV, generator=gen, dtype=torch.int32).to(torch.int8)
        codes, c = q.contiguous(), q.double()
        zp = torch.randint(-127, 129, (G, N), device=DEV, generator=gen).float()
    if zp_null:
        zp = None
    if scales == "pow2":     # 2^-3 .. 2^3, varying over both indices
        sw = 2.0 ** torch.randint(-3, 4, (G, N), device=DEV, generator=gen).float()
    elif scales == "odd":    # a distinct non-power-of-two per (group, channel)
        sw = (1.0 + (torch.arange(G * N, device=DEV).float().view(G, N) * 2 + 1) / 1024.0) * 0.37
    else:                    # real scales of a quantised weight's size
        sw = (torch.rand(G, N, device=DEV, generator=gen) * 0.01 + 1e-3) * K ** -0.5
    wint = c + (0.0 if zp is None else zp.double().T.repeat_interleave(gs, dim=1))
    return codes, wint, sw.contiguous(), None if zp is None else zp.contiguous()


def ref64(a, wint, sw, gs):
    """(y64, S): the contract in float64 and the sum of absolute group terms"""
    a64, y, S = a.double(), 0.0, 0.0
    for g in range(wint.shape[1] // gs):
        sl = slice(g * gs, (g + 1) * gs)
        y = y + (a64[:, sl] @ wint[:, sl].T) * sw[g].double()
        S = S + (a64[:, sl].abs() @ wint[:, sl].abs().T) * sw[g].double().abs()
    return y, S


def call_abi(a, codes, w4, sw, zp, gs, out_dtype, bias=None, gelu=False, gate=None, residual=None, inplace=False):
    """wanq_gemm_wq16_grouped through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape
    N = codes.shape[0]
    win = Window(M, N, out_dtype)
    if residual is not None and inplace:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_wq16_grouped(
        a.data_ptr(), codes.data_ptr(), DT[a.dtype], 4 if w4 else 8, sw.data_ptr(), None if zp is None else zp.data_ptr(), gs,
        win.out.data_ptr(), DT[out_dtype], None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
        None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


W4S = pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


# ---- 1. exact integer probe ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,gs", [(128, 64), (256, 128), (384, 192)])
@W4S
@DTYPES
def test_exact_probe_equals_the_float64_contract(K, gs, w4, dtype):
    gen = torch.Generator(device=DEV).manual_seed(K + 7 * w4)
    for N in (8, 136):
        for zp_null in (False, True):
            codes, wint, sw, zp = make_grouped(N, K, gs, w4, gen, "pow2", zp_null)
            for M in (1, 129):
                a = torch.randint(-2, 3, (M, K), device=DEV, generator=gen).to(dtype)
                y64, S = ref64(a, wint, sw, gs)
                assert float(S.max()) * 8 < 2.0 ** 24 and torch.equal(y64 * 8, (y64 * 8).round())  # multiples of 2^-3 below 2^24 units
                out = call_abi(a, codes, w4, sw, zp, gs, torch.float32)
                assert torch.equal(out.double(), y64), (M, N, K, gs, zp_null)


# ---- 2. group-boundary probes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,gs", [(256, 128), (128, 64), (384, 192)])
@W4S
@DTYPES
def test_one_hot_rows_identify_the_scale_and_zero_point_of_every_probed_k(K, gs, w4, dtype):
    """row m of a = e_k(m), k over {0, g-1, g, K-1} and the K-tile boundary 63 | 64 (inside a group when g = 128): every other product
    is 0, each group's fold is fma(0, s, acc) = acc or fma(c + zp, s, 0), so
        out[m, n] == fp32(c[n,k] + zp[g(k),n]) * sw[g(k),n]   (one fp32 multiplication, rounded once)
    and, the scales being distinct non-powers-of-two per (group, channel) and the zero points random, a scale or zero point of
    another group or channel gives another value.  M = 200 (ragged second tile) and N = 136 (clamped channel loads in the last
    workgroup)."""
    M, N = 200, 136
    gen = torch.Generator(device=DEV).manual_seed(11 + w4)
    codes, wint, sw, zp = make_grouped(N, K, gs, w4, gen, "odd")
    ks = sorted({0, gs - 1, gs, K - 1, 63, 64})
    k_of = torch.tensor([ks[m % len(ks)] for m in range(M)], device=DEV)
    a = torch.zeros(M, K, device=DEV, dtype=dtype)
    a[torch.arange(M, device=DEV), k_of] = 1
    out = call_abi(a, codes, w4, sw, zp, gs, torch.float32)
    expect = wint.float()[:, k_of].T * sw[k_of // gs]          # fp32 x fp32 -> fp32, [M, N]
    assert expect.dtype == torch.float32 and torch.equal(out, expect)
    other = wint.float()[:, k_of].T * sw[(k_of // gs + 1) % (K // gs)]  # the neighbouring group's scale is told apart
    assert not torch.equal(out, other)


# ---- 3. one group == the per-channel kernel ---------------------------------------------------------------------------------
@W4S
@DTYPES
def test_one_group_is_bit_equal_to_the_per_channel_kernel(w4, dtype):
    M, N, K = 200, 136, 256
    gen = torch.Generator(device=DEV).manual_seed(3 + w4)
    codes, _, sw, zp = make_grouped(N, K, K, w4, gen, "real")
    a = torch.randn(M, K, device=DEV, generator=gen).to(dtype)
    for out_dtype in (torch.float32, dtype):
        twin = W.call_abi(a, codes, w4, sw[0].contiguous(), zp[0].contiguous(), out_dtype)
        assert torch.equal(call_abi(a, codes, w4, sw, zp, K, out_dtype), twin), out_dtype


# ---- 4. random data and the epilogue against float64 ------------------------------------------------------------------------
@W4S
@DTYPES
def test_random_data_and_epilogues_within_the_derived_bound(w4, dtype):
    M, N, K, gs = 200, 136, 512, 128
    gen = torch.Generator(device=DEV).manual_seed(N + K + w4)
    codes, wint, sw, zp = make_grouped(N, K, gs, w4, gen, "real")
    a = torch.randn(M, K, device=DEV, generator=gen).to(dtype)
    bias = torch.randn(N, device=DEV, generator=gen) * 0.1
    gate = torch.rand(N, device=DEV, generator=gen) * 2 - 1
    y0, S = ref64(a, wint, sw, gs)
    s0 = S * (2.0 ** -14 + (K // gs) * 2.0 ** -24) + 2.0 ** -23 * y0.abs()
    for out_dtype in (torch.float32, torch.bfloat16, torch.float16):
        res = torch.randn(M, N, device=DEV, generator=gen).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(a, codes, w4, sw, zp, gs, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None,
                           inplace=gres)  # out aliases residual
            y, s = y0 + bias.double(), s0
            if gelu:
                s = s * 1.13 + 3e-6 * gelu64(y).abs()
                y = gelu64(y)
            if gres:
                y = res.double() + y * gate.double()
                s = s * gate.double().abs()
            tol = s + y.abs() * _ULP[out_dtype] + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
            err = (out.double() - y).abs()
            print(f"grouped w4={w4} {dtype} -> {out_dtype} gelu={gelu} gres={gres}: worst err / bound {(err / tol).max().item():.3f}")
            assert not (err > tol).any(), f"{int((err > tol).sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}"


# ---- 5. rows bit-equal in any launch ----------------------------------------------------------------------------------------
@W4S
def test_rows_are_bit_equal_in_any_launch(w4):
    M, N, K, gs = 200, 136, 512, 128
    gen = torch.Generator(device=DEV).manual_seed(9)
    codes, _, sw, zp = make_grouped(N, K, gs, w4, gen, "real")
    a = torch.randn(M, K, device=DEV, generator=gen).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=gen)
    full = call_abi(a, codes, w4, sw, zp, gs, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, codes, w4, sw, zp, gs, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 199), (77, 100)):
        part = call_abi(a[off:off + m].contiguous(), codes, w4, sw, zp, gs, torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)


# ---- 6. the grouped quantiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [64, 128])
@pytest.mark.parametrize("bits,sym", [(4, False), (8, False), (8, True)])
def test_grouped_static_quantizer_is_the_oracle_on_the_regrouped_weight(gs, bits, sym):
    from oracle import qdiff_ref as qr
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer

    N, K = 16, 256
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(gs + bits)) * 0.05
    wg = w.numpy().reshape(-1, gs)
    delta, zp = qr.static_quant_params(wg, bits, sym)
    q = qr.static_quantize(wg, delta, zp, bits, sym)
    deq, _, _ = qr.static_fake_quant(wg, bits, sym)
    sq = StaticQuantizer(qcfg.create({"n_bits": bits, "sym": sym, "group_size": gs}))
    codes, dq = sq.codes_and_dequant(w.to(DEV))
    assert tuple(sq.delta.shape) == (N, K // gs) and tuple(sq.zero_point.shape) == (N, K // gs)
    assert np.array_equal(sq.delta.cpu().numpy(), delta.reshape(N, -1)) and np.array_equal(sq.zero_point.cpu().numpy(), zp.reshape(N, -1))
    lim = 2 ** (bits - 1)
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (N, K)
    assert np.array_equal(codes.cpu().numpy(), np.clip(q, -lim, lim - 1).reshape(N, K))  # integer storage saturates
    assert np.array_equal(dq.cpu().numpy(), deq.reshape(N, K))
    assert torch.equal(sq(w.to(DEV)), dq) and torch.equal(sq.quantize(w.to(DEV)), codes.float())


def test_groups_of_128_beat_one_scale_per_row_on_outlier_columns():
    """the weight of the issue: [64, 512], N(0, 0.02^2), three columns x 20, 4 bits asymmetric; the oracle alone gives 0.358
    (per row) against 0.197 (groups of 128)"""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer

    w = torch.randn(64, 512, generator=torch.Generator().manual_seed(0)) * 0.02
    w[:, [17, 200, 461]] *= 20.0
    w = w.to(DEV)
    err = {}
    for gs in (None, 128):
        cfg = {"n_bits": 4, "sym": False}
        if gs:
            cfg["group_size"] = gs
        err[gs] = ((StaticQuantizer(qcfg.create(cfg))(w) - w).norm() / w.norm()).item()
    print(f"relative Frobenius error, 4-bit asymmetric: per row {err[None]:.3f}, groups of 128 {err[128]:.3f}")
    assert err[128] < err[None]


# ---- 7. simulation mode -----------------------------------------------------------------------------------------------------
def _sim_layer(gs, bits=4):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    K, N = 256, 136
    gen = torch.Generator().manual_seed(5)
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(torch.randn(N, K, generator=gen) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=gen) * 0.1)
    ql = QuantizedLinear(K, N, True, DEV, qcfg.create({"weight": {"n_bits": bits, "sym": False, "group_size": gs}}), fp, module_name="lin")
    x = torch.randn(1, 33, K, generator=gen).to(torch.bfloat16).to(DEV)
    return ql, x


def test_simulation_forward_is_the_grouped_gemm_on_the_layers_operands():
    from viditq_extension import qgemm

    ql, x = _sim_layer(128)
    K, N, gs = 256, 136, 128
    assert ql.a_quantizer is None and ql.group_size == gs and tuple(ql.w_quantizer.delta.shape) == (N, K // gs)
    codes, sw, zp, w4 = ql.weight_only_operands()
    assert w4 and codes.dtype == torch.uint8 and tuple(sw.shape) == (K // gs, N) and tuple(zp.shape) == (K // gs, N)
    assert ql.weight_only_operands()[1] is sw  # made once
    assert torch.equal(sw, ql.w_quantizer.delta.t()) and torch.equal(zp, ql.w_quantizer.zero_point.t() - 8.0)
    out = ql(x)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 33, N)
    assert torch.equal(out[0], qgemm.wq16_grouped_linear(x[0].contiguous(), codes, sw, zp, gs, ql.bias.detach(), w4=True))
    # F.linear on the dequantised weight, in float64: the bound of the header, plus 2^-24 S for the fp32 rounding of
    # (c + zp) * delta in weight.data, plus the bf16 output's unit
    wint = qgemm.unpack_w4(codes, bias=0).double() + zp.double().T.repeat_interleave(gs, dim=1)
    y0, S = ref64(x[0], wint, sw, gs)
    y = x[0].double() @ ql.weight.data.double().T + ql.bias.double()
    tol = S * (2.0 ** -14 + (K // gs + 1) * 2.0 ** -24) + 2.0 ** -23 * y0.abs() + y.abs() * 2.0 ** -7
    assert not ((out[0].double() - y).abs() > tol).any()


def test_a_group_size_the_kernel_does_not_take_falls_back_to_f_linear():
    ql, x = _sim_layer(32)
    assert tuple(ql.w_quantizer.delta.shape) == (136, 8)
    want = torch.nn.functional.linear(x, ql.weight.to(torch.bfloat16), ql.bias.to(torch.bfloat16))
    assert torch.equal(ql(x), want)


# ---- 8. kernel mode -----------------------------------------------------------------------------------------------------------
def _group_cfg(gs, bits=4):
    from qdiff import config as qcfg

    cfg = qcfg.load(YAML)
    cfg.weight.group_size, cfg.weight.n_bits = gs, bits
    return cfg


def test_kernel_mode_block_within_the_bar_of_the_per_channel_block_test(monkeypatch):
    """tests/test_gpu_wq16.py's weight-only block test (kernel-mode block against the float64 block on the dequantised weights; bar:
    1.5 x the FP block's error against its own oracle) with every Linear quantised in groups of 128: its config and its oracle's
    fake-quant are replaced by the group-wise ones, nothing else."""
    from oracle import qdiff_ref as qr
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearWq16

    gs, plain = 128, qr.static_fake_quant

    def grouped_fake_quant(w, n_bits=8, sym=False, params=None):
        deq, d, z = plain(np.asarray(w).reshape(-1, gs), n_bits, sym)
        return deq.reshape(np.asarray(w).shape), d, z

    monkeypatch.setattr(W, "_wq_config", lambda bits: qcfg.create({"weight": {"n_bits": bits, "sym": False, "group_size": gs}}))
    monkeypatch.setattr(qr, "static_fake_quant", grouped_fake_quant)
    seen = []
    real = HipLinearWq16.forward
    monkeypatch.setattr(HipLinearWq16, "forward", lambda self, *a, **k: (seen.append(self.group_size), real(self, *a, **k))[1])
    W.test_kernel_mode_block_weight_only_vs_float64_oracle(4, torch.bfloat16)
    assert len(seen) >= 10 and set(seen) == {gs}  # every Linear of the block ran the group-wise GEMM


def _tiny_model(cfg, build=True, dim=256, ffn=512, heads=2):
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=2, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 3, 20, 18)
    ctx = torch.randn(24, 64, device=DEV, generator=g) * 0.1
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, cfg)
    model.quant_layer_refactor()
    model.set_init_done()
    if build:
        model.hardware_forward_refactor()
    return model, seq_len_for(shape), ctx, lat0


def test_checkpoint_round_trip_is_bit_equal(tmp_path, caplog):
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearWq16

    model, seq_len, ctx, lat0 = _tiny_model(qcfg.load(YAML))
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearWq16)]
    assert len(lins) == 20 and all(m.group_size == 128 and tuple(m.scale_weight.shape) == (m.in_features // 128, m.out_features) for m in lins)
    t = torch.tensor([700], device=DEV)
    want = model([lat0], t, [ctx], seq_len)[0].clone()
    assert torch.isfinite(want).all()
    sim = model.blocks[0].ffn[2]   # kernel mode took the simulation layer's parameters over, transposed
    assert torch.equal(model.hip_blocks[0].ffn2.scale_weight, sim.w_quantizer.delta.t())
    assert torch.equal(model.hip_blocks[0].ffn2.zp_gemm, sim.w_quantizer.zero_point.t() - 8.0)
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.2.weight"].dtype == torch.uint8 and tuple(sd["blocks.0.ffn.2.scale_weight"].shape) == (4, 256)
    assert tuple(sd["blocks.0.ffn.2.zp_weight"].shape) == (4, 256) and sd["blocks.0.ffn.2.scale_weight"].dtype == torch.float32
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q.*weight\.group_size"):
        model.quantize_and_save_weight(None, reference_format=True)
    fresh, *_ = _tiny_model(qcfg.load(YAML), build=False)
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=path)
    assert any("loaded 80 tensors" in r.getMessage() and "80 of them into weight-only layers" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, [ctx], seq_len)[0], want)


def test_a_group_size_of_96_has_no_kernel_mode_form_and_the_layer_is_named():
    """(96 must divide in_features for the layer to exist at all -- a group size that does not is refused when the simulation layer
    is built -- so this model is 3 heads of 128: dim 384, ffn 768.)  Simulation mode runs such a layer through F.linear."""
    model, seq_len, ctx, lat0 = _tiny_model(_group_cfg(96), build=False, dim=384, ffn=768, heads=3)
    assert tuple(model.blocks[0].self_attn.q.w_quantizer.delta.shape) == (384, 4)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q: weight\.group_size=96"):
        model.hardware_forward_refactor()
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q: weight\.group_size=96 does not divide in_features=256"):
        _tiny_model(_group_cfg(96), build=False)


def test_entry_point_chain_with_the_grouped_config(tmp_path):
    """fp_generate -> ptq_wanx -> quant_generate with quant_configs/w4a16_g128_all_linears.yaml, kernel mode and simulation mode (the
    helpers and the 3e-2 bar between the two modes are those of tests/test_gpu_wq16.py's W4A16 chain)."""
    W._entry("fp_generate.py", cwd=tmp_path)
    fp = torch.load(tmp_path / "fp_latent_0.pt", weights_only=True)
    W._entry("ptq_wanx.py", "--quant_config", YAML, cwd=tmp_path)
    qp = torch.load(tmp_path / "checkpoint" / "quant_params.pth", weights_only=True)
    assert sum(k.endswith("w_quantizer") for k in qp) == 20 and not any(k.endswith("a_quantizer") for k in qp)
    assert qp["blocks.0.ffn.2.w_quantizer"]["delta"].shape == (1536, 8960 // 128)
    iw = torch.load(tmp_path / "checkpoint" / "int_weight.pt", weights_only=True)
    assert iw["blocks.0.ffn.0.weight"].dtype == torch.uint8 and tuple(iw["blocks.0.ffn.0.weight"].shape) == (8960, 1536 // 2)
    assert tuple(iw["blocks.0.ffn.0.scale_weight"].shape) == (1536 // 128, 8960) == tuple(iw["blocks.0.ffn.0.zp_weight"].shape)
    log = W._entry("quant_generate.py", "--quant_config", YAML, cwd=tmp_path)
    assert "loaded 80 tensors" in log and "80 of them into weight-only layers" in log
    hw = torch.load(tmp_path / "quant_latent_0.pt", weights_only=True)
    assert hw.shape == fp.shape and torch.isfinite(hw).all() and not torch.equal(hw, fp)
    W._entry("quant_generate.py", "--quant_config", YAML, "--hardware", "false", "--save_file", str(tmp_path / "sim.pt"), cwd=tmp_path)
    sim = torch.load(tmp_path / "sim.pt", weights_only=True)
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    print(f"w4a16 g128: kernel-mode vs fp {rel(hw, fp):.3e}; simulation-mode vs fp {rel(sim, fp):.3e}; kernel vs simulation {rel(hw, sim):.3e}")
    assert torch.isfinite(sim).all() and not torch.equal(sim, fp) and rel(hw, sim) < 0.03
