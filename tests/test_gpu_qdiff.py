"""GPU parity of the qdiff drop-in modules (real int8 compute) against golden vectors produced by the
reference's own fake-quant modules, and of the fused ViDiT transform kernel against the oracle."""
import numpy as np
import pytest
import torch

from oracle import qdiff_ref as qr

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_grad_enabled(False)


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.to(dtype) if dtype is not None else x


def cfg(**extra):
    from qdiff import config as qcfg

    return qcfg.create(dict({"weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": 8, "sym": True}}, **extra))


@pytest.mark.parametrize("n", [1536, 5120, 8960, 13824])
def test_rotation_kernel_vs_reference_hadamard_products(golden, n):
    """out_fp of wanq_rotate_quant_rows == hadU(x) of the reference (golden a5), fp32 vs fp64: 1e-5.  (13824: repo-defined K = 108 --
    the fixture is made from the reference's own get_had108 table and butterfly, tests/golden/make_golden_had108.py.)"""
    import viditq_extension.fused as fused
    from qdiff.quarot import quarot_utils as qu

    g = golden(f"a5_hadamard_{n}")
    x = t(g["x"], torch.float32)
    rot = qu.kernel_rotation_params(n, DEV)
    out = torch.empty_like(x)
    fused.rotate_quant(x, None, rot, None, None, out_fp=out, quantize=False)
    np.testing.assert_allclose(out.cpu().numpy(), g["hadU_x"], rtol=0, atol=2e-5)
    # with a sign pre-multiplier it is x @ R
    s = t(g["signs"], torch.float32)
    fused.rotate_quant(x, s, rot, None, None, out_fp=out, quantize=False)
    ref = qr.matmul_hadU(g["x"].astype(np.float64) * g["signs"], strict=False)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=2e-5)


@pytest.mark.parametrize("n,rows", [(1536, 131), (5120, 37), (4096, 16), (128, 9), (8960, 1), (8960, 1031)])
def test_rotate_quant_codes_vs_oracle(n, rows):
    import viditq_extension.fused as fused
    from qdiff.quarot import quarot_utils as qu

    g = torch.Generator().manual_seed(n)
    x = torch.randn(rows, n, generator=g) * torch.exp(torch.randn(n, generator=g))
    pm = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    ref = qr.matmul_hadU((x.double() * pm.double()).numpy()).astype(np.float32)
    oq, oscale = qr.dynamic_quantize_sym(ref)
    scale = torch.zeros(rows, device=DEV)
    ssum = torch.zeros(rows, device=DEV)
    q = fused.rotate_quant(x.to(DEV), pm.to(DEV), qu.kernel_rotation_params(n, DEV), ssum, scale)
    np.testing.assert_allclose(scale.cpu().numpy(), oscale, rtol=2e-6)
    d = np.abs(q.cpu().numpy().astype(np.int32) - oq)
    assert d.max() <= 1 and (d != 0).mean() < 2e-3  # fp32 transform vs fp64: codes move only at .5 boundaries
    np.testing.assert_allclose(ssum.cpu().numpy(), q.cpu().numpy().astype(np.int64).sum(1) * scale.cpu().numpy().astype(np.float64), rtol=1e-6, atol=1e-6)


def test_layernorm_rotate_quant_vs_oracle():
    import viditq_extension.fused as fused
    from oracle import kernel_ref as kr
    from qdiff.quarot import quarot_utils as qu

    n, rows = 1536, 70
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, n, generator=g) * 2 + 0.1
    sh, sc = torch.randn(1, n, generator=g) * 0.2, torch.randn(1, n, generator=g) * 0.2
    pm = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    h = kr.layernorm_t2i(x.numpy(), None, sh.numpy(), sc.numpy(), 1e-6, rows)
    ref = qr.matmul_hadU(h * pm.double().numpy()).astype(np.float32)
    oq, oscale = qr.dynamic_quantize_sym(ref)
    q = torch.empty(rows, n, dtype=torch.int8, device=DEV)
    scale, ssum = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    fused.layernorm_rotate_quant(q, x.to(DEV), None, sh.to(DEV), sc.to(DEV), pm.to(DEV), qu.kernel_rotation_params(n, DEV), ssum, scale, 1e-6)
    np.testing.assert_allclose(scale.cpu().numpy(), oscale, rtol=1e-5)
    d = np.abs(q.cpu().numpy().astype(np.int32) - oq)
    assert d.max() <= 1 and (d != 0).mean() < 3e-3


@pytest.mark.parametrize("n,rows", [(1536, 70), (5120, 9), (256, 5)])
def test_layernorm_rotate_quant_multi_equals_three_single_calls(n, rows):
    """One pass over x for the q / k / v consumers of a block == three independent passes, bit for bit (codes, scales,
    sums), including ragged row counts (surplus waves of the last workgroup) and the 4-waves-per-row variant (5120)."""
    import viditq_extension.fused as fused
    from qdiff.quarot import quarot_utils as qu

    g = torch.Generator().manual_seed(n + rows)
    x = (torch.randn(rows, n, generator=g) * 2 + 0.1).to(DEV)
    sh, sc = (torch.randn(1, n, generator=g) * 0.2).to(DEV), (torch.randn(1, n, generator=g) * 0.2).to(DEV)
    pms = [((torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).to(DEV) for _ in range(3)]
    rot = qu.kernel_rotation_params(n, DEV)
    single = []
    for pm in pms:
        q = torch.empty(rows, n, dtype=torch.int8, device=DEV)
        scale, ssum = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        fused.layernorm_rotate_quant(q, x, None, sh, sc, pm, rot, ssum, scale, 1e-6)
        single.append((q, scale, ssum))
    for k in (2, 3):
        qs = [torch.empty(rows, n, dtype=torch.int8, device=DEV) for _ in range(k)]
        scales, sums = [torch.zeros(rows, device=DEV) for _ in range(k)], [torch.zeros(rows, device=DEV) for _ in range(k)]
        fused.layernorm_rotate_quant_multi(qs, x, None, sh, sc, pms[:k], rot, sums, scales, 1e-6)
        for i in range(k):
            assert torch.equal(qs[i], single[i][0]) and torch.equal(scales[i], single[i][1]) and torch.equal(sums[i], single[i][2])
    with pytest.raises(RuntimeError):
        fused.layernorm_rotate_quant_multi([single[0][0]] * 4, x, None, sh, sc, pms + pms[:1], rot, [single[0][2]] * 4, [single[0][1]] * 4, 1e-6)


def test_quantized_linear_vs_reference_golden(golden):
    """qdiff.QuantizedLinear (int8 GEMM inside) == the reference's QuantizedLinear.forward output (golden a3)."""
    from qdiff.base.quant_layer import QuantizedLinear

    g = golden("a3_qlinear")
    lin = torch.nn.Linear(64, 48).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"]), t(g["b"])
    ql = QuantizedLinear(64, 48, True, DEV, cfg(), lin)
    assert np.array_equal(ql.weight.data.cpu().numpy(), g["w_dequant"])  # the fake-quantised weight, bit for bit
    assert np.array_equal(ql.w_quantizer.delta.reshape(-1).cpu().numpy(), g["w_delta"])
    assert np.array_equal(ql.w_quantizer.zero_point.reshape(-1).cpu().numpy(), g["w_zp"])
    y = ql(t(g["x"]))
    assert y.shape == g["y"].shape
    np.testing.assert_allclose(y.cpu().numpy(), g["y"], rtol=2e-5, atol=2e-5)
    # quantizers on their own follow the reference API
    x2 = t(g["x"]).reshape(-1, 64)
    deq = ql.a_quantizer(x2)
    np.testing.assert_array_equal(deq.cpu().numpy(), qr.dynamic_fake_quant_sym(g["x"].reshape(-1, 64)))
    assert ql.a_quantizer.delta.shape == (33, 1)
    ql.quant_mode = False
    np.testing.assert_allclose(ql(t(g["x"])).cpu().numpy(), (g["x"] @ g["w"].T + g["b"]), rtol=1e-4, atol=1e-4)


def test_viditq_linear_vs_reference_golden(golden):
    """ViDiTQuantizedLinear at in_features 1536: channel mask, double-quantised rotated weight and forward output
    against what the reference's own module produced (golden a4_viditq_1536)."""
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    g = golden("a4_viditq_1536")
    n, out = 1536, 24
    lin = torch.nn.Linear(n, out).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"]), t(g["b"])
    vl = ViDiTQuantizedLinear(n, out, True, DEV, cfg(viditq={"alpha": 0.5665, "layer_name_regex": ""}), lin)
    vl.get_channel_mask(t(g["act_mask"]))
    np.testing.assert_allclose(vl.channel_mask.cpu().numpy(), g["channel_mask"], rtol=3e-7)  # powf ulp
    vl.channel_mask = t(g["channel_mask"])
    vl.rotation_signs = torch.from_numpy(g["signs"])
    vl.update_quantized_weight_rotated_and_scaled()
    assert np.array_equal(vl.w_quantizer.delta.reshape(-1).cpu().numpy(), g["w_delta"])
    assert np.array_equal(vl.w_quantizer.zero_point.reshape(-1).cpu().numpy(), g["w_zp"])
    assert np.array_equal(vl.weight.data.cpu().numpy(), g["w_final"])
    # activation codes: fp32 fast transform vs the reference's fp64 dense product
    q, scale, _ = vl.a_quantizer.quantize_int8(t(g["x"]).reshape(-1, n), *vl._act_transform())
    np.testing.assert_allclose(scale.cpu().numpy(), g["x_delta"], rtol=2e-6)
    d = np.abs(q.cpu().numpy().astype(np.int32) - g["x_q"].astype(np.int32))
    assert d.max() <= 1 and (d != 0).mean() < 2e-3
    y = vl(t(g["x"]))
    # one flipped code changes y by <= delta_x * |w|: compare at the level of the quantisation step
    assert np.abs(y.cpu().numpy() - g["y"]).max() < 5e-3 * np.abs(g["y"]).max() + 1e-3
    # rotation_matrix property materialises the reference's matrix
    R = vl.rotation_matrix
    np.testing.assert_allclose(R.cpu().numpy()[[0, 1, 777, n - 1]], qr.hadamard_from_signs(g["signs"])[[0, 1, 777, n - 1]], atol=1e-15)


def test_rotate_8960_dtypes_and_outputs():
    """n = 8960 = 140 x 64 (csrc/rotate_paley.hip: Paley-140 mix on the matrix cores with a three-way bf16 split of the fp32
    values): bf16 / fp16 input as the GELU output has it, fp output in every dtype, scale / sum vectors in fp16 too."""
    import viditq_extension.fused as fused
    from qdiff.quarot import quarot_utils as qu

    n, rows = 8960, 67
    g = torch.Generator().manual_seed(8960)
    x = (torch.randn(rows, n, generator=g) * torch.exp(0.7 * torch.randn(n, generator=g))).clamp_min(-0.17)  # GELU-like
    x[5] = 0  # an all-zero token: the eps rule
    pm = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    rot = qu.kernel_rotation_params(n, DEV)
    assert rot[0] == 140
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        xd = x.to(dt)
        ref = qr.matmul_hadU(xd.double().numpy() * pm.double().numpy())
        oq, oscale = qr.dynamic_quantize_sym(ref.astype(np.float32))
        scale, ssum = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        out = torch.empty(rows, n, device=DEV)
        q = fused.rotate_quant(xd.to(DEV), pm.to(DEV), rot, ssum, scale, out_fp=out)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=3e-6 * np.abs(ref).max())
        np.testing.assert_allclose(scale.cpu().numpy(), oscale, rtol=2e-6)
        d = np.abs(q.cpu().numpy().astype(np.int32) - oq)
        assert d.max() <= 1 and (d != 0).mean() < 2e-3
        np.testing.assert_allclose(ssum.cpu().numpy(), q.cpu().numpy().astype(np.int64).sum(1) * scale.cpu().numpy().astype(np.float64),
                                   rtol=1e-6, atol=1e-6)
        assert scale[5].item() == pytest.approx(1e-6) and int(q[5].abs().max()) == 0
    # 16-bit fp output and fp16 vectors
    for odt in (torch.bfloat16, torch.float16):
        out = torch.empty(rows, n, dtype=odt, device=DEV)
        s16, m16 = torch.zeros(rows, dtype=torch.float16, device=DEV), torch.zeros(rows, dtype=torch.float16, device=DEV)
        fused.rotate_quant(x.to(DEV), pm.to(DEV), rot, m16, s16, out_fp=out)
        ref = qr.matmul_hadU(x.double().numpy() * pm.double().numpy())
        np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=2 ** -8, atol=1e-6)
        np.testing.assert_allclose(s16.float().cpu().numpy(), np.maximum(np.abs(ref).max(1) / 127, 1e-6), rtol=2e-3, atol=1e-7)
    # the LayerNorm forms have no 8960 variant (no model dimension is 8960): refused, not mis-computed
    with pytest.raises(RuntimeError, match="8960"):
        fused.layernorm_rotate_quant(torch.empty(4, n, dtype=torch.int8, device=DEV), x[:4].to(DEV), None, None, None, pm.to(DEV), rot,
                                     torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), 1e-6)


def test_viditq_linear_8960_vs_oracle():
    """The 1.3B ffn.2 shape (in_features 8960) as a ViDiT layer: mask, double-quantised rotated weight and forward vs the
    oracle (x @ R evaluated as hadU(x * signs): quarot_utils.py:186-192)."""
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    n, out, rows = 8960, 48, 33
    g = torch.Generator().manual_seed(140)
    w = torch.randn(out, n, generator=g) * 0.02 * torch.exp(0.5 * torch.randn(n, generator=g))
    b = torch.randn(out, generator=g) * 0.1
    x = torch.randn(rows, n, generator=g) * torch.exp(0.8 * torch.randn(n, generator=g))
    act_mask = x.abs().amax(0).clamp_min(1e-3)
    signs = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    lin = torch.nn.Linear(n, out).to(DEV)
    lin.weight.data, lin.bias.data = w.to(DEV), b.to(DEV)
    vl = ViDiTQuantizedLinear(n, out, True, DEV, cfg(viditq={"alpha": 0.5665, "layer_name_regex": ""}), lin)
    vl.get_channel_mask(act_mask.to(DEV))
    mask = qr.vidit_channel_mask(w.numpy(), act_mask.numpy(), 0.5665)
    np.testing.assert_allclose(vl.channel_mask.cpu().numpy(), mask, rtol=3e-7)
    vl.channel_mask = torch.from_numpy(mask).to(DEV)
    vl.rotation_signs = signs
    vl.update_quantized_weight_rotated_and_scaled()
    w1, _, _ = qr.static_fake_quant((w.numpy() / mask[None, :]).astype(np.float32), 8, False)
    w2in = qr.matmul_hadU(w1.astype(np.float64) * signs.numpy()[None, :]).astype(np.float32)
    # the kernel's transform is fp32: the rotated weight is within an ulp or two of the fp64 product, so delta / zp agree to
    # rounding and a code moves only at a .5 boundary
    w2, d2, z2 = qr.static_fake_quant(w2in, 8, False)
    np.testing.assert_allclose(vl.w_quantizer.delta.reshape(-1).cpu().numpy(), d2.reshape(-1), rtol=2e-6)
    dw = np.abs(vl.weight.data.cpu().numpy() - w2) / d2.reshape(-1, 1)
    assert dw.max() <= 1.0 + 1e-3 and (dw > 0.5).mean() < 2e-3
    xt = qr.matmul_hadU((x.numpy() * mask[None, :]).astype(np.float32).astype(np.float64) * signs.numpy()[None, :]).astype(np.float32)
    xq, xs = qr.dynamic_quantize_sym(xt)
    y_ref = (xq.astype(np.float64) * xs[:, None]) @ w2.astype(np.float64).T + b.numpy()
    y = vl(x.to(DEV))
    assert np.abs(y.cpu().numpy() - y_ref).max() < 5e-3 * np.abs(y_ref).max() + 1e-3


def test_surgery_save_load_roundtrip_and_mixed_precision():
    """quant_layer_refactor_ / save / load / bitwidth_refactor_ on a toy module tree."""
    import torch.nn as nn

    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from qdiff.base.quant_model import QuantModel
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    class Toy(QuantModel):
        def __init__(self, q_cfg):
            nn.Module.__init__(self)
            self.q_cfg = q_cfg
            self.blocks = nn.ModuleList([nn.ModuleDict({"q": nn.Linear(1536, 64), "ffn": nn.Linear(64, 64)}) for _ in range(2)])
            self.head = nn.Linear(64, 8)

        def forward(self, x):
            return self.head(sum(b["ffn"](b["q"](x)) for b in self.blocks))

    torch.manual_seed(0)
    c = cfg(viditq={"alpha": 0.5665, "layer_name_regex": r"\.q$"}, remain_fp_regex="head")
    m = Toy(c).to(DEV)
    fp_state = {k: v.clone() for k, v in m.state_dict().items()}
    m.quant_layer_refactor()
    assert isinstance(m.blocks[0]["q"], ViDiTQuantizedLinear) and type(m.blocks[1]["ffn"]) is QuantizedLinear
    assert type(m.head) is nn.Linear and m.blocks[0]["q"].module_name == "blocks.0.q"
    for b in m.blocks:
        b["q"].get_channel_mask(torch.rand(1536, device=DEV) + 0.5)
        b["q"].get_rotation_matrix()
        b["q"].update_quantized_weight_rotated_and_scaled()
    m.set_init_done()
    x = torch.randn(1, 50, 1536, device=DEV)
    y0 = m(x)
    d = m.save_quant_param_dict()
    assert set(d) == {f"blocks.{i}.{l}.{q}" for i in range(2) for l in ("q", "ffn") for q in ("w_quantizer", "a_quantizer")}
    assert d["blocks.0.q.w_quantizer"]["rotation_matrix"] is None and d["blocks.0.q.w_quantizer"]["channel_mask"].shape == (1536,)
    # a fresh model with the same FP weights + the saved dict reproduces the outputs exactly
    m2 = Toy(c).to(DEV)
    m2.load_state_dict(fp_state)
    m2.quant_layer_refactor()
    m2.load_quant_param_dict({k: {kk: (vv.cpu() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in d.items()})
    m2.set_init_done()
    assert torch.equal(m2(x), y0)

    # mixed precision: ffn weights to 4 bit
    cm = qcfg.create({"weight": {"n_bits": [4, 8], "i_bitwidth": 1, "sym": False}, "act": {"n_bits": 8, "sym": True},
                      "remain_fp_regex": "head",
                      "mixed_precision": {"weight": {"layer_name_regex": ["", "ffn", ""]}, "act": {"layer_name_regex": ["", ""]}}})
    m3 = Toy(cm).to(DEV)
    m3.quant_layer_refactor()
    w8 = m3.blocks[0]["ffn"].int_weight.clone()
    m3.bitwidth_refactor()
    f = m3.blocks[0]["ffn"]
    assert f.w_quantizer.n_bits == 4 and f.int_weight.min() >= -8 and f.int_weight.max() <= 7 and not torch.equal(w8, f.int_weight)
    assert m3.blocks[0]["q"].w_quantizer.n_bits == 8
    deq = qr.static_fake_quant(f.fp_module.weight.data.cpu().numpy(), 4, False)[0]
    assert np.array_equal(f.weight.data.cpu().numpy(), deq)
    assert torch.isfinite(m3(x)).all()


@pytest.mark.parametrize("name", ["a1_static_16x64", "a1_static_12x1536"])
def test_reference_format_export_vs_reference_golden(golden, name):
    """wanq_weight_export_f16 == quantize_and_save_weight_ of the reference (W/wan/quant_wanx_cuda.py:39-53), bit for bit:
    fp16 weight / fp16 delta in half arithmetic, minus the fp16 zero point, clamped to int8 (fixture a12_*, generated by the
    reference's own four-line equation on the reference quantizer's delta / zero_point)."""
    import viditq_extension.fused as fused

    g = golden(name)  # a missing fixture is a failure (FileNotFoundError), never a skip
    assert "a12_int_weight" in g, f"{name}.npz carries no a12 vectors: regenerate it with tests/golden/make_golden.py"
    w = t(g["w"], torch.float32)
    s16 = torch.from_numpy(g["a12_scale_f16"]).to(DEV)
    z16 = torch.from_numpy(g["a12_zp_f16"]).to(DEV)
    assert s16.dtype == torch.float16 and z16.dtype == torch.float16
    q = fused.weight_export_f16(w, s16, z16)
    assert np.array_equal(q.cpu().numpy(), g["a12_int_weight"])
    # a fp16 copy of the weight gives the same codes (the equation starts by casting the weight to half)
    assert torch.equal(fused.weight_export_f16(w.half(), s16, z16), q)


def test_refresh_keeps_rotated_weights_consistent_under_mixed_precision():
    """bitwidth_refactor_ on a ViDiT layer: after the weight drops to 4 bit, the integer codes must still be
    those of the scaled + rotated weight (the activations keep being rotated), i.e. refresh() takes the layer's own PTQ
    derivation.  Checked against the fake-quant oracle with the same mask / signs at 4 bit."""
    import torch.nn as nn

    from qdiff import config as qcfg
    from qdiff.base.quant_model import bitwidth_refactor_, quant_layer_refactor_
    from qdiff.utils import apply_func_to_submodules

    n, N = 1536, 96
    torch.manual_seed(5)
    holder = nn.ModuleDict({"ffn": nn.Linear(n, N)}).to(DEV)
    c = qcfg.create({"weight": {"n_bits": [4, 8], "i_bitwidth": 1, "sym": False}, "act": {"n_bits": 8, "sym": True},
                     "viditq": {"alpha": 0.5665, "layer_name_regex": ""},
                     "mixed_precision": {"weight": {"layer_name_regex": ["", "ffn", ""]}, "act": {"layer_name_regex": ["", ""]}}})
    apply_func_to_submodules(holder, nn.Linear, quant_layer_refactor_, name=None, parent_module=None, quant_config=c,
                             full_name=None, remain_fp_regex=None)
    lin = holder["ffn"]
    g = torch.Generator().manual_seed(6)
    act_mask = torch.rand(n, generator=g) * 3 + 0.2
    lin.get_channel_mask(act_mask.to(DEV))
    lin.get_rotation_matrix(g)
    lin.update_quantized_weight_rotated_and_scaled()
    apply_func_to_submodules(holder, type(lin), bitwidth_refactor_, name=None, parent_module=None, quant_config=c, full_name=None)
    assert lin.w_quantizer.n_bits == 4 and lin.int_weight.min() >= -8 and lin.int_weight.max() <= 7
    R = qr.hadamard_from_signs(lin.rotation_signs.numpy())
    w = lin.fp_module.weight.data.cpu().numpy()
    mask = lin.channel_mask.cpu().numpy()
    w_final = qr.vidit_weight(w, mask, R, 4, False)
    w_final = w_final[0] if isinstance(w_final, tuple) else w_final
    got = lin.weight.data.cpu().numpy()
    assert np.abs(got - w_final).max() <= 1e-6 * np.abs(w_final).max() + 1e-7, np.abs(got - w_final).max()
    x = torch.randn(40, n, generator=g) * 2
    y = lin(x.to(DEV))
    ref = qr.vidit_linear(x.numpy()[None], w_final, lin.bias.detach().cpu().numpy(), mask, R)
    ref = ref[0] if ref.ndim == 3 else ref
    assert np.abs(y.cpu().numpy() - ref).max() < 2e-2 * np.abs(ref).max()


def test_surgery_and_param_dict_vs_reference_golden(golden):
    """quant_layer_refactor_ / save_quant_param_dict_ / bitwidth_refactor_ on a toy tree with Wan's module names, driven with the
    keyword arguments QuantWanModel uses, against what the reference's own functions did on the same tree (fixture a6_surgery):
    which Linear becomes which class under the reference's shipped config.yaml, the quant_param_dict's keys and shapes (our extra
    `rotation_signs` entry aside), and per-layer bit-width / quant_mode under a mixed-precision config."""
    import json

    import torch.nn as nn
    import yaml

    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import BaseQuantizer
    from qdiff.base.quant_layer import QuantizedLinear
    from qdiff.base.quant_model import bitwidth_refactor_, quant_layer_refactor_, save_quant_param_dict_
    from qdiff.utils import apply_func_to_submodules

    ref = json.loads(str(golden("a6_surgery")["json"]))

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.q, self.k, self.v, self.o = (nn.Linear(256, 256) for _ in range(4))

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn, self.cross_attn = Attn(), Attn()
            self.ffn = nn.Sequential(nn.Linear(256, 512), nn.GELU(approximate="tanh"), nn.Linear(512, 256))

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.head = nn.Linear(256, 64)

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.text_embedding = nn.Sequential(nn.Linear(64, 256), nn.GELU(approximate="tanh"), nn.Linear(256, 256))
            self.time_embedding = nn.Sequential(nn.Linear(64, 256), nn.SiLU(), nn.Linear(256, 256))
            self.time_projection = nn.Sequential(nn.SiLU(), nn.Linear(256, 1536))
            self.blocks = nn.ModuleList([Block(), Block()])
            self.head = Head()
            self.quant_param_dict = {}

    def refactor(model, c):
        apply_func_to_submodules(model, class_type=nn.Linear, function=quant_layer_refactor_, name=None, parent_module=None,
                                 quant_config=c, full_name=None, remain_fp_regex=c.remain_fp_regex)

    def classes(model):
        return {n: type(m).__name__ for n, m in model.named_modules() if isinstance(m, nn.Linear) or hasattr(m, "w_quantizer")}

    # (1) the reference's shipped Wan config, verbatim
    import os
    with open(os.path.join(os.path.dirname(__file__), "..", "wan2.1-quantization_amd", "quant_configs", "config.yaml")) as fh:
        wan_cfg = qcfg.create(yaml.safe_load(fh))
    torch.manual_seed(6)
    m = Toy().to(DEV)
    refactor(m, wan_cfg)
    mine = classes(m)
    # the reference keeps the wrapped nn.Linear as `.fp_module` of every quantized layer: those names appear in both maps
    assert mine == ref["wan_config_classes"]
    g = torch.Generator().manual_seed(7)
    for n, mod in m.named_modules():
        if type(mod).__name__ == "ViDiTQuantizedLinear":
            mod.get_channel_mask((torch.rand(mod.in_features, generator=g) + 0.5).to(DEV))
            mod.rotation_signs = torch.randint(0, 2, (mod.in_features,), generator=g).double() * 2 - 1
            mod.update_quantized_weight_rotated_and_scaled()
    apply_func_to_submodules(m, class_type=BaseQuantizer, function=save_quant_param_dict_, full_name=None, parent_module=None, model=m)
    shapes = {k: {kk: (None if vv is None else list(vv.shape)) for kk, vv in v.items() if kk != "rotation_signs"} for k, v in m.quant_param_dict.items()}
    assert shapes == ref["wan_config_param_dict"]
    assert all("rotation_signs" in v for v in m.quant_param_dict.values())  # ours in addition: the rotation is rebuilt from it exactly
    # (2) mixed precision
    mp = qcfg.create({"remain_fp_regex": r"text_embedding|time_embedding|time_projection|head\.head",
                      "weight": {"n_bits": [4, 8], "i_bitwidth": 1, "sym": False}, "act": {"n_bits": 8, "sym": True},
                      "mixed_precision": {"weight": {"layer_name_regex": [r"cross_attn\.o", "ffn", ""]}, "act": {"layer_name_regex": ["", ""]}}})
    torch.manual_seed(6)
    m2 = Toy().to(DEV)
    refactor(m2, mp)
    apply_func_to_submodules(m2, class_type=QuantizedLinear, function=bitwidth_refactor_, name=None, parent_module=None, quant_config=mp, full_name=None)
    assert classes(m2) == ref["mixed_classes"]
    bits = {n: {"w_bits": int(mod.w_quantizer.n_bits), "quant_mode": bool(mod.quant_mode)} for n, mod in m2.named_modules() if hasattr(mod, "w_quantizer")}
    assert bits == ref["mixed_bits"]


def test_smoothquant_linear_vs_reference_golden(golden):
    """SQQuantizedLinear (channel mask only) at in_features 1536 against the reference's own module (fixture a4_smoothquant_1536):
    mask, scaled + quantised weight bit for bit, forward output."""
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear

    g = golden("a4_smoothquant_1536")
    n, out = 1536, 24
    lin = torch.nn.Linear(n, out).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"]), t(g["b"])
    sq = SQQuantizedLinear(n, out, True, DEV, cfg(smooth_quant={"alpha": 0.5, "layer_name_regex": ""}), lin)
    sq.get_channel_mask(t(g["act_mask"]))
    np.testing.assert_allclose(sq.channel_mask.cpu().numpy(), g["channel_mask"], rtol=3e-7)  # powf ulp
    sq.channel_mask = t(g["channel_mask"])
    sq.update_quantized_weight_scaled()
    assert np.array_equal(sq.w_quantizer.delta.reshape(-1).cpu().numpy(), g["w_delta"])
    assert np.array_equal(sq.w_quantizer.zero_point.reshape(-1).cpu().numpy(), g["w_zp"])
    assert np.array_equal(sq.weight.data.cpu().numpy(), g["w_final"])
    y = sq(t(g["x"]))
    assert np.abs(y.cpu().numpy() - g["y"]).max() < 2e-5 * np.abs(g["y"]).max() + 2e-5  # int8 GEMM vs fp32 linear on the same codes


def test_quarot_linear_vs_reference_golden(golden):
    """QuarotQuantizedLinear (rotation only) at in_features 1536 against the reference's own module (fixture a4_quarot_1536):
    rotated + quantised weight (fp32 fast transform vs the reference's fp64 product: a code moves only at a .5 boundary),
    activation codes, forward output."""
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear

    g = golden("a4_quarot_1536")
    n, out = 1536, 24
    lin = torch.nn.Linear(n, out).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"]), t(g["b"])
    ql = QuarotQuantizedLinear(n, out, True, DEV, cfg(quarot={"layer_name_regex": ""}), lin)
    ql.rotation_signs = torch.from_numpy(g["signs"])
    ql.update_quantized_weight_rotated()
    np.testing.assert_allclose(ql.w_quantizer.delta.reshape(-1).cpu().numpy(), g["w_delta"], rtol=2e-6)
    dw = np.abs(ql.weight.data.cpu().numpy() - g["w_final"]) / g["w_delta"].reshape(-1, 1)
    assert dw.max() <= 1.0 + 1e-3 and (dw > 0.5).mean() < 2e-3
    q, scale, _ = ql.a_quantizer.quantize_int8(t(g["x"]).reshape(-1, n), *ql._act_transform())
    np.testing.assert_allclose(scale.cpu().numpy(), g["x_delta"], rtol=2e-6)
    d = np.abs(q.cpu().numpy().astype(np.int32) - g["x_q"].astype(np.int32))
    assert d.max() <= 1 and (d != 0).mean() < 2e-3
    y = ql(t(g["x"]))
    assert np.abs(y.cpu().numpy() - g["y"]).max() < 5e-3 * np.abs(g["y"]).max() + 1e-3


def test_dynamic_quantizer_asymmetric_branch_vs_reference_golden(golden):
    """qdiff.DynamicQuantizer with sym=False (the branch of Q/base/base_quantizer.py:130-157 no Wan configuration selects) on the
    HIP row-statistics / static-quantisation kernels: delta, zero point, codes and dequantised values bit for bit against the
    reference's own module (tests/golden/make_golden_dyn_asym.py), 8 and 4 bits; and a QuantizedLinear with asymmetric
    activations (int8 GEMM + the zero point's rank-one term) against the reference layer's output."""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import DynamicQuantizer
    from qdiff.base.quant_layer import QuantizedLinear

    g = golden("a2_dynamic_asym")
    x = t(g["x"], torch.float32)
    for bits in (8, 4):
        dq = DynamicQuantizer(qcfg.create({"n_bits": bits, "sym": False}))
        codes = dq.quantize(x)
        assert np.array_equal(dq.delta.reshape(-1).cpu().numpy(), g[f"delta{bits}"])
        assert np.array_equal(dq.zero_point.reshape(-1).cpu().numpy(), g[f"zp{bits}"])
        assert np.array_equal(codes.cpu().numpy().astype(np.int32), np.clip(g[f"q{bits}"], -128, 127))
        assert np.array_equal(dq(x).cpu().numpy(), g[f"dequant{bits}"])
    lin = torch.nn.Linear(256, 24).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"], torch.float32), t(g["b"], torch.float32)
    ql = QuantizedLinear(256, 24, True, DEV, qcfg.create({"weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": 8, "sym": False}}), lin)
    ql.w_quantizer.init_done = True
    y = ql(x.unsqueeze(0))[0].float().cpu().numpy()
    assert np.abs(y - g["y"]).max() < 2e-5 * np.abs(g["y"]).max() + 2e-5


@pytest.mark.parametrize("sym", [True, False])
def test_mixed_precision_dynamic_quantizer_vs_reference_golden(golden, sym):
    """qdiff.MixedPrecisionDynamicQuantizer (Q/base/mixed_precision_quantizer.py:126-186) on the HIP quantise kernels at every entry
    of its bit-width list [8, 6, 4], `bitwidth_refactor` between calls: codes, delta, zero point and dequantised values BIT FOR BIT
    against the reference's own class (tests/golden/make_golden_mixed_dynamic.py), including the tiny row that keeps its own delta
    (no eps floor in the symmetric branch) and the asymmetric floor 1e-6.  The all-zero row is where the reference is undefined
    (0 / 0: NaN codes): here delta 0, codes 0, output 0."""
    from qdiff import config as qcfg
    from qdiff.base.mixed_precision_quantizer import MixedPrecisionDynamicQuantizer

    g = golden("a7_mixed_dynamic")
    tag = "sym" if sym else "asym"
    x = t(g["x"], torch.float32)
    mq = MixedPrecisionDynamicQuantizer(qcfg.create({"n_bits": [8, 6, 4], "i_bitwidth": 0, "sym": sym}))
    ok = np.array([r for r in range(x.shape[0]) if not (sym and r == 5)])
    for i, bits in list(enumerate((8, 6, 4))) + [(0, 8)]:
        mq.bitwidth_refactor(i)
        assert mq.n_bits == bits
        codes = mq.quantize(x).cpu().numpy()
        delta, zp = mq.delta.reshape(-1).cpu().numpy(), mq.zero_point.reshape(-1).cpu().numpy()
        deq = mq(x).cpu().numpy()
        assert np.array_equal(delta[ok], g[f"{tag}_delta{bits}"][ok]) and np.array_equal(zp[ok], g[f"{tag}_zp{bits}"][ok])
        assert np.array_equal(codes[ok], g[f"{tag}_q{bits}"][ok])
        assert np.array_equal(deq[ok], g[f"{tag}_dequant{bits}"][ok])
        if sym:
            assert np.isnan(g[f"{tag}_q{bits}"][5]).all()                      # the reference: NaN
            assert delta[5] == 0 and not codes[5].any() and not deq[5].any()   # here: zeros
            assert 0 < delta[4] < 1e-6 and np.abs(codes[4]).max() == 2 ** (bits - 1) - 1
        else:
            assert delta[4] == np.float32(1e-6) and delta[5] == np.float32(1e-6)


@pytest.mark.parametrize("bits", [6, 4, 2])
def test_dynamic_quantizer_below_8_bits_and_quantized_linear_with_a_bitwidth_list(golden, bits):
    """Activation n_bits < 8 on the int8 path (the codes fit int8, only the range changes, the GEMM is unchanged):
    DynamicQuantizer codes / scales bit-exact against the oracle (eps floor 1e-6 kept: base_quantizer.py:122-127) for fp32 / bf16 /
    fp16 rows of several widths; and a QuantizedLinear whose activation n_bits is a list (-> MixedPrecisionDynamicQuantizer,
    quant_layer.py:48-52) against the reference layer's own output at 6 bits."""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import DynamicQuantizer
    from qdiff.base.mixed_precision_quantizer import MixedPrecisionDynamicQuantizer
    from qdiff.base.quant_layer import QuantizedLinear

    gen = torch.Generator().manual_seed(bits)
    for rows, cols, dt in [(33, 1536, torch.float32), (7, 5120, torch.bfloat16), (5, 8960, torch.float16), (9, 64, torch.float32)]:
        x = (torch.randn(rows, cols, generator=gen) * torch.exp(0.5 * torch.randn(cols, generator=gen))).to(dt)
        x[0] = 0
        x[1] *= 1e-8
        dq = DynamicQuantizer(qcfg.create({"n_bits": bits, "sym": True}))
        q, scale, ssum = dq.quantize_int8(x.to(DEV))
        oq, od = qr.dynamic_quantize_sym(x.float().numpy(), bits)
        assert np.array_equal(scale.cpu().numpy(), od) and np.array_equal(q.cpu().numpy().astype(np.int32), oq)
        assert np.abs(q.cpu().numpy()).max() == 2 ** (bits - 1) - 1 and od[0] == np.float32(1e-6)
        np.testing.assert_allclose(ssum.cpu().numpy(), oq.sum(axis=1) * od, rtol=1e-6, atol=1e-12)
        assert np.array_equal(dq(x.to(DEV)).cpu().numpy(), qr.dynamic_fake_quant_sym(x.float().numpy(), bits))
    if bits == 6:
        g = golden("a7_mixed_dynamic")
        lin = torch.nn.Linear(256, 24).to(DEV)
        lin.weight.data, lin.bias.data = t(g["w"], torch.float32), t(g["b"], torch.float32)
        conf = qcfg.create({"weight": {"n_bits": 8, "sym": False}, "act": {"n_bits": [8, 6, 4], "i_bitwidth": 1, "sym": True}})
        ql = QuantizedLinear(256, 24, True, DEV, conf, lin)
        assert isinstance(ql.a_quantizer, MixedPrecisionDynamicQuantizer) and ql.a_quantizer.n_bits == 6
        ql.w_quantizer.init_done = True
        y = ql(t(g["x"][g["lin_rows"]], torch.float32).unsqueeze(0))[0].float().cpu().numpy()
        assert np.abs(y - g["y6"]).max() < 2e-5 * np.abs(g["y6"]).max() + 2e-5


@pytest.mark.parametrize("act", [{"n_bits": 8, "sym": False}, {"n_bits": 6, "sym": True}, {"n_bits": [8, 4], "i_bitwidth": 1, "sym": False}])
def test_viditq_linear_with_asymmetric_or_narrow_activations_vs_oracle(golden, act):
    """ViDiTQuantizedLinear accepts any activation quantiser in the reference (viditq_quant_layer.py:60-73: mask, fp64 rotation, then
    `self.a_quantizer`): asymmetric (base_quantizer.py:130-149), below 8 bits, or a bit-width list.  Here the transformed row is
    written in fp32 and quantised by the plain kernels; checked against the oracle's definition evaluated in float64 on the
    reference-made layer of golden a4_viditq_1536 (same weights, mask and signs): layer output at the level of one activation step."""
    from qdiff import config as qcfg
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    g = golden("a4_viditq_1536")
    n, out = 1536, 24
    lin = torch.nn.Linear(n, out).to(DEV)
    lin.weight.data, lin.bias.data = t(g["w"]), t(g["b"])
    conf = qcfg.create({"weight": {"n_bits": 8, "sym": False}, "act": act, "viditq": {"alpha": 0.5665, "layer_name_regex": ""}})
    vl = ViDiTQuantizedLinear(n, out, True, DEV, conf, lin)
    vl.channel_mask = t(g["channel_mask"])
    vl.rotation_signs = torch.from_numpy(g["signs"])
    vl.update_quantized_weight_rotated_and_scaled()
    assert np.array_equal(vl.weight.data.cpu().numpy(), g["w_final"])
    x = g["x"].reshape(-1, n)
    y = vl(t(g["x"])).float().cpu().numpy().reshape(-1, out)
    # oracle: x' = (x * mask) @ R in float64 -> fp32, the configured quantiser, then x_dq . w_final^T + b
    R = qr.hadamard_from_signs(g["signs"])
    xt = ((x.astype(np.float64) * g["channel_mask"].astype(np.float64)) @ R).astype(np.float32)
    bits = act["n_bits"] if isinstance(act["n_bits"], int) else act["n_bits"][act["i_bitwidth"]]
    if isinstance(act["n_bits"], int):
        xdq = qr.dynamic_fake_quant_asym(xt, bits) if not act["sym"] else qr.dynamic_fake_quant_sym(xt, bits)
    else:
        xdq = qr.mixed_dynamic_fake_quant(xt, bits, act["sym"])
    want = xdq.astype(np.float64) @ g["w_final"].astype(np.float64).T + g["b"]
    step = np.abs(xt).max(axis=1).max() / (2 ** (bits - 1))   # one activation step
    assert np.abs(y - want).max() < 0.02 * step * np.abs(g["w_final"]).sum(axis=1).max() + 1e-3
    assert np.linalg.norm(y - want) / np.linalg.norm(want) < 2e-3


def test_rotate_13824_dtypes_outputs_and_viditq_layer():
    """n = 13824 = 108 x 128, the 14B ffn.2 input (csrc/rotate_paley.hip; REPO-DEFINED: the reference asserts on this width):
    bf16 / fp16 / fp32 input, fp output in every dtype, codes / scales / sums against the oracle's H_108 (x) H_128 in float64, the
    eps row; then the width as a ViDiT layer (mask, double-quantised rotated weight, forward) against the oracle."""
    import viditq_extension.fused as fused
    from qdiff.quarot import quarot_utils as qu
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    n, rows = 13824, 67
    g = torch.Generator().manual_seed(13824)
    x = (torch.randn(rows, n, generator=g) * torch.exp(0.7 * torch.randn(n, generator=g))).clamp_min(-0.17)  # GELU-like
    x[5] = 0
    pm = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    rot = qu.kernel_rotation_params(n, DEV)
    assert rot[0] == 108
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        xd = x.to(dt)
        ref = qr.matmul_hadU(xd.double().numpy() * pm.double().numpy(), strict=False)
        oq, oscale = qr.dynamic_quantize_sym(ref.astype(np.float32))
        scale, ssum = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        out = torch.empty(rows, n, device=DEV)
        q = fused.rotate_quant(xd.to(DEV), pm.to(DEV), rot, ssum, scale, out_fp=out)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=3e-6 * np.abs(ref).max())
        np.testing.assert_allclose(scale.cpu().numpy(), oscale, rtol=2e-6)
        d = np.abs(q.cpu().numpy().astype(np.int32) - oq)
        assert d.max() <= 1 and (d != 0).mean() < 2e-3
        np.testing.assert_allclose(ssum.cpu().numpy(), q.cpu().numpy().astype(np.int64).sum(1) * scale.cpu().numpy().astype(np.float64),
                                   rtol=1e-6, atol=1e-6)
        assert scale[5].item() == pytest.approx(1e-6) and int(q[5].abs().max()) == 0
    for odt in (torch.bfloat16, torch.float16):
        out = torch.empty(rows, n, dtype=odt, device=DEV)
        s16, m16 = torch.zeros(rows, dtype=torch.float16, device=DEV), torch.zeros(rows, dtype=torch.float16, device=DEV)
        fused.rotate_quant(x.to(DEV), pm.to(DEV), rot, m16, s16, out_fp=out)
        ref = qr.matmul_hadU(x.double().numpy() * pm.double().numpy(), strict=False)
        np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=2 ** -8, atol=1e-6)
    with pytest.raises(RuntimeError, match="13824"):  # no LayerNorm form at this width (no model dimension is 13824)
        fused.layernorm_rotate_quant(torch.empty(4, n, dtype=torch.int8, device=DEV), x[:4].to(DEV), None, None, None, pm.to(DEV), rot,
                                     torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), 1e-6)
    # ---- the layer
    out_f, rows = 40, 21
    w = torch.randn(out_f, n, generator=g) * 0.02 * torch.exp(0.5 * torch.randn(n, generator=g))
    b = torch.randn(out_f, generator=g) * 0.1
    x = torch.randn(rows, n, generator=g) * torch.exp(0.8 * torch.randn(n, generator=g))
    act_mask = x.abs().amax(0).clamp_min(1e-3)
    signs = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    lin = torch.nn.Linear(n, out_f).to(DEV)
    lin.weight.data, lin.bias.data = w.to(DEV), b.to(DEV)
    vl = ViDiTQuantizedLinear(n, out_f, True, DEV, cfg(viditq={"alpha": 0.5665, "layer_name_regex": ""}), lin)
    mask = qr.vidit_channel_mask(w.numpy(), act_mask.numpy(), 0.5665)
    vl.channel_mask = torch.from_numpy(mask).to(DEV)
    vl.rotation_signs = signs
    vl.update_quantized_weight_rotated_and_scaled()
    w1, _, _ = qr.static_fake_quant((w.numpy() / mask[None, :]).astype(np.float32), 8, False)
    w2in = qr.matmul_hadU(w1.astype(np.float64) * signs.numpy()[None, :], strict=False).astype(np.float32)
    w2, d2, z2 = qr.static_fake_quant(w2in, 8, False)
    np.testing.assert_allclose(vl.w_quantizer.delta.reshape(-1).cpu().numpy(), d2.reshape(-1), rtol=2e-6)
    dw = np.abs(vl.weight.data.cpu().numpy() - w2) / d2.reshape(-1, 1)
    assert dw.max() <= 1.0 + 1e-3 and (dw > 0.5).mean() < 2e-3
    xt = qr.matmul_hadU((x.numpy() * mask[None, :]).astype(np.float32).astype(np.float64) * signs.numpy()[None, :], strict=False).astype(np.float32)
    xq, xs = qr.dynamic_quantize_sym(xt)
    y_ref = (xq.astype(np.float64) * xs[:, None]) @ w2.astype(np.float64).T + b.numpy()
    y = vl(x.to(DEV))
    assert np.abs(y.cpu().numpy() - y_ref).max() < 5e-3 * np.abs(y_ref).max() + 1e-3


def test_forward_with_quant_params_vs_reference_golden(golden):
    """DynamicQuantizer.forward_with_quant_params (Q/base/base_quantizer.py:164-206: fake-quant with a precomputed delta of x's shape,
    optionally a per-element bit-width map) as one HIP launch, against what the reference's own method returned
    (tests/golden/make_golden_fwqp.py): bit for bit for fp32 inputs -- the plain 8 / 4-bit form on an attention-map-like tensor and on
    signed scores, the mixed form with bits in {0, 2, 4, 8}, delta floored in place; bf16 input within one bf16 rounding."""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import DynamicQuantizer

    g = golden("a16_forward_with_quant_params")
    for b in (8, 4):
        dq = DynamicQuantizer(qcfg.create({"n_bits": b, "sym": True}))
        d = t(g["delta"], torch.float32)
        y = dq.forward_with_quant_params(t(g["x"], torch.float32), d)
        assert np.array_equal(y.cpu().numpy(), g[f"y{b}"]) and np.array_equal(d.cpu().numpy(), g[f"delta_after{b}"])
        ys = dq.forward_with_quant_params(t(g["xs"], torch.float32), t(g["delta_s"], torch.float32))
        assert np.array_equal(ys.cpu().numpy(), g[f"ys{b}"])
    dq = DynamicQuantizer(qcfg.create({"n_bits": 8, "sym": True}))
    bits = t(g["bits"], torch.int64)
    assert np.array_equal(dq.forward_with_quant_params(t(g["x"], torch.float32), t(g["delta"], torch.float32), bits).cpu().numpy(), g["y_mixed"])
    assert np.array_equal(dq.forward_with_quant_params(t(g["xs"], torch.float32), t(g["delta_s"], torch.float32), bits).cpu().numpy(), g["ys_mixed"])
    yb = dq.forward_with_quant_params(t(g["x"], torch.bfloat16), t(g["delta"], torch.float32))
    ref = qr.fake_quant_with_delta(t(g["x"], torch.bfloat16).float().cpu().numpy(), g["delta"], 8)[0]
    assert yb.dtype == torch.bfloat16 and np.abs(yb.float().cpu().numpy() - ref).max() <= 2 ** -8 * np.abs(ref).max()
    with pytest.raises(AssertionError):
        DynamicQuantizer(qcfg.create({"n_bits": 8, "sym": False})).forward_with_quant_params(t(g["x"], torch.float32), t(g["delta"], torch.float32))
