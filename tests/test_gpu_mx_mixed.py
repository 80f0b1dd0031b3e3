"""MX Linears with outlier channels on the GPU: the mixed row quantiser (csrc/quant_mixed.hip) against the host expression bit for bit,
the two-phase GEMM (csrc/gemm_mx_mixed.hip) on exact probes, integer products and random codes, and the layers built on them.
Bound on random codes: bound_case of tests/test_gpu_fp8.py (copied below), |y - y64| <= MX_ACC (1.01 K + 3) u S + the epilogue terms, S =
sum_k |a w|, MX_ACC = 24: the constant tests/test_gpu_mx.py established for the block-scaled MFMA with e4m3 operands
(profiles/PARITY_NOTES.md "MX GEMM"); the e2m1 tiles add into an accumulator that already holds the e4m3 tiles' sum, so their own
exactness does not carry over.  Layer operands come from the quantiser and keep the plain bound (MX_ACC = 1)."""
import ctypes
import math
import os

import pytest
import torch
from qdiff.base import base_quantizer as bq
from viditq_extension import _C, fused, qgemm

pytestmark = pytest.mark.gpu
DEV = "cuda"
YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wan2.1-quantization_amd", "quant_configs", "mx",
                    "w4a4_mxfp4_o128_all_linears.yaml")
OUTS = (torch.float32, torch.bfloat16, torch.float16)
U32, MX_ACC = 2.0 ** -24, 24.0
U_OUT, TINY = {OUTS[0]: 0.0, OUTS[1]: 2.0 ** -8, OUTS[2]: 2.0 ** -11}, {OUTS[0]: 0.0, OUTS[1]: 0.0, OUTS[2]: 2.0 ** -25}
C1 = -2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e)
C3 = C1 * 0.044715
C1F, C3F = float(torch.tensor(-2.3022082, dtype=torch.float32)), float(torch.tensor(-0.10294324, dtype=torch.float32))


def gelu_ref(x):
    return x * torch.special.expit(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def gelu_bound(x):  # tests/test_gpu_gemm_probes.py::gelu_bound (profiles/PARITY_NOTES.md): gelu_tanh_fast_f32 against gelu_ref
    T = x * (C1 + C3 * x * x)
    dT = 3 * U32 * T.abs() * (1 + 2.0 ** -10) + x.abs() * abs(C1F - C1) + x.abs() ** 3 * abs(C3F - C3)
    rel = (torch.special.expit(T * math.log(2.0)) * (torch.expm1(math.log(2.0) * dT) + 2 * U32) + 4 * U32) * (1 + 2.0 ** -10)
    return gelu_ref(x).abs() * rel + 2.0 ** -125 * torch.clamp(x.abs(), min=1.0)


def bound_case(S, acc, bias, gelu, gate, res, out_dtype, K):  # (y64, tol): tests/test_gpu_fp8.py::bound_case with unit fp32 scales
    y, e = acc + bias.double(), (1.01 * K + 3) * U32 * (S + bias.double().abs())
    if gelu:
        y, e = gelu_ref(y), 1.13 * e + gelu_bound(y) * (1 + 2.0 ** -10)
    if gate is not None:
        yg = y * gate.double()
        y, e = res.double() + yg, gate.double().abs() * e + 2 * U32 * (res.double().abs() + yg.abs())
    return y, e + U_OUT[out_dtype] * y.abs() * (1 + 2.0 ** -10) + TINY[out_dtype]


def gemm(a, w, sa, sw, n8, out_dtype, bias=None, gelu=False, gate=None, residual=None):
    return qgemm.mx_mixed_linear(a, w, sa, sw, n8, bias, out_dtype, gelu, gate, None if residual is None else residual.clone())


def codes_of(v, n8):  # exactly representable values [rows, K], permuted order -> (mixed-format code bytes, unit scale bytes) on the GPU
    v = v.float().cpu()
    c8, v4, lut = v[:, :n8].to(torch.float8_e4m3fn), v[:, n8:], torch.tensor((0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0))
    mag = (v4.abs()[..., None] == lut).float().argmax(-1)
    assert torch.equal(c8.float(), v[:, :n8]) and torch.equal(lut[mag], v4.abs()), "not exact in the segment's format"
    c4 = bq.mx_pack_e2m1((mag | (torch.signbit(v4).long() << 3)).to(torch.uint8))
    return torch.cat((c8.view(torch.uint8), c4), 1).to(DEV), torch.full((v.shape[0], v.shape[1] // 32), 127, dtype=torch.uint8, device=DEV)


# (8960, 256): two block slots per lane; (16384, 128) in fp32: the one-buffer pipeline.  act = 1: the input of the host expression is
# this library's own gelu_tanh_fast_f32(x) (the GEMM epilogue on an identity weight), the tolerance class of tests/test_gpu_mx4.py
@pytest.mark.parametrize("act", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("kind", ["identity", "reversed", "random"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("cols,n8", [(256, 128), (1536, 128), (1536, 1408), (8960, 256), (16384, 128)])
def test_quantiser_matches_the_host_expression_bit_for_bit(cols, n8, dtype, kind, act):
    g = torch.Generator().manual_seed(cols + n8)
    perm = {"identity": torch.arange(cols), "reversed": torch.arange(cols - 1, -1, -1), "random": torch.randperm(cols, generator=g)}[kind].int()
    for rows in (1, 5, 130):
        x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, cols // 32), generator=g).float()).repeat_interleave(32, 1)
        x[:, ::97] *= 64                                                 # outliers that own their block's scale
        x = x.to(torch.bfloat16 if act and dtype == torch.float32 else dtype).to(DEV)
        x[x == 0] = 1                                                    # (the GEMM that makes the act = 1 reference turns a -0 into +0)
        ref = x if not act else qgemm.fp_linear(x.view(-1, 64), torch.eye(64, dtype=x.dtype, device=DEV), None, torch.float32, gelu=True)
        want, s = bq.mx_quant_rows_mixed_host(ref.float().view(rows, cols).cpu(), perm, n8)
        codes, scale = fused.quant_rows_mx_mixed(x.to(dtype), perm.to(DEV), n8, gelu=act)
        assert tuple(codes.shape) == (rows, n8 + (cols - n8) // 2) and torch.equal(scale.cpu(), s) and torch.equal(codes.cpu(), want), rows


@pytest.mark.parametrize("K,n8", [(256, 128), (512, 384)])
def test_address_probe_one_token_element_against_one_weight_element(K, n8):
    """all codes zero but token (m, k) = 1.5 and weight (n, k) = -2 at ONE permuted position k, scale bytes 127 but 128 (token) and 125
    (weight) on k's block: the output is 1.5 * -2 * 2 * 2^-2 = -1.5 at (m, n) and zero elsewhere, exactly.  k on both sides of the
    segment boundary, of a block, of a K-tile: the segment offset, the nibble order and the scale-tile index."""
    M, N = 130, 136
    for i, k in enumerate((0, 127, n8 - 1, n8, n8 + 31, n8 + 127, K - 1)):
        m, n = (5, 129, 64)[i % 3], (135, 3, 70)[i % 3]
        av, wv, want = torch.zeros(M, K), torch.zeros(N, K), torch.zeros(M, N, device=DEV)
        av[m, k], wv[n, k], want[m, n] = 1.5, -2.0, -1.5
        (a, sa), (w, sw) = codes_of(av, n8), codes_of(wv, n8)
        sa[m, k // 32], sw[n, k // 32] = 128, 125
        out = gemm(a, w, sa, sw, n8, torch.float32)
        assert torch.equal(out, want), (k, out[m, n].item(), out.nonzero().tolist()[:4])


@pytest.mark.parametrize("M,N,K,n8", [(M, N, K, n8) for M in (1, 129) for N in (8, 136) for K, n8 in ((256, 128), (640, 256))])
def test_integer_operands_equal_the_float64_product_in_every_output_type(M, N, K, n8):
    g = torch.Generator().manual_seed(M + N + K)
    av, wv = torch.randint(-4, 5, (M, K), generator=g).float(), torch.randint(-4, 5, (N, K), generator=g).float()
    acc = (av.double() @ wv.double().T).to(DEV)                           # |acc| <= 16 K: exact in fp32 in any order
    (a, sa), (w, sw) = codes_of(av, n8), codes_of(wv, n8)
    for out_dtype in OUTS:
        assert torch.equal(gemm(a, w, sa, sw, n8, out_dtype), acc.to(out_dtype)), out_dtype


def random_side(rows, K, n8, lo8, lo4, gen):  # random codes (the e4m3 NaN codes replaced by 0), random scale bytes, their float64 decode
    c = torch.randint(0, 256, (rows, n8 + (K - n8) // 2), device=DEV, generator=gen, dtype=torch.uint8)
    c[:, :n8][(c[:, :n8] & 0x7f) == 0x7f] = 0
    s = torch.cat((torch.randint(lo8, lo8 + 7, (rows, n8 // 32), device=DEV, generator=gen, dtype=torch.uint8),
                   torch.randint(lo4, lo4 + 7, (rows, (K - n8) // 32), device=DEV, generator=gen, dtype=torch.uint8)), dim=1)
    return c, s, bq.mx_decode_mixed(c, s, n8, torch.float64)


@pytest.mark.parametrize("M,N,K,n8", [(M, N, K, n8) for M in (1, 127, 257) for N in (8, 264) for K, n8 in ((256, 128), (1536, 256))])
def test_random_codes_and_scale_bytes_within_the_derived_bound_and_bit_equal_across_launches(M, N, K, n8):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    (a, sa, a64), (w, sw, w64) = random_side(M, K, n8, 112, 117, g), random_side(N, K, n8, 111, 116, g)
    acc, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    assert float(S.max()) < 3e4                                           # every output inside fp16
    bias, gate = torch.randn(N, device=DEV, generator=g) * 0.1, torch.rand(N, device=DEV, generator=g) * 2 - 1
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = gemm(a, w, sa, sw, n8, out_dtype, bias, gelu, gate if gres else None, res if gres else None)
            y, tol = bound_case(MX_ACC * S, acc, bias, gelu, gate if gres else None, res, out_dtype, K)
            worst[(str(out_dtype)[6:], gelu, gres)] = round(((out.double() - y).abs() / tol).max().item(), 4)
    print(f"mixed MX GEMM ({M}, {N}, {K}, n8 {n8}): worst err / bound {max(worst.values()):.4f} {worst}")
    assert max(worst.values()) <= 1.0, worst
    m = M // 2                                                            # the same bits again, and for a row in a launch of another M
    assert torch.equal(out, gemm(a, w, sa, sw, n8, out_dtype, bias, True, gate, res))
    assert torch.equal(out[m:m + 1], gemm(a[m:m + 1].contiguous(), w, sa[m:m + 1].contiguous(), sw, n8, out_dtype, bias, True, gate, res[m:m + 1]))


def test_refusals_carry_the_entrys_text_and_zero_rows_are_ok():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)  # noqa: E731
    st, p = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), z(16).data_ptr()
    assert _C.lib.wanq_gemm_mx_mixed(p, p, p, p, 128, p, 1, None, 2, None, None, 0, 0, 8, 256, st) == 0            # M == 0
    assert _C.lib.wanq_quant_rows_mx_mixed(p, 1, p, 128, p, p, 0, 256, 0, st) == 0                                 # rows == 0
    assert _C.lib.wanq_gemm_mx_mixed(p, p, p, p, 256, p, 1, None, 2, None, None, 0, 4, 8, 256, st) == 2
    assert b"wanq_gemm_mx_mixed: n8=256 must be a multiple of 128 with 128 <= n8 <= K - 128" in _C.lib.wanq_last_error()
    assert _C.lib.wanq_quant_rows_mx_mixed(p, 1, None, 128, p, p, 4, 256, 0, st) == 1
    assert b"wanq_quant_rows_mx_mixed: perm must be non-NULL" in _C.lib.wanq_last_error()
    with pytest.raises(RuntimeError, match=r"mx_mixed_linear: n8=256 must be a multiple of 128 with 128 <= n8 <= K - 128"):
        qgemm.mx_mixed_linear(z(4, 256), z(8, 256), z(4, 8), z(8, 8), 256)
    with pytest.raises(RuntimeError, match=r"quant_rows_mx_mixed: n8=256 must be a multiple of 128"):
        fused.quant_rows_mx_mixed(torch.zeros(4, 256, device=DEV), torch.arange(256, device=DEV, dtype=torch.int32), 256)


def _tiny_model():  # tests/test_gpu_fp8.py::_tiny_model (one block) under the o128 config; channel orders from seeded statistics, one vector per width
    from qdiff import config as qcfg
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 1, 20, 26)   # 130 tokens
    args = ([torch.randn(shape, device=DEV, generator=g)], torch.tensor([700], device=DEV), [torch.randn(24, 64, device=DEV, generator=g) * 0.1],
            seq_len_for(shape))
    model = QuantWanModel.from_float(fp, qcfg.load(YAML))
    model.quant_layer_refactor()
    stat = {K: torch.rand(K, device=DEV, generator=g) for K in (256, 512)}
    for mod in model.modules():
        if getattr(mod, "mx_n8", None) is not None:
            mod.get_channel_mask(stat[mod.in_features])
    model.set_init_done()
    return model, fp, (lambda m: m(*args)[0].float().clone())


def test_toy_model_both_modes_layer_bound_shared_quantiser_launch_and_checkpoint_round_trip(tmp_path, monkeypatch):
    from wan import quant_wanx_hip as H
    model, fp, run = _tiny_model()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref_fp = run(fp)
    sim = run(model)
    model.hardware_forward_refactor()
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, H.HipLinearMx)]
    assert len(lins) == 10 and all(m.n8 == 128 and m.act_form == "mxmix128" and m.mx_perm.dtype == torch.int32 for m in lins)
    # one layer, kernel mode against simulation mode: each within the plain bound of the float64 product of the decoded operands
    hl, ql, K = model.hip_blocks[0].ffn2, model.blocks[0].ffn[2], 512
    x = torch.randn(130, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(torch.bfloat16)
    a_q, a_s = hl.operands(H._FpSrc(x))
    a64, w64 = (bq.mx_decode_mixed(c, s, 128, torch.float64) for c, s in ((a_q, a_s), (hl.weight, hl.scale_weight)))
    y64 = a64 @ w64.T + hl.bias.double()
    tol = (1.01 * K + 3) * U32 * (a64.abs() @ w64.abs().T + hl.bias.double().abs()) + 2.0 ** -8 * y64.abs() * (1 + 2.0 ** -10)
    for what, y in (("kernel", hl(a_q, a_s, torch.bfloat16)), ("simulation", ql(x))):
        assert y.dtype == torch.bfloat16 and not ((y.double() - y64).abs() > tol).any(), what
    # the whole block; q, k and v read ONE quantised copy of their source: its cache holds the form once, made by one launch
    srcs, calls, init, quant = [], [], H._LnSrc.__init__, fused.quant_rows_mx_mixed
    monkeypatch.setattr(H._LnSrc, "__init__", lambda self, *a, **k: (init(self, *a, **k), srcs.append(self))[0])
    monkeypatch.setattr(fused, "quant_rows_mx_mixed", lambda x, *a, **k: (calls.append(x.data_ptr()), quant(x, *a, **k))[1])
    hw = run(model)
    assert "mxmix128" in srcs[0].cache and calls.count(srcs[0].cache["fp32"].data_ptr()) == 1 and len(calls) < len(lins)
    err, noise = float((hw - sim).norm() / sim.norm()), float((sim - ref_fp).norm() / ref_fp.norm())
    print(f"o128 block, kernel mode vs simulation mode: rel err {err:.3e}; simulation mode vs the floating-point model {noise:.3e}")
    assert torch.isfinite(hw).all() and noise > 0 and err < 1e-2 and err < 0.5 * noise + 5e-3   # the margin of tests/test_gpu_fp8.py
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.2.mx_perm"].dtype == torch.int32 and sd["blocks.0.ffn.2.mx_n8"].tolist() == [128]
    fresh = _tiny_model()[0]
    fresh.hardware_forward_refactor(load_path=path)
    assert torch.equal(run(fresh), hw)
