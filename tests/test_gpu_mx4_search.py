"""The e2m1 row quantiser under the block-scale rule `search` on the GPU (csrc/rowwise.hip: wanq_quant_rows_mx4_search /
fused.quant_rows_mx4_search; the rule: csrc/mx_block.h, include/wanq_hip.h) and the layers built on it from
quant_configs/mx/w4a4_mxfp4_search_all_linears.yaml and w4a4_mxfp4_had32_search_all_linears.yaml.

1. bit-equality with the host expression mx_quant_rows_host(search=True) on every rung of the row ladder;
2. against a float64 reference that shares nothing with it (tests/test_mx4_search_abi.py::check_against_float64, which that file holds
   the host expression to on the same rows);
3. exact probes in scaled units at a fixed s0;
4. one kernel-mode Linear per shipped config against simulation mode in host memory, under the plain bound of K - 1 fp32 additions
   (tests/test_gpu_mx4.py), and which consumers of one source share a quantisation.
The largest scale byte: for emax = 2 OCP's byte is at most 253 (an infinite maximum) and 252 for a finite one, so "s0 = 254" cannot be
built and the `s0 < 254` guard of the kernel and the host expression can never fire; the probe row holds the largest finite block instead, which is searched like any other and takes 253."""
import pytest
import torch

from test_gpu_fp8 import bound_case, gen_for, ones
from test_gpu_mx import deq64
from test_gpu_mx4 import _sim_layer
from test_gpu_rowwise_probes import FORMS, form_of
from test_gpu_wq16 import DEV
from test_mx4_search_abi import YAML44S, YAML44HS, check_against_float64, search_rows

pytestmark = pytest.mark.gpu
FP4 = "mxfp4_e2m1"
# every rung of row_ladder: one block, two ragged row counts on the rungs they reach, the smallest width of each other rung (its last
# chunk slot ragged), and the ladder's widest width; 5 rows leave a ragged workgroup in the wave-per-row forms
SHAPES = [(1, 32), (5, 128), (200, 1536)]
SHAPES += [(5 if wpr == 1 else 3, 16384 if hi == FORMS[-1][0] else lo * 8 + 32) for (lo, _, _), (hi, wpr, nch) in zip(FORMS, FORMS[1:])
           if (wpr, nch) not in [form_of(c) for _, c in SHAPES]]


def library_gelu(x16):
    """gelu_tanh_fast_f32 of a 16-bit tensor as the library computes it (the GEMM epilogue on an identity), fp32"""
    from viditq_extension import qgemm

    flat = torch.zeros((x16.numel() + 63) // 64 * 64, dtype=x16.dtype, device=DEV)
    flat[:x16.numel()] = x16.reshape(-1)
    eye = torch.eye(64, dtype=x16.dtype, device=DEV)
    return qgemm.fp_linear(flat.view(-1, 64), eye, None, torch.float32, gelu=True).reshape(-1)[:x16.numel()].view(x16.shape)


@pytest.mark.parametrize("had32", [False, True], ids=["plain", "had32"])
@pytest.mark.parametrize("gelu", [False, True], ids=["id", "gelu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_codes_and_scale_bytes_equal_the_host_expression(dtype, gelu, had32):
    """every rung of the ladder; rows with a scale of their own, one large element in every third block, a zero block.  With the GELU
    the host expression is applied to the library's own GELU (held fixed: tests/test_gpu_mx4.py), of 16-bit values in every dtype"""
    from qdiff.base.base_quantizer import mx_quant_rows_host
    from viditq_extension import fused

    assert {form_of(c) for _, c in SHAPES} == {(w, n) for _, w, n in FORMS} and len(SHAPES) == len(FORMS) + 1
    taken = 0
    for rows, cols in SHAPES:
        g = torch.Generator().manual_seed(rows + cols)
        x = torch.randn(rows, cols, generator=g) * 2.0 ** torch.randint(-8, 9, (rows, 1), generator=g).float()
        xb = x.view(rows, cols // 32, 32)
        xb[:, ::3, 5] *= 9.0
        xb[rows // 2, (cols // 32) // 2] = 0.0
        x = x.to(torch.bfloat16 if gelu and dtype == torch.float32 else dtype).to(dtype).to(DEV)
        ref = library_gelu(x.to(torch.bfloat16) if dtype == torch.float32 else x) if gelu else x.float()
        want, s = mx_quant_rows_host(ref.cpu(), FP4, had32=had32, search=True)
        codes, scale = fused.quant_rows_mx4_search(x, gelu=gelu, had32=had32)
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (rows, cols // 2) and tuple(scale.shape) == (rows, cols // 32)
        assert torch.equal(scale.cpu(), s), ((rows, cols), (scale.cpu() != s).nonzero()[:8].tolist())
        assert torch.equal(codes.cpu(), want), ((rows, cols), (codes.cpu() != want).nonzero()[:8].tolist())
        taken += int((scale != fused.quant_rows_mx(x, FP4, gelu, had32)[1]).sum())
    assert taken > 0      # (the rule is not a no-op)


@pytest.mark.parametrize("kind", ["gauss", "outlier"])
@pytest.mark.parametrize("had32", [False, True], ids=["plain", "had32"])
def test_chosen_byte_is_the_float64_argmin_and_never_worse_than_ocp(had32, kind):
    from viditq_extension import fused

    x = search_rows(kind)
    codes, scale = fused.quant_rows_mx4_search(x.to(DEV), had32=had32)
    check_against_float64(x, codes.cpu(), scale.cpu(), had32, kind)


def test_exact_probes_in_scaled_units():
    """s0 = 129 (x = 4 t).  7.75 alone: e(s0) = 1.75^2, e(s0 + 1) = (4 - 3.875)^2 -> s0 + 1, code 4.0.  4.0 over 0.5s: exact -> s0.
    7.0 alone: clipped to 6, e(s0) = 1; 3.5 ties up to 4, 4 e(s0 + 1) = 4 x 0.25 = 1: a tie -> s0.  A zero block.  The largest finite
    fp32: s0 = 252, just under 8 clips -> 253.  An Inf block and a NaN block: what wanq_quant_rows_mx writes."""
    from viditq_extension import fused

    blk = torch.zeros(7, 32)
    blk[0, 9] = 7.75 * 4
    blk[1] = 0.5 * 4
    blk[1, 31] = -4.0 * 4
    blk[2, 17] = 7.0 * 4
    blk[4, 2] = torch.finfo(torch.float32).max
    blk[5, :8], blk[5, 8] = 3.0, float("inf")
    blk[6, :8], blk[6, 30] = 3.0, float("nan")
    x = blk.reshape(1, -1).to(DEV)
    codes, scale = fused.quant_rows_mx4_search(x)
    ocp_c, ocp_s = fused.quant_rows_mx(x, FP4)
    assert scale[0].tolist()[:5] == [130, 129, 129, 0, 253] and ocp_s[0].tolist()[:5] == [129, 129, 129, 0, 252]
    d = deq64(codes, scale, FP4)[0].view(7, 32).cpu()
    assert d[0, 9].item() == 32.0 and d[0].count_nonzero().item() == 1                 # code 4.0 under s0 + 1
    assert torch.equal(d[1], blk[1].double())                                            # exact under s0
    assert d[2, 17].item() == 24.0                                                       # the tie keeps s0: 7 clips to 6
    assert not bool(d[3].any()) and not bool(codes[0, 48:64].any())
    assert d[4, 2].item() == 2.0 ** 128                                                  # 4.0 x 2^(253 - 127): nothing clips
    assert torch.equal(scale[0, 5:], ocp_s[0, 5:]) and torch.equal(codes[0, 80:], ocp_c[0, 80:])


@pytest.mark.parametrize("path,had", [(YAML44S, False), (YAML44HS, True)], ids=["plain", "had32"])
def test_kernel_mode_linear_matches_simulation_mode_in_host_memory(path, had):
    """rows 200, K 256, N 128: the kernel-mode layer's operands are the host expression's bit for bit, and its output stays within the
    plain bound around the float64 product of the decoded operands, which is what simulation mode computes in host memory.  q / k / v
    of one source share one quantisation; a `floor` layer on the same source gets its own."""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import mx_quant_rows_host
    from qdiff.base.quant_layer import QuantizedLinear
    from wan.quant_wanx_hip import HipLinearMx, _FpSrc

    M, K, N = 200, 256, 128
    ql, gen = _sim_layer(path, K, N, "blocks.0.self_attn.q")
    fp = torch.nn.Linear(K, N)
    fp.load_state_dict({k: v.cpu() for k, v in ql.fp_module.state_dict().items()})
    host = QuantizedLinear(K, N, True, "cpu", qcfg.load(path), fp, module_name="blocks.0.self_attn.q")
    assert torch.equal(host._codes, ql._codes.cpu()) and torch.equal(host.w_quantizer.scale_u8, ql.w_quantizer.scale_u8.cpu())
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    x[:, 9] *= 20
    q, k, v = (HipLinearMx.from_quantized(ql, f"blocks.0.self_attn.{n}") for n in "qkv")
    assert q.act_form == ("mxfp4_h32_s" if had else "mxfp4_s") and q._gemm == "mx4_linear"
    src = _FpSrc(x.to(DEV))
    a_q, a_s = q.operands(src)
    assert k.operands(src)[0] is a_q and v.operands(src)[0] is a_q
    hq, hs = mx_quant_rows_host(x.float(), FP4, had32=had, search=True)
    assert torch.equal(a_q.cpu(), hq) and torch.equal(a_s.cpu(), hs)
    floor = HipLinearMx(K, N, True, FP4, "floor", FP4, had).to(DEV)
    f_q, f_s = floor.operands(src)
    assert f_q is not a_q and not torch.equal(f_s, a_s) and q.operands(src)[0] is a_q
    out = q(a_q, a_s, torch.bfloat16)
    sim = host(x.unsqueeze(0))[0]
    a64, w64 = deq64(a_q, a_s, FP4), deq64(q.weight, q.scale_weight, FP4)
    y, tol = bound_case(a64.abs() @ w64.abs().T, a64 @ w64.T, ones(M), ones(N), q.bias, False, None, None, torch.bfloat16, K)
    assert not ((out.double() - y).abs() > tol).any() and not ((sim.to(DEV).double() - y).abs() > tol).any()
