"""The fp8 (OCP e4m3fn) W8A8 Linears on the GPU: the row-wise quantiser (csrc/rowwise.hip, wanq_quant_rows_fp8 / fused.quant_rows_fp8),
the GEMM (csrc/gemm_fp8.hip, wanq_gemm_fp8 / qgemm.fp8_linear) and what is built on them: simulation mode of a QuantizedLinear with
`format: fp8_e4m3`, kernel mode's HipLinearFp8, the integer checkpoint and the entry points, with quant_configs/w8a8_fp8_all_linears.yaml.

Contract (include/wanq_hip.h):
    scale_r = max(absmax_r / 448, 1e-6);  q = e4m3fn_rne(clamp(x / scale_r, -448, 448))            (true division, one rounding)
    acc = sum_k a[m,k] w[n,k] (fp32);  y = fma(acc * sa[m], sw[n], bias[n]);  GELU;  residual + y * gate;  one rounding.
The quantiser is compared bit for bit with the torch expression evaluated in host memory (this torch build casts fp32 -> float8_e4m3fn
on the CPU to nearest even and keeps subnormals: tests/test_fp8_abi.py).  GEMM probes use integer operands (exact in e4m3 up to 16) and
power-of-two scales, so every partial sum is exact in fp32 in any order and the output must EQUAL the float64 evaluation.

Bound on random data (profiles/PARITY_NOTES.md, "fp8 GEMM"), u = 2^-24, S = sum_k |a w|, T = sa[m] sw[n] S + |bias[n]|:
    |y - y64| <= (1.01 K + 3) u T        K - 1 fp32 additions of exact products in any order (gamma_K <= 1.01 K u), acc * sa, the fma
through GELU:  1.13 e + gelu_bound (tests/test_gpu_gemm_probes.py);  through gate + residual:  |gate| e + 2 u (|residual| + |y gate|);
the store:  + u_out |out|, u_out = 2^-8 (bf16), 2^-11 (fp16), 0 (fp32); fp16 below 2^-14 is spaced 2^-24 apart: + 2^-25."""
import ctypes
import logging
import os

import pytest
import torch

from test_gpu_gemm_probes import gelu_bound, gelu_ref
from test_gpu_wq16 import DEV, DT, EPI_GATE_RES, EPI_GELU, PKG, Window

pytestmark = pytest.mark.gpu
YAML = os.path.join(PKG, "quant_configs", "w8a8_fp8_all_linears.yaml")
U32 = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
OUTS = (torch.float32, torch.bfloat16, torch.float16)
KSTEP = 64


# ---- references, in host memory ------------------------------------------------------------------------------------------------
def cpu_quant(x32):
    """(codes uint8, scale fp32 [rows]) of the torch expression on an fp32 CPU tensor"""
    am = x32.abs().amax(dim=-1, keepdim=True)
    s = (am / torch.full_like(am, 448.0)).clamp_min(1e-6)
    return (x32 / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), s.reshape(-1)


def decode(codes):
    return codes.cpu().view(torch.float8_e4m3fn).double()


def e4m3(t):
    """exactly representable values -> their codes, on the GPU"""
    c = t.detach().float().cpu().to(torch.float8_e4m3fn)
    assert torch.equal(c.float(), t.detach().float().cpu()), "not exact in e4m3"
    return c.view(torch.uint8).to(DEV).contiguous()


def gen_for(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---- 1. the quantiser, bit for bit ------------------------------------------------------------------------------------------------
def test_code_table_every_code_its_midpoints_and_their_neighbours():
    """one row: every finite code's value, the midpoint to the next code of its sign (ties to even; the subnormal range included) and
    the fp32 neighbours of that midpoint, with +-448 in the row: scale = 1 exactly, the codes are the conversion's alone"""
    from viditq_extension import fused

    allc = torch.arange(256, dtype=torch.uint8)
    val = allc.view(torch.float8_e4m3fn).float()
    vals = [torch.tensor([448.0, -448.0])]
    for c in range(256):
        if c & 0x7f == 0x7f:
            continue  # NaN
        v = val[c:c + 1]
        vals.append(v)
        if (c + 1) & 0x7f != 0x7f:
            mid = (v.double() + val[c + 1].double()) / 2
            assert torch.equal(mid.float().double(), mid)
            mid = mid.float()   # never 0: next to +-0 it is +-2^-10
            vals += [mid, torch.nextafter(mid, torch.zeros(1)), torch.nextafter(mid, mid * 2)]
    row = torch.cat(vals)
    row = torch.cat([row, torch.zeros(-len(row) % 8)])[None, :].contiguous()
    want, s = cpu_quant(row)
    assert s.tolist() == [1.0]
    assert len(set(want.view(-1).tolist())) == 254  # every finite code is asked for
    codes, scale = fused.quant_rows_fp8(row.to(DEV))
    assert scale.tolist() == [1.0]
    bad = (codes.cpu() != want).nonzero()
    assert bad.numel() == 0, [(row[0, j].item(), hex(codes[0, j].item()), hex(want[0, j].item())) for _, j in bad[:8].tolist()]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [8, 1536, 2056, 8960])
def test_random_rows_match_the_torch_expression_bit_for_bit(cols, dtype):
    """widths in both branch classes of the ladder (one wave per row: 8, 1536; four: 2056, 8960), a ragged last chunk slot (2056, 8960),
    rows of very different size, an outlier column, a row of zeros and a row below the scale floor; two workgroups of the wave-per-row
    form"""
    from viditq_extension import fused

    rows = 7
    g = torch.Generator().manual_seed(cols + 3)
    x = torch.randn(rows, cols, generator=g) * (10.0 ** torch.arange(-4, 3).float())[:, None]
    x[:, cols // 3] *= 25.0
    x[2] = 0
    x[4] = torch.randn(cols, generator=g) * 1e-7
    x = x.to(dtype)
    want, s = cpu_quant(x.float())
    codes, scale = fused.quant_rows_fp8(x.to(DEV))
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (rows, cols) and scale.dtype == torch.float32
    assert torch.equal(scale.cpu(), s)
    assert s[2] == torch.tensor(1e-6) and s[4] == torch.tensor(1e-6)
    assert not bool(codes[2].any()) and torch.equal(codes.cpu(), want)


def test_zero_rows_get_the_floor_scale_and_zero_codes():
    from viditq_extension import fused

    codes, scale = fused.quant_rows_fp8(torch.zeros(5, 2056, device=DEV))
    assert not bool(codes.any()) and torch.equal(scale.cpu(), torch.full((5,), 1e-6))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [64, 1536, 2112, 8960])
def test_gelu_form_quantises_this_librarys_own_gelu(cols, dtype):
    """act = 1 against the torch expression applied to gelu_tanh_fast_f32(x) as the library itself computes it: the fp32 output of the
    16-bit GEMM's GELU epilogue on x times the identity (exact pre-activation), 64 columns at a time -- the comparison holds the GELU
    fixed and tests what is new, the quantiser behind it"""
    from viditq_extension import fused, qgemm

    rows = 6
    g = torch.Generator().manual_seed(cols)
    x16 = (torch.randn(rows, cols, generator=g) * 3).to(torch.bfloat16 if dtype == torch.float32 else dtype).to(DEV)
    eye = torch.eye(64, dtype=x16.dtype, device=DEV)
    gel = qgemm.fp_linear(x16.view(-1, 64).contiguous(), eye, None, torch.float32, gelu=True).view(rows, cols)
    want, s = cpu_quant(gel.cpu())
    codes, scale = fused.quant_rows_fp8(x16.to(dtype), gelu=True)
    assert torch.equal(scale.cpu(), s) and torch.equal(codes.cpu(), want)


# ---- 2. the GEMM ----------------------------------------------------------------------------------------------------------------
def call_abi(a, w, sa, sw, out_dtype, bias=None, gelu=False, gate=None, residual=None, inplace=False):
    """wanq_gemm_fp8 through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape
    N = w.shape[0]
    win = Window(M, N, out_dtype)
    if residual is not None and inplace:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_fp8(a.data_ptr(), w.data_ptr(), sa.data_ptr(), sw.data_ptr(), win.out.data_ptr(), DT[out_dtype],
                              None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
                              None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


def ones(n):
    return torch.ones(n, device=DEV)


PROBE_ROWS = (0, 15, 16, 31, 32, 47, 48, 63, 64, 127, 128, 129)


def test_operand_map_probe_one_nonzero_activation_against_asymmetric_weights():
    """a = 2 at one (m, k), w[n, k] = 1 + (3 n + 5 k) % 13: the output is 2 w[:, k] in row m and 0 elsewhere, exactly.  Every k of a
    K-tile = of one 128-deep MFMA (both 16-byte fragment reads of a lane, every byte of them), rows in all four 16-row blocks of a wave and on both sides of the
    128-row tile edge; 136 channels: all four 16-channel blocks, both waves, both sides of the 128-channel tile edge"""
    M, N, K = 130, 136, 128
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    wv = (1 + (3 * n + 5 * k) % 13).float()
    w = e4m3(wv)
    two = e4m3(torch.tensor([2.0]))
    for k0 in range(K):
        m0 = PROBE_ROWS[k0 % len(PROBE_ROWS)]
        a = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
        a[m0, k0] = two[0]
        out = call_abi(a, w, ones(M), ones(N), torch.float32)
        expect = torch.zeros(M, N)
        expect[m0] = 2 * wv[:, k0]
        assert torch.equal(out.cpu(), expect), (m0, k0)


def test_operand_map_probe_every_row_and_k_in_one_launch():
    """one nonzero per row, a[m, (37 m + 5) % K] = 1 + m % 3, over three K-tiles with a ragged last one (K = 320)"""
    M, N, K = 260, 136, 320
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    wv = (1 + (3 * n + 5 * k) % 13).float()
    k_of = (torch.arange(M) * 37 + 5) % K
    av = torch.zeros(M, K)
    av[torch.arange(M), k_of] = (1 + torch.arange(M) % 3).float()
    out = call_abi(e4m3(av), e4m3(wv), ones(M), ones(N), torch.float32)
    assert torch.equal(out.cpu(), wv[:, k_of].T * (1 + torch.arange(M) % 3).float()[:, None])


def int_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, K), generator=g).float(), torch.randint(-8, 9, (N, K), generator=g).float()


@pytest.mark.parametrize("K", [KSTEP, 2 * KSTEP, 3 * KSTEP, 5 * KSTEP])
def test_integer_operands_equal_the_int64_product(K):
    """integers in [-8, 8]: |partial sums| <= 64 K < 2^24, exact in any order.  K = one step, one full K-tile, a tile and a ragged half
    tile (3 steps), two tiles and a half"""
    M, N = 130, 136
    av, wv = int_operands(M, N, K, K)
    out = call_abi(e4m3(av), e4m3(wv), ones(M), ones(N), torch.float32)
    assert torch.equal(out.cpu().long(), av.long() @ wv.long().T)


@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_scales_bias_gate_and_residual_exactly_in_every_output_type(out_dtype):
    """sa, sw, |gate| in {1/2, 1, 2}, integer bias (fp32, fp16 and bf16 vectors) and residual: every step is exact in fp32 (multiples of
    2^-3 below 2^18), so the output is the float64 value rounded once into the output type; out of place and in place"""
    M, N, K = 130, 136, 192
    av, wv = int_operands(M, N, K, 7)
    a, w = e4m3(av), e4m3(wv)
    g = gen_for(11)
    sa = 2.0 ** torch.randint(-1, 2, (M,), device=DEV, generator=g).float()
    sw = 2.0 ** torch.randint(-1, 2, (N,), device=DEV, generator=g).float()
    bias = torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
    gate = (2.0 ** torch.randint(-1, 2, (N,), device=DEV, generator=g).float()) * (torch.randint(0, 2, (N,), device=DEV, generator=g) * 2 - 1)
    res = torch.randint(-16, 17, (M, N), device=DEV, generator=g).to(out_dtype)
    acc = (av.double() @ wv.double().T).to(DEV)
    y64 = acc * sa.double()[:, None] * sw.double()[None, :]
    for b in (None, bias, bias.half(), bias.bfloat16()):
        y = y64 + (0.0 if b is None else b.double())
        assert torch.equal(y.float().double(), y)
        assert torch.equal(call_abi(a, w, sa, sw, out_dtype, b), y.float().to(out_dtype))
        yr = res.double() + y * gate.double()
        assert torch.equal(yr.float().double(), yr)
        for inplace in (False, True):
            r = res.clone()
            out = call_abi(a, w, sa, sw, out_dtype, b, False, gate, r, inplace)
            assert torch.equal(out, yr.float().to(out_dtype)), (b is None, inplace)
            assert torch.equal(r, res)


def bound_case(S, acc, sa, sw, bias, gelu, gate, res, out_dtype, K):
    """(y64, tol) of the module docstring's bound; S = sum_k |a w|, acc = sum_k a w, float64 [M, N]"""
    sasw = sa.double()[:, None] * sw.double()[None, :]
    b = 0.0 if bias is None else bias.double()
    T = sasw * S + (0.0 if bias is None else bias.double().abs())
    y = acc * sasw + b
    e = (1.01 * K + 3) * U32 * T
    if gelu:
        e = 1.13 * e + gelu_bound(y) * (1 + 2.0 ** -10)
        y = gelu_ref(y)
    if gate is not None:
        yg = y * gate.double()
        y = res.double() + yg
        e = gate.double().abs() * e + 2 * U32 * (res.double().abs() + yg.abs())
    return y, e + U_OUT[out_dtype] * y.abs() * (1 + 2.0 ** -10) + TINY[out_dtype]


@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_gelu_epilogue_on_exact_pre_activations(out_dtype):
    """the pre-activation is exact (integers, power-of-two scales), so the error is the GELU's alone: gelu_bound, then gate + residual
    and the store"""
    M, N, K = 130, 136, 128
    av, wv = int_operands(M, N, K, 5)
    av, wv = av * (torch.rand(M, K) < 0.1), wv.clamp(-2, 2)   # pre-activations of a few units
    g = gen_for(13)
    sa = 2.0 ** torch.randint(-2, 0, (M,), device=DEV, generator=g).float()
    sw = 2.0 ** torch.randint(-2, 1, (N,), device=DEV, generator=g).float()
    bias = torch.randint(-2, 3, (N,), device=DEV, generator=g).float() / 4
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
    acc = (av.double() @ wv.double().T).to(DEV)
    zero = torch.zeros_like(acc)
    for gres in (False, True):
        out = call_abi(e4m3(av), e4m3(wv), sa, sw, out_dtype, bias, True, gate if gres else None, res.clone() if gres else None)
        y, tol = bound_case(zero, acc, sa, sw, bias, True, gate if gres else None, res, out_dtype, 0)
        err = (out.double() - y).abs()
        assert not (err > tol).any(), (gres, (err / tol).max().item())


def random_codes(rows, cols, gen, spread):
    """e4m3 codes of a quantised random matrix (what the quantiser writes: the full range up to 448 in every row), their scales"""
    from viditq_extension import fused

    x = torch.randn(rows, cols, device=DEV, generator=gen) * spread
    return fused.quant_rows_fp8(x)


@pytest.mark.parametrize("M,N,K", [(130, 136, 192), (300, 264, 1536), (257, 128, 8960)])
def test_random_e4m3_operands_and_epilogues_within_the_derived_bound(M, N, K):
    g = gen_for(M + N + K)
    a, sa = random_codes(M, K, g, 1.0)
    w, sw = random_codes(N, K, g, K ** -0.5)
    a64, w64 = decode(a).to(DEV), decode(w).to(DEV)
    acc, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(a, w, sa, sw, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None, inplace=gres)
            y, tol = bound_case(S, acc, sa, sw, bias, gelu, gate if gres else None, res, out_dtype, K)
            err = (out.double() - y).abs()
            worst[(str(out_dtype)[6:], gelu, gres)] = round((err / tol).max().item(), 4)
            assert not (err > tol).any(), (out_dtype, gelu, gres, int((err > tol).sum()), (err / tol).max().item())
    print(f"fp8 GEMM ({M}, {N}, {K}): worst err / bound {max(worst.values()):.4f} {worst}")


def test_repeated_calls_and_rows_in_launches_of_another_size_are_bit_equal():
    M, N, K = 300, 136, 448
    g = gen_for(9)
    a, sa = random_codes(M, K, g, 1.0)
    w, sw = random_codes(N, K, g, K ** -0.5)
    bias = torch.randn(N, device=DEV, generator=g)
    full = call_abi(a, w, sa, sw, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, w, sa, sw, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 299), (77, 100), (130, 170)):
        part = call_abi(a[off:off + m].contiguous(), w, sa[off:off + m].contiguous(), sw, torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)
    f32 = call_abi(a, w, sa, sw, torch.float32)
    moved = torch.cat([a[200:201], a[:130]]).contiguous(), torch.cat([sa[200:201], sa[:130]]).contiguous()   # row 200 placed at m = 0
    assert torch.equal(call_abi(moved[0], w, moved[1], sw, torch.float32)[0], f32[200])


def test_python_wrapper_refusals_carry_the_rule():
    from viditq_extension import qgemm

    a = torch.zeros(8, 96, dtype=torch.uint8, device=DEV)
    w = torch.zeros(16, 96, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"fp8_linear: K=96 must be a positive multiple of 64"):
        qgemm.fp8_linear(a, w, ones(8), ones(16))
    a = torch.zeros(8, 128, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"fp8_linear: N=12 must be a positive multiple of 8"):
        qgemm.fp8_linear(a, torch.zeros(12, 128, dtype=torch.uint8, device=DEV), ones(8), ones(12))
    w = torch.zeros(16, 128, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"w_q must have dtype"):
        qgemm.fp8_linear(a, w.view(torch.int8), ones(8), ones(16))
    with pytest.raises(RuntimeError, match=r"a_scale must have shape"):
        qgemm.fp8_linear(a, w, ones(9), ones(16))
    with pytest.raises(RuntimeError, match=r"gate and residual must be given together"):
        qgemm.fp8_linear(a, w, ones(8), ones(16), gate=ones(16))
    out = qgemm.fp8_linear(a, w, ones(8), ones(16), torch.arange(16, device=DEV).float())
    assert out.dtype == torch.bfloat16 and torch.equal(out.float(), torch.arange(16, device=DEV).float().expand(8, 16))


# ---- 3. layer level ---------------------------------------------------------------------------------------------------------------
def _sim_layer(K=256, N=136):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    gen = torch.Generator().manual_seed(5)
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(torch.randn(N, K, generator=gen) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=gen) * 0.1)
    ql = QuantizedLinear(K, N, True, DEV, qcfg.load(YAML), fp, module_name="blocks.0.ffn.0")
    x = torch.randn(1, 133, K, generator=gen).to(torch.bfloat16).to(DEV)
    return ql, x


def test_simulation_and_kernel_mode_layers_run_the_same_entries_and_match_the_host_expression():
    from viditq_extension import fused, qgemm
    from wan.quant_wanx_hip import HipLinearFp8

    ql, x = _sim_layer()
    K, N = 256, 136
    w = ql.fp_module.weight.data
    wc, ws = cpu_quant(w.cpu())      # the weight went through the GPU entry: the same bits as the host expression
    assert ql.fp8 and torch.equal(ql._codes.cpu(), wc) and torch.equal(ql.w_quantizer.delta.reshape(-1).cpu(), ws)
    out = ql(x)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 133, N)
    q, s = fused.quant_rows_fp8(x[0])
    bias = ql.bias.detach().float()
    assert torch.equal(out[0], qgemm.fp8_linear(q, ql._codes, s, ql.w_quantizer.delta.reshape(-1).contiguous(), bias, torch.bfloat16))
    hl = HipLinearFp8.from_quantized(ql, "blocks.0.ffn.0")
    assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.delta.reshape(-1))
    assert torch.equal(hl(q, s, torch.bfloat16), out[0])
    # the host expression F.linear(fq(x), fq(w), bias) in float64, under the module's bound
    a64, w64 = decode(q).to(DEV), decode(ql._codes).to(DEV)
    y, tol = bound_case(a64.abs() @ w64.abs().T, a64 @ w64.T, s, hl.scale_weight, bias, False, None, None, torch.bfloat16, K)
    host = torch.nn.functional.linear((decode(q) * s.cpu().double()[:, None]), (decode(ql._codes) * ws.double()[:, None]), bias.cpu().double())
    assert float((host.to(DEV) - y).abs().max()) <= 1e-12 * float(y.abs().max())
    err = (out[0].double() - y).abs()
    print(f"fp8 layer vs the host expression: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()


def test_a_shape_the_gemm_refuses_falls_back_to_the_torch_expression():
    from qdiff.base.base_quantizer import fp8_decode
    from viditq_extension import fused

    ql, x = _sim_layer(K=96, N=24)
    q, s = fused.quant_rows_fp8(x[0, :, :96].contiguous())
    want = torch.nn.functional.linear(fp8_decode(q) * s[:, None], ql.weight.data.float(), ql.bias.detach().float()).to(torch.bfloat16)
    assert torch.equal(ql(x[:, :, :96].contiguous())[0], want)


# ---- 4. block and model level ---------------------------------------------------------------------------------------------------
def _tiny_model(cfg, layers=2):
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=layers, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 1, 20, 26)   # 130 tokens
    ctx = torch.randn(24, 64, device=DEV, generator=g) * 0.1
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, cfg)
    model.quant_layer_refactor()
    model.set_init_done()
    return model, fp, seq_len_for(shape), ctx, lat0


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_kernel_mode_block_matches_simulation_mode_and_the_checkpoint_round_trips(tmp_path, caplog):
    """One block (dim 256, ffn 512, 2 heads of 128, 130 tokens) built from w8a8_fp8_all_linears.yaml: kernel mode against simulation
    mode on the GPU.  Both run wanq_quant_rows_fp8 and wanq_gemm_fp8; what differs is the 16-bit tensors between kernel mode's layers.
    Margin: the one of tests/test_gpu_block.py::test_kernel_mode_block_vs_simulation_oracle for the per-channel W8A8 block -- rel
    Frobenius error below 1e-2 and below 0.5 x (quantised vs floating-point model) + 5e-3.  Then quantize_and_save_weight ->
    hardware_forward_refactor(load_path=...) gives the output of the model built directly, bit for bit."""
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearFp8

    t = torch.tensor([700], device=DEV)
    model, fp, seq_len, ctx, lat0 = _tiny_model(qcfg.load(YAML), layers=1)
    assert seq_len == 130
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref_fp = fp([lat0], t, [ctx], seq_len)[0].float().clone()
    sim = model([lat0], t, [ctx], seq_len)[0].float().clone()
    model.hardware_forward_refactor()
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearFp8)]
    assert len(lins) == 10 and all(m.weight.dtype == torch.uint8 for m in lins)
    hw = model([lat0], t, [ctx], seq_len)[0].float().clone()
    assert torch.isfinite(sim).all() and torch.isfinite(hw).all()
    err, noise = rel_l2(hw, sim), rel_l2(sim, ref_fp)
    print(f"fp8 block, kernel mode vs simulation mode: rel err {err:.3e}; simulation mode vs the floating-point model {noise:.3e}")
    assert noise > 0 and err < 1e-2 and err < 0.5 * noise + 5e-3

    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.2.weight"].dtype == torch.uint8 and tuple(sd["blocks.0.ffn.2.weight"].shape) == (256, 512)
    assert tuple(sd["blocks.0.ffn.2.scale_weight"].shape) == (256,) and "blocks.0.ffn.2.zp_weight" not in sd
    fresh, *_ = _tiny_model(qcfg.load(YAML), layers=1)
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=path)
    assert any("loaded 30 tensors" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, [ctx], seq_len)[0].float(), hw)


def test_two_pass_streams_and_sharded_weights_are_bit_equal_to_the_plain_kernel_mode_model():
    """the conditional and the unconditional pass on two streams (wan/utils/two_pass.py), and --dit_fsdp's re-pointing of `weight` at
    views of the gathered buffer (one rank: the whole buffer), give the bits of the plain kernel-mode model"""
    from qdiff import config as qcfg
    from wan.utils.two_pass import TwoPassStreams

    model, _, seq_len, ctx, lat0 = _tiny_model(qcfg.load(YAML))
    model.hardware_forward_refactor()
    ctxs = [ctx, torch.zeros_like(ctx)]
    t = torch.tensor([500], device=DEV)

    def both(two):
        out = two(lambda c: model([lat0], t, [c], seq_len)[0], lat0, ctxs)
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    one = both(TwoPassStreams(DEV, enabled=False))
    two = TwoPassStreams(DEV, mode="2")
    both(two)                      # (call 1 fills the caches both passes read, on one stream)
    assert two.enabled and all(torch.isfinite(a).all() and torch.equal(a, b) for a, b in zip(one, both(two)))
    model.shard_blocks(None)
    assert all(torch.equal(a, b) for a, b in zip(one, both(TwoPassStreams(DEV, enabled=False))))


def test_shipped_config_through_ptq_and_quant_generate(tmp_path):
    """ptq_wanx -> quant_generate (kernel mode from the exported checkpoint, and simulation mode) on the truncated backbone at toy size,
    as tests/test_gpu_entrypoints.py runs the other shipped configs; the config needs no calibration file.  Kernel mode against
    simulation mode: that test's margin for the per-channel W8A8 config (3e-2)."""
    from test_gpu_entrypoints import run

    run("ptq_wanx.py", "--quant_config", YAML, cwd=tmp_path)
    qp = torch.load(tmp_path / "checkpoint" / "quant_params.pth", weights_only=True)
    assert sum(1 for k in qp if k.endswith("w_quantizer")) == 20 and qp["blocks.0.self_attn.q.w_quantizer"]["delta"].shape == (1536, 1)
    iw = torch.load(tmp_path / "checkpoint" / "int_weight.pt", weights_only=True)
    assert iw["blocks.0.self_attn.q.weight"].dtype == torch.uint8 and tuple(iw["blocks.1.ffn.0.weight"].shape) == (8960, 1536)
    assert iw["blocks.1.ffn.0.scale_weight"].dtype == torch.float32 and "blocks.1.ffn.0.zp_weight" not in iw
    run("quant_generate.py", "--quant_config", YAML, cwd=tmp_path)
    hw = torch.load(tmp_path / "quant_latent_0.pt", weights_only=True).float()
    run("quant_generate.py", "--quant_config", YAML, "--hardware", "false", "--save_file", str(tmp_path / "sim.pt"), cwd=tmp_path)
    sim = torch.load(tmp_path / "sim.pt", weights_only=True).float()
    rel = ((hw - sim).norm() / sim.norm()).item()
    print(f"w8a8_fp8_all_linears.yaml: kernel mode vs simulation mode {rel:.3e}")
    assert hw.shape == (16, 2, 60, 104) and torch.isfinite(hw).all() and torch.isfinite(sim).all() and rel < 0.03
    # two ranks (one-GPU rehearsal, as tests/test_gpu_entrypoints.py launches it): Ulysses + --dit_fsdp reproduce the one-rank latent
    import socket
    import subprocess
    import sys

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(PKG, "quant_generate.py"), "--task", "t2v-1.3B", "--size", "832*480", "--frame_num", "5",
           "--num_layers", "2", "--sample_steps", "2", "--base_seed", "42", "--output_dir", str(tmp_path), "--quant_config", YAML,
           "--ulysses_size", "2", "--dit_fsdp", "--save_file", str(tmp_path / "two.pt")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_ON_ONE_GPU="1"))
    assert r.returncode == 0, f"two-rank quant_generate failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "dit_fsdp:" in r.stdout + r.stderr
    assert torch.equal(torch.load(tmp_path / "two.pt", weights_only=True).float(), hw)
