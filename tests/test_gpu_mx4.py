"""The W4A4 MXFP4 Linears on the GPU: the GEMM with both operands e2m1 (csrc/gemm_mx.hip, wanq_gemm_mx4 / qgemm.mx4_linear), the block
quantiser behind the 32-point Hadamard rotation (csrc/rowwise.hip, wanq_quant_rows_mx_had32 / fused.quant_rows_mx(had32=True)) and what
is built on them: simulation mode of a QuantizedLinear with `format: mxfp4_e2m1` on both sides, kernel mode's HipLinearMx, the integer
checkpoint, with quant_configs/mx/w4a4_mxfp4_all_linears.yaml and w4a4_mxfp4_had32_all_linears.yaml.

Probes A-C establish the token side of the 4-bit fragment cut as probes 1-3 of tests/test_gpu_mx.py did the weight side: which k a
token nibble is, which (row, block) each scale byte belongs to; every expected value is an exact small number.  The integer tests
use integer-valued e2m1 operands and scale exponents in {-1, 0, 1}: every partial sum is a multiple of 2^-2 below 2^24, exact in fp32
in any order, so the output must EQUAL the float64 evaluation.

Bound on random codes and random scale bytes: the form of tests/test_gpu_mx.py, |y - y64| <= MX4_ACC (1.01 K + 3) u S + the epilogue
terms (bias, GELU, gate + residual, the store; bound_case of tests/test_gpu_fp8.py).  MX4_ACC is twice the worst err / ((1.01 K + 3) u S)
measured against the float64 product for e2m1 x e2m1 (fp32 output, no bias; tools/bench_gemm_mx4.py, profiles/gemm_mx4.txt,
profiles/PARITY_NOTES.md "MX4 GEMM").  That worst case is 0 at K = 256, 1536 and 8960, on the tool's operands and on this file's: an
e2m1 value has two significant bits, a product four, and with scale exponents spread over 2^6 per side the 128 products of an
instruction and the running fp32 sum never need more than 24 bits, so the accumulation does not round at all.  Twice 0 is 0: on
these operands the test allows the epilogue's error and nothing for the accumulation.  Operands that come from the quantiser (every
block filled up to its top binade, real data behind them) are held to the plain bound of K - 1 fp32 additions, factor 1."""
import ctypes
import logging
import os

import pytest
import torch

from test_gpu_fp8 import OUTS, _tiny_model, bound_case, gen_for, ones, rel_l2
from test_gpu_mx import E2M1, deq64, e2m1, unit
from test_gpu_wq16 import DEV, DT, EPI_GATE_RES, EPI_GELU, PKG, Window

pytestmark = pytest.mark.gpu
MX4_ACC = 0.0   # twice the measured worst err / bound of the block-scaled accumulation, e2m1 x e2m1: measured 0 (module docstring)
FP8, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"
YAML44 = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_all_linears.yaml")
YAML44H = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_had32_all_linears.yaml")
YAML48 = os.path.join(PKG, "quant_configs", "w4a8_mxfp4_all_linears.yaml")
CFGS = pytest.mark.parametrize("path,had", [(YAML44, False), (YAML44H, True)], ids=["plain", "had32"])


def host_quant(x32, fmt, gelu=False, had32=False):
    from qdiff.base.base_quantizer import mx_quant_rows_host

    return mx_quant_rows_host(x32, fmt, gelu, had32)


def call_abi(a, w, sa, sw, out_dtype, bias=None, gelu=False, gate=None, residual=None, inplace=False):
    """wanq_gemm_mx4 through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape[0], a.shape[1] * 2
    N = w.shape[0]
    assert tuple(w.shape) == (N, K // 2) and tuple(sa.shape) == (M, K // 32) and tuple(sw.shape) == (N, K // 32)
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (a, w, sa, sw))
    win = Window(M, N, out_dtype)
    if residual is not None and inplace:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_mx4(a.data_ptr(), w.data_ptr(), sa.data_ptr(), sw.data_ptr(), win.out.data_ptr(), DT[out_dtype],
                              None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
                              None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


# ---- probes ---------------------------------------------------------------------------------------------------------------------------
def probe_operands(K, N=16):
    """token row m: the single code 1.0 at k = m; w[n, k]: the 15 non-zero e2m1 codes (-0 among them) by 1 + (3 n + 5 k) % 15, which
    differs between neighbouring k and between neighbouring n"""
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    code = 1 + (3 * n + 5 * k) % 15
    wv = torch.tensor(E2M1)[code & 7] * (1 - 2 * (code >> 3)).float()
    from qdiff.base.base_quantizer import mx_pack_e2m1

    w = mx_pack_e2m1(code.to(torch.uint8)).to(DEV).contiguous()
    return e2m1(torch.eye(K)), w, wv


@pytest.mark.parametrize("K", [256, 384])
def test_probe_a_token_k_map(K):
    """y[m, n] == w[n, m] for every (m, n): every nibble of a token fragment, all four lane groups, two and three K-tiles, rows in
    every 16-row block and in two and three row tiles"""
    a, w, wv = probe_operands(K)
    out = call_abi(a, w, unit(K, K), unit(16, K), torch.float32).cpu()
    assert torch.equal(out, wv.T.contiguous()), (out != wv.T).nonzero()[:8].tolist()


@pytest.mark.parametrize("K", [256, 384])
def test_probe_b_both_scale_maps(K):
    """probe A with sa[m, b] and sw[n, b] drawn from {126, 127, 128} by fixed patterns: y[m, n] == w[n, m] 2^(sa - 127 + sw - 127) with
    the bytes of block m / 32, so a byte taken from a neighbouring row or block shows as the wrong power of two"""
    a, w, wv = probe_operands(K)
    nb = K // 32
    m, b = torch.meshgrid(torch.arange(K), torch.arange(nb), indexing="ij")
    sa = (126 + (m + 2 * b) % 3).to(torch.uint8)
    n, b = torch.meshgrid(torch.arange(16), torch.arange(nb), indexing="ij")
    sw = (126 + (2 * n + b) % 3).to(torch.uint8)
    out = call_abi(a, w, sa.to(DEV), sw.to(DEV), torch.float32).cpu()
    blk = torch.arange(K) // 32
    e = (sa[torch.arange(K), blk].int() - 127)[:, None] + (sw[:, blk].int() - 127).T
    want = wv.T * torch.ldexp(torch.ones(K, 16), e)
    assert torch.equal(out, want), (out != want).nonzero()[:8].tolist()


def int_operands(M, N, K, seed):
    """integer e2m1 values {0, +-1, +-2, +-3, +-4, +-6} on both sides, scale exponents in {-1, 0, 1} per (row, block): |a w| 2^(ea + ew)
    <= 144 and a multiple of 2^-2, so every partial sum is exact in fp32 below 2^24"""
    g = torch.Generator().manual_seed(seed)
    ints = torch.tensor([0.0, 1, 2, 3, 4, 6])

    def side(rows):
        v = ints[torch.randint(0, 6, (rows, K), generator=g)] * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float()
        return e2m1(v), torch.randint(126, 129, (rows, K // 32), generator=g).to(torch.uint8).to(DEV)

    (a, sa), (w, sw) = side(M), side(N)
    return a, w, sa, sw, deq64(a, sa, FP4) @ deq64(w, sw, FP4).T


@pytest.mark.parametrize("N", [8, 136])
@pytest.mark.parametrize("K", [128, 256, 1536])
def test_probe_c_integer_operands_equal_the_float64_product_in_every_output_type(K, N):
    for M in (1, 127, 129, 130):
        a, w, sa, sw, acc = int_operands(M, N, K, K + M + N)
        assert torch.equal(acc.float().double(), acc) and float(acc.abs().max()) < 65504 and bool(acc.any())
        for out_dtype in OUTS:
            assert torch.equal(call_abi(a, w, sa, sw, out_dtype), acc.float().to(out_dtype)), (M, out_dtype)


# ---- epilogues ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_bias_gate_and_residual_exactly_in_every_output_type(out_dtype):
    """|gate| in {1/2, 1, 2}, integer bias (fp32, fp16 and bf16 vectors) and residual: every step is exact in fp32, so the output is the
    float64 value rounded once into the output type; out of place and with `out` aliasing `residual`"""
    M, N, K = 130, 136, 256
    a, w, sa, sw, acc = int_operands(M, N, K, 7)
    g = gen_for(11)
    bias = torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
    gate = (2.0 ** torch.randint(-1, 2, (N,), device=DEV, generator=g).float()) * (torch.randint(0, 2, (N,), device=DEV, generator=g) * 2 - 1)
    res = torch.randint(-16, 17, (M, N), device=DEV, generator=g).to(out_dtype)
    for b in (None, bias, bias.half(), bias.bfloat16()):
        y = acc + (0.0 if b is None else b.double())
        assert torch.equal(y.float().double(), y)
        assert torch.equal(call_abi(a, w, sa, sw, out_dtype, b), y.float().to(out_dtype))
        yr = res.double() + y * gate.double()
        assert torch.equal(yr.float().double(), yr)
        for inplace in (False, True):
            r = res.clone()
            out = call_abi(a, w, sa, sw, out_dtype, b, False, gate, r, inplace)
            assert torch.equal(out, yr.float().to(out_dtype)), (b is None, inplace)
            assert torch.equal(r, res)


@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_gelu_epilogue_on_exact_pre_activations(out_dtype):
    """the pre-activation is exact (sparse small integers, power-of-two scales), so the error is the GELU's alone: bound_case of
    tests/test_gpu_fp8.py with S = 0, then gate + residual and the store"""
    M, N, K = 130, 136, 128
    g0 = torch.Generator().manual_seed(5)
    ints = torch.tensor([0.0, 1, 2, 3, 4])
    av = ints[torch.randint(0, 5, (M, K), generator=g0)] * (torch.randint(0, 2, (M, K), generator=g0) * 2 - 1) * (torch.rand(M, K, generator=g0) < 0.1)
    wv = ints[torch.randint(0, 3, (N, K), generator=g0)] * (torch.randint(0, 2, (N, K), generator=g0) * 2 - 1)
    a, w = e2m1(av.float()), e2m1(wv.float())
    sa = torch.randint(125, 127, (M, K // 32), generator=g0).to(torch.uint8).to(DEV)
    sw = torch.randint(125, 128, (N, K // 32), generator=g0).to(torch.uint8).to(DEV)
    acc = deq64(a, sa, FP4) @ deq64(w, sw, FP4).T
    assert torch.equal(acc.float().double(), acc)
    g = gen_for(13)
    bias = torch.randint(-2, 3, (N,), device=DEV, generator=g).float() / 4
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
    zero = torch.zeros_like(acc)
    for gres in (False, True):
        out = call_abi(a, w, sa, sw, out_dtype, bias, True, gate if gres else None, res.clone() if gres else None)
        y, tol = bound_case(zero, acc, ones(M), ones(N), bias, True, gate if gres else None, res, out_dtype, 0)
        err = (out.double() - y).abs()
        assert not (err > tol).any(), (gres, (err / tol).max().item())


def test_m_zero_and_wrapper_refusals_carry_the_entrys_text():
    from viditq_extension import _C, qgemm

    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)  # noqa: E731
    t = z(16, 64)
    guard = torch.full((8, 16), 7.0, device=DEV, dtype=torch.bfloat16)
    rc = _C.lib.wanq_gemm_mx4(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), guard.data_ptr(), 1, None, 2, None, None, 0, 0, 16, 128, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((guard == 7.0).all())       # M == 0: accepted, nothing launched, nothing written
    rc = _C.lib.wanq_gemm_mx4(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, None, 2, None, None, 0, 8, 16, 64, None)
    assert rc != 0 and b"wanq_gemm_mx4: K=64 must be a positive multiple of 128" in _C.lib.wanq_last_error()
    rc = _C.lib.wanq_gemm_mx4(t.data_ptr(), t.data_ptr(), t.data_ptr() + 2, t.data_ptr(), t.data_ptr(), 1, None, 2, None, None, 0, 8, 16, 128, None)
    assert rc != 0 and b"wanq_gemm_mx4: sa_u8 and sw_u8 must be 4-byte aligned" in _C.lib.wanq_last_error()
    with pytest.raises(RuntimeError, match=r"mx4_linear: K=192 must be a positive multiple of 128"):
        qgemm.mx4_linear(z(8, 96), z(16, 96), z(8, 6), z(16, 6))
    with pytest.raises(RuntimeError, match=r"mx4_linear: N=12 must be a positive multiple of 8"):
        qgemm.mx4_linear(z(8, 64), z(12, 64), z(8, 4), z(12, 4))
    with pytest.raises(RuntimeError, match=r"w_q must have shape \(16, 64\)"):
        qgemm.mx4_linear(z(8, 64), z(16, 128), z(8, 4), z(16, 4))
    with pytest.raises(RuntimeError, match=r"a_scale must have shape"):
        qgemm.mx4_linear(z(8, 64), z(16, 64), z(8, 3), z(16, 4))
    with pytest.raises(RuntimeError, match=r"w_scale must have dtype"):
        qgemm.mx4_linear(z(8, 64), z(16, 64), z(8, 4), torch.ones(16, 4, device=DEV))
    with pytest.raises(RuntimeError, match=r"gate and residual must be given together"):
        qgemm.mx4_linear(z(8, 64), z(16, 64), z(8, 4), z(16, 4), gate=ones(16))
    out = qgemm.mx4_linear(z(8, 64), z(16, 64), z(8, 4), z(16, 4), torch.arange(16, device=DEV).float())
    assert out.dtype == torch.bfloat16 and torch.equal(out.float(), torch.arange(16, device=DEV).float().expand(8, 16))


# ---- random codes, determinism --------------------------------------------------------------------------------------------------------
def random_operands(M, N, K, gen):
    """random e2m1 codes and random scale bytes, the scale ranges of tests/test_gpu_mx.py::random_operands"""
    a = torch.randint(0, 256, (M, K // 2), device=DEV, generator=gen, dtype=torch.uint8)
    w = torch.randint(0, 256, (N, K // 2), device=DEV, generator=gen, dtype=torch.uint8)
    sa = torch.randint(117, 124, (M, K // 32), device=DEV, generator=gen, dtype=torch.uint8)
    sw = torch.randint(116, 123, (N, K // 32), device=DEV, generator=gen, dtype=torch.uint8)
    return a, w, sa, sw


@pytest.mark.parametrize("M,N,K", [(130, 136, 256), (300, 264, 1536), (257, 128, 8960)])
def test_random_codes_and_scale_bytes_within_the_derived_bound(M, N, K):
    g = gen_for(M + N + K)
    a, w, sa, sw = random_operands(M, N, K, g)
    a64, w64 = deq64(a, sa, FP4), deq64(w, sw, FP4)
    acc, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    assert float(S.max()) < 3e4                                                                               # every output inside fp16
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    plain = call_abi(a, w, sa, sw, torch.float32)
    raw = ((plain.double() - acc).abs() / ((1.01 * K + 3) * 2.0 ** -24 * S)).max().item()
    print(f"MX4 GEMM ({M}, {N}, {K}): worst err / ((1.01 K + 3) u S) against float64, fp32 output, no bias: {raw:.3e}")
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(a, w, sa, sw, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None, inplace=gres)
            y, tol = bound_case(MX4_ACC * S, acc, ones(M), ones(N), bias, gelu, gate if gres else None, res, out_dtype, K)
            err = (out.double() - y).abs()
            worst[(str(out_dtype)[6:], gelu, gres)] = round((err / tol).max().item(), 4)
    print(f"MX4 GEMM ({M}, {N}, {K}): worst err / (MX4_ACC = {MX4_ACC:.0f} bound, the epilogue terms alone) {max(worst.values()):.4f} {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_repeated_calls_and_rows_in_launches_of_another_size_are_bit_equal():
    M, N, K = 300, 136, 512
    g = gen_for(9)
    a, w, sa, sw = random_operands(M, N, K, g)
    bias = torch.randn(N, device=DEV, generator=g)
    full = call_abi(a, w, sa, sw, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, w, sa, sw, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 299), (77, 100), (130, 170)):
        part = call_abi(a[off:off + m].contiguous(), w, sa[off:off + m].contiguous(), sw, torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)
    f32 = call_abi(a, w, sa, sw, torch.float32)
    moved = torch.cat([a[200:201], a[:130]]).contiguous(), torch.cat([sa[200:201], sa[:130]]).contiguous()   # row 200 placed at m = 0
    assert torch.equal(call_abi(moved[0], w, moved[1], sw, torch.float32)[0], f32[200])


# ---- the rotating quantiser, bit for bit ----------------------------------------------------------------------------------------------
def special_blocks():
    """blocks whose ROTATED maximum sits at a power of two and one ulp either side (v e_0 rotates to v in all 32 places), a zero
    block, and the outlier block [8, 0.3 x 31]"""
    one = torch.tensor(1.0)
    out = []
    for v in (torch.nextafter(one, one * 0).item(), 1.0, torch.nextafter(one, one * 2).item(), 4.0, torch.nextafter(one * 4, one).item()):
        b = torch.zeros(32)
        b[0] = v
        out.append(b)
        b = torch.zeros(32)
        b[5] = -v
        out.append(b)
    out.append(torch.zeros(32))
    b = torch.full((32,), 0.3)
    b[0] = 8.0
    out.append(b)
    return out


@pytest.mark.parametrize("fmt", [FP8, FP4], ids=["e4m3", "e2m1"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [32, 1536, 8960, 13824])
def test_rotating_quantiser_matches_the_host_expression_bit_for_bit(cols, dtype, fmt):
    """rows 1, 3 and 257 (one wave, one ragged workgroup of the wave-per-row form, many workgroups); widths on the one-wave rungs
    (32, 1536) and the four-wave ones with a ragged last chunk slot (8960, 13824: NCH 5 and 7)"""
    from viditq_extension import fused

    nb = cols // 32
    for rows in (1, 3, 257):
        g = torch.Generator().manual_seed(cols + rows)
        x = torch.randn(rows, cols, generator=g) * (10.0 ** torch.randint(-3, 3, (rows, 1), generator=g).float())
        x[:, cols // 3] *= 25.0
        for j, blk in enumerate(special_blocks()):
            x.view(rows, nb, 32)[j % rows, (7 * j) % nb] = blk
        x = x.to(dtype)
        want, s = host_quant(x.float(), fmt, had32=True)
        codes, scale = fused.quant_rows_mx(x.to(DEV), fmt, had32=True)
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (rows, cols // (2 if fmt == FP4 else 1))
        assert torch.equal(scale.cpu(), s), (rows, (scale.cpu() != s).nonzero()[:8].tolist())
        bad = (codes.cpu() != want).nonzero()
        assert bad.numel() == 0, (rows, [(r, j, hex(codes[r, j].item()), hex(want[r, j].item())) for r, j in bad[:8].tolist()])
        plain, _ = fused.quant_rows_mx(x.to(DEV), fmt)
        assert not torch.equal(plain, codes)     # (the rotation is not a no-op)


def test_rotated_special_blocks_land_where_the_hand_figures_say():
    from viditq_extension import fused

    x = torch.stack(special_blocks()).reshape(1, -1)
    codes, scale = fused.quant_rows_mx(x.to(DEV), FP4, had32=True)
    want, s = host_quant(x, FP4, had32=True)
    assert torch.equal(codes.cpu(), want) and torch.equal(scale.cpu(), s)
    # amax just below 1 -> E = 126; 1 and just above -> 127; 4 -> 129, just below -> 128; zero block -> 0; the outlier block: 17.3 -> 131
    assert scale[0].tolist() == [124, 124, 125, 125, 125, 125, 127, 127, 126, 126, 0, 129]
    d = deq64(codes, scale, FP4)[0].view(-1, 32)
    assert d[-1, 0].item() == 16.0 and bool((d[-1, 1:] == 8.0).all()) and not bool(d[-2].any())


@pytest.mark.parametrize("fmt", [FP8, FP4], ids=["e4m3", "e2m1"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [64, 2112])
def test_gelu_form_rotates_this_librarys_own_gelu(cols, dtype, fmt):
    """act = 1 against the host expression applied to gelu_tanh_fast_f32(x) as the library itself computes it, the tolerance class of
    tests/test_gpu_mx.py::test_gelu_form_quantises_this_librarys_own_gelu: the GELU is held fixed, everything behind it is bit-equal"""
    from viditq_extension import fused, qgemm

    rows = 6
    g = torch.Generator().manual_seed(cols)
    x16 = (torch.randn(rows, cols, generator=g) * 3).to(torch.bfloat16 if dtype == torch.float32 else dtype).to(DEV)
    eye = torch.eye(64, dtype=x16.dtype, device=DEV)
    gel = qgemm.fp_linear(x16.view(-1, 64).contiguous(), eye, None, torch.float32, gelu=True).view(rows, cols)
    want, s = host_quant(gel.cpu(), fmt, had32=True)
    codes, scale = fused.quant_rows_mx(x16.to(dtype), fmt, gelu=True, had32=True)
    assert torch.equal(scale.cpu(), s) and torch.equal(codes.cpu(), want)


# ---- layer level ------------------------------------------------------------------------------------------------------------------
def _sim_layer(path, K, N, name, seed=5):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    gen = torch.Generator().manual_seed(seed)
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(torch.randn(N, K, generator=gen) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=gen) * 0.1)
    return QuantizedLinear(K, N, True, DEV, qcfg.load(path), fp, module_name=name), gen


@CFGS
def test_simulation_and_kernel_mode_layers_run_the_same_entries_under_the_plain_bound(path, had):
    """K = 256, N = 128, M = 130: the simulation-mode layer, the two entries called directly and HipLinearMx give the same bits; against
    the float64 product of the decoded (rotated) operands the error stays inside the plain bound of K - 1 fp32 additions.  Then
    ffn.0 -> ffn.2 with the late GELU: ffn.2's quantiser applies the GELU to ffn.0's 16-bit output"""
    from viditq_extension import fused, qgemm
    from wan.quant_wanx_hip import HipLinearMx, _late_gelu

    K, N, M = 256, 128, 130
    ql, gen = _sim_layer(path, K, N, "blocks.0.ffn.0")
    w = ql.fp_module.weight.data.cpu()
    wc, ws = host_quant(w * 0.03125, FP4, had32=True) if had else host_quant(w, FP4)
    assert ql.mx == FP4 and ql.mx_act == FP4 and ql.mx_had32 is had
    assert torch.equal(ql._codes.cpu(), wc) and torch.equal(ql.w_quantizer.scale_u8.cpu(), ws)
    x = torch.randn(1, M, K, generator=gen).to(torch.bfloat16).to(DEV)
    x[:, :, 9] *= 20
    out = ql(x)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, M, N)
    q, s = fused.quant_rows_mx(x[0], FP4, had32=had)
    bias = ql.bias.detach().float()
    assert torch.equal(out[0], qgemm.mx4_linear(q, ql._codes, s, ql.w_quantizer.scale_u8, bias, torch.bfloat16))
    hl = HipLinearMx.from_quantized(ql, "blocks.0.ffn.0")
    assert hl.a_fmt == FP4 and hl.had32 is had and torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.scale_u8)
    assert torch.equal(hl(q, s, torch.bfloat16), out[0])
    a64, w64 = deq64(q, s, FP4), deq64(ql._codes, ql.w_quantizer.scale_u8, FP4)
    assert torch.equal(w64.float(), ql.weight.data)
    y, tol = bound_case(a64.abs() @ w64.abs().T, a64 @ w64.T, ones(M), ones(N), bias, False, None, None, torch.bfloat16, K)
    err = (out[0].double() - y).abs()
    print(f"MX4 layer had32={had} vs the host expression: worst err / plain bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()
    fpy = ql.fp_module(x.float())
    print(f"MX4 layer had32={had} vs the floating-point layer (one outlier channel): rel err {rel_l2(out.float(), fpy):.3f}")

    # ffn.0 -> ffn.2, late GELU
    ql2, _ = _sim_layer(path, N, K, "blocks.0.ffn.2", seed=6)
    hl2 = HipLinearMx.from_quantized(ql2, "blocks.0.ffn.2")
    assert _late_gelu(hl, hl2)
    y0 = hl(q, s, torch.bfloat16)                                        # the pre-activation, 16 bits
    q2, s2 = fused.quant_rows_mx(y0, FP4, gelu=True, had32=had)          # what _FpSrc(gelu=True).rows(hl2.act_form) runs
    eye = torch.eye(64, dtype=torch.bfloat16, device=DEV)
    gel = qgemm.fp_linear(y0.view(-1, 64).contiguous(), eye, None, torch.float32, gelu=True).view(M, N)
    hq, hs = host_quant(gel.cpu(), FP4, had32=had)
    assert torch.equal(q2.cpu(), hq) and torch.equal(s2.cpu(), hs)
    res = torch.randn(M, K, generator=gen).to(DEV)
    gate = torch.rand(K, generator=gen).to(DEV)
    out2 = hl2(q2, s2, torch.float32, gate=gate, residual=res.clone())
    a64, w64 = deq64(q2, s2, FP4), deq64(hl2.weight, hl2.scale_weight, FP4)
    y, tol = bound_case(a64.abs() @ w64.abs().T, a64 @ w64.T, ones(M), ones(K), hl2.bias, False, gate, res, torch.float32, N)
    assert not ((out2.double() - y).abs() > tol).any()


@CFGS
def test_src_rows_makes_one_copy_per_form(path, had):
    """q / k / v of one source share one quantised copy: _FpSrc.rows(form) runs the quantiser once and hands the same tensors out"""
    from wan.quant_wanx_hip import _FpSrc

    form = "mxfp4_h32" if had else "mxfp4"
    t = torch.randn(40, 256, device=DEV, generator=gen_for(3)).to(torch.bfloat16)
    src = _FpSrc(t)
    q, s = src.rows(form)
    assert src.rows(form)[0] is q and tuple(q.shape) == (40, 128) and tuple(s.shape) == (40, 8)
    hq, hs = host_quant(t.float().cpu(), FP4, had32=had)
    assert torch.equal(q.cpu(), hq) and torch.equal(s.cpu(), hs)
    q8, _ = src.rows("mxfp8")
    assert tuple(q8.shape) == (40, 256) and src.rows(form)[0] is q


# ---- block and model level ------------------------------------------------------------------------------------------------------
@CFGS
def test_kernel_mode_model_matches_simulation_mode_and_the_checkpoint_round_trips(tmp_path, caplog, path, had):
    """The tiny 2-block model of tests/test_gpu_mx.py (dim 256, ffn 512, 2 heads of 128, 130 tokens) under each W4A4 config: kernel mode
    against simulation mode, under that file's bar -- rel Frobenius error below 1e-2 and below 0.5 x (quantised vs floating-point
    model) + 5e-3.  Then quantize_and_save_weight -> hardware_forward_refactor(load_path=...) gives the output of the model built
    directly, bit for bit; codes saved under the other rotation setting are refused by layer name."""
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearMx

    t = torch.tensor([700], device=DEV)
    model, fp, seq_len, ctx, lat0 = _tiny_model(qcfg.load(path))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref_fp = fp([lat0], t, [ctx], seq_len)[0].float().clone()
    sim = model([lat0], t, [ctx], seq_len)[0].float().clone()
    model.hardware_forward_refactor()
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearMx)]
    assert len(lins) == 20 and all(m.a_fmt == FP4 and m.mx == FP4 and m.had32 is had for m in lins)
    hw = model([lat0], t, [ctx], seq_len)[0].float().clone()
    assert torch.isfinite(sim).all() and torch.isfinite(hw).all()
    err, noise = rel_l2(hw, sim), rel_l2(sim, ref_fp)
    print(f"MX4 model had32={had}, kernel mode vs simulation mode: rel err {err:.3e}; simulation mode vs the floating-point model {noise:.3e}")
    assert noise > 0 and err < 1e-2 and err < 0.5 * noise + 5e-3

    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    assert sd["blocks.0.ffn.2.weight"].dtype == torch.uint8 and tuple(sd["blocks.0.ffn.2.weight"].shape) == (256, 256)
    assert tuple(sd["blocks.0.ffn.2.scale_weight"].shape) == (256, 16) and ("blocks.0.ffn.2.mx_had32" in sd) is had
    fresh, *_ = _tiny_model(qcfg.load(path))
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=file)
    assert any(f"loaded {80 if had else 60} tensors" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, [ctx], seq_len)[0].float(), hw)
    other, *_ = _tiny_model(qcfg.load(YAML44 if had else YAML44H))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q holds codes quantised " + ("behind" if had else "without")):
        other.hardware_forward_refactor(load_path=file)


def test_an_existing_style_w4a8_checkpoint_still_loads(tmp_path):
    from qdiff import config as qcfg

    t = torch.tensor([700], device=DEV)
    model, _, seq_len, ctx, lat0 = _tiny_model(qcfg.load(YAML48))
    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    assert not any(k.endswith(".mx_had32") for k in sd)
    hw = model.hardware_forward_refactor()([lat0], t, [ctx], seq_len)[0].float().clone()
    fresh, *_ = _tiny_model(qcfg.load(YAML48))
    assert torch.equal(fresh.hardware_forward_refactor(load_path=file)([lat0], t, [ctx], seq_len)[0].float(), hw)
