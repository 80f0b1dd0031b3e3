"""The MXFP6 (e2m3) Linears on the GPU: the block quantiser to 6-bit codes (csrc/rowwise.hip, wanq_quant_rows_mx6 /
fused.quant_rows_mx(fmt="mxfp6_e2m3fn")), the GEMM with e2m3 tokens against e2m3 or packed e2m1 weights (csrc/gemm_mx.hip, wanq_gemm_mx6 /
qgemm.mx6_linear) and what is built on them: simulation mode of a QuantizedLinear, kernel mode's HipLinearMx and the integer checkpoint
under quant_configs/mx/w6a6_mxfp6_all_linears.yaml and w4a6_mxfp4_mxfp6_all_linears.yaml.

Probes A-C establish the 6-bit fragment cut on the hardware, on both operand sides: which k and which bit positions of the six
registers a code is, which (row, block) each scale byte belongs to; every expected value is an exact small number.  Probe C uses
integer-valued operands (e2m3: {0, +-1 .. +-7}; e2m1: {0, +-1, 2, 3, 4, 6}) and scale exponents in {-1, 0, 1}: every partial sum is a
multiple of 2^-2 below 2^24, exact in fp32 in any order, so the output must EQUAL the float64 product.

Bound on random codes and random scale bytes: that of tests/test_gpu_mx.py with its accumulation factor MX_ACC = 24,
|y - y64| <= MX_ACC (1.01 K + 3) u S + the epilogue terms (bound_case of tests/test_gpu_fp8.py).  It carries over because every e2m3
and every e2m1 value is also an e4m3 value: these operands are a subset of what that constant was measured on.  The raw ratio
err / ((1.01 K + 3) u S) is printed.  Operands that come from the quantiser are held to the plain bound of K - 1 fp32 additions."""
import ctypes
import logging
import os

import pytest
import torch

from test_gpu_fp8 import OUTS, _tiny_model, bound_case, gen_for, ones, rel_l2
from test_gpu_mx import MX_ACC, deq64, e2m1, unit
from test_gpu_mx4 import probe_operands as probe_operands_e2m1
from test_gpu_wq16 import DEV, DT, EPI_GATE_RES, EPI_GELU, PKG, Window

pytestmark = pytest.mark.gpu
FP6, FP4, FP8 = "mxfp6_e2m3fn", "mxfp4_e2m1", "mxfp8_e4m3"
YAML66 = os.path.join(PKG, "quant_configs", "mx", "w6a6_mxfp6_all_linears.yaml")
YAML46 = os.path.join(PKG, "quant_configs", "mx", "w4a6_mxfp4_mxfp6_all_linears.yaml")
YAML48 = os.path.join(PKG, "quant_configs", "w4a8_mxfp4_all_linears.yaml")
YAML44 = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_all_linears.yaml")
WFMTS = pytest.mark.parametrize("w_fmt", [FP6, FP4], ids=["w6", "w4"])
CFGS = pytest.mark.parametrize("path,w_fmt", [(YAML66, FP6), (YAML46, FP4)], ids=["w6a6", "w4a6"])
# the 32 e2m3 magnitudes, written out from the rule: E = 0: M / 8; E > 0: 2^(E - 1) (1 + M / 8)
E2M3 = (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
        2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5)
GUARD = 256


def host_quant(x32, fmt=FP6, gelu=False):
    from qdiff.base.base_quantizer import mx_quant_rows_host

    return mx_quant_rows_host(x32, fmt, gelu)


def pack6(codes):
    """[rows, K] 6-bit codes -> the stored bytes [rows, 3 K / 4], on the GPU: element j of a block in bits 6 j .. 6 j + 5 of the block's
    192-bit little-endian string, built bit by bit (independent of mx_pack_e2m3)"""
    c = codes.to(torch.int64)
    rows, K = c.shape
    bits = ((c[:, :, None] >> torch.arange(6)) & 1).reshape(rows, K * 6)
    return (bits.reshape(rows, K * 6 // 8, 8) << torch.arange(8)).sum(-1).to(torch.uint8).to(DEV).contiguous()


def e2m3(t):
    """exactly representable values [rows, cols] -> packed e2m3 codes [rows, 3 cols / 4] on the GPU"""
    t = t.detach().float().cpu()
    lut = torch.tensor(E2M3)
    mag = (t.abs()[..., None] == lut).float().argmax(-1)
    assert torch.equal(lut[mag], t.abs()), "not exact in e2m3"
    return pack6(mag | (torch.signbit(t).long() << 5))


def codes_of(t, fmt):
    return e2m3(t) if fmt == FP6 else e2m1(t)


class ByteWindow:
    """a [rows, cols] uint8 output between two guard regions of one flat allocation, everything preset to 0xA5"""

    def __init__(self, rows, cols):
        self.n = rows * cols
        self.flat = torch.full((2 * GUARD + self.n,), 0xA5, dtype=torch.uint8, device=DEV)
        self.out = self.flat[GUARD:GUARD + self.n].view(rows, cols)
        assert self.out.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.flat[:GUARD] == 0xA5).all()) and bool((self.flat[GUARD + self.n:] == 0xA5).all())


def quant_abi(x, gelu=False, entry="wanq_quant_rows_mx6"):
    """wanq_quant_rows_mx6 (or wanq_quant_rows_mx with fmt E2M1) through the C ABI into guarded windows -> (codes, scale bytes)"""
    from viditq_extension import _C

    rows, cols = x.shape
    six = entry == "wanq_quant_rows_mx6"
    q, s = ByteWindow(rows, cols // 4 * 3 if six else cols // 2), ByteWindow(rows, cols // 32)
    args = (x.data_ptr(), DT[x.dtype], q.out.data_ptr(), s.out.data_ptr(), rows, cols) + (() if six else (1,)) + \
        (1 if gelu else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = getattr(_C.lib, entry)(*args)
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert q.guards_intact() and s.guards_intact(), "a guard region next to the codes or the scale bytes was written"
    return q.out, s.out


def call_abi(a, w, sa, sw, w_fmt, out_dtype, bias=None, gelu=False, gate=None, residual=None, inplace=False):
    """wanq_gemm_mx6 through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape[0], a.shape[1] // 3 * 4
    N = w.shape[0]
    assert tuple(a.shape) == (M, K // 4 * 3) and tuple(w.shape) == (N, K // 4 * 3 if w_fmt == FP6 else K // 2)
    assert tuple(sa.shape) == (M, K // 32) and tuple(sw.shape) == (N, K // 32)
    assert all(t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda for t in (a, w, sa, sw))
    win = Window(M, N, out_dtype)
    if residual is not None and inplace:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_mx6(a.data_ptr(), w.data_ptr(), sa.data_ptr(), sw.data_ptr(), _C.MX6_FMT[w_fmt], win.out.data_ptr(), DT[out_dtype],
                              None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
                              None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


# ---- the quantiser, bit for bit -------------------------------------------------------------------------------------------------------
def special_blocks():
    """hand-figured blocks -> (values [32], scale byte, the 32 codes)"""
    out = [(torch.zeros(32), 0, [0] * 32)]
    for e in (-3, 0, 5):      # one element at 7.75 x 2^e: E = 129 + e, s = 127 + e, t = 7.75 is clamped to 7.5 = code 31
        b = torch.zeros(32)
        b[3], b[4], b[31] = 7.75 * 2.0 ** e, -7.75 * 2.0 ** e, 2.0 ** e
        out.append((b, 127 + e, [0, 0, 0, 31, 63, *[0] * 26, 8]))
    # ties at every quantum, block pinned at 7.5 (s = 127): 1/16 -> 0, 3/16 -> 2 (0.25), 1.9375 -> 16 (2.0), 2.125 -> 16, 2.375 -> 18
    # (2.5), 3.875 -> 24 (4.0), 4.25 -> 24, 4.75 -> 26 (5.0), 7.25 -> 30 (7.0); and the negative tie that rounds to zero keeps its sign
    ties = [0.0625, 0.1875, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 7.25, -0.0625, -0.1875, -2.125, -7.25]
    want = [0, 2, 16, 16, 18, 24, 24, 26, 30, 32, 34, 48, 62]
    b = torch.zeros(32)
    b[0] = 7.5
    b[1:1 + len(ties)] = torch.tensor(ties)
    out.append((b, 127, [31, *want, *[0] * (31 - len(want))]))
    b = torch.zeros(32)       # -0 keeps its sign, in a block of its own scale (amax 1: E = 127, s = 125, 1 -> t = 4 = code 24)
    b[0], b[1], b[2] = 1.0, -0.0, -1.0
    out.append((b, 125, [24, 32, 56, *[0] * 29]))
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [32, 1536, 8960, 13824])
def test_quantiser_matches_the_host_expression_bit_for_bit(cols, dtype):
    """rows 1, 3 and 257 (one wave, one ragged workgroup of the wave-per-row form, many workgroups); widths on the one-wave rungs (32,
    1536) and the four-wave ones with a ragged last chunk slot (8960, 13824).  Codes and scale bytes equal the host expression's, and
    the scale bytes equal wanq_quant_rows_mx(fmt = E2M1)'s on the same input, all through the ABI into guarded windows"""
    nb = cols // 32
    for rows in (1, 3, 257):
        g = torch.Generator().manual_seed(cols + rows)
        x = torch.randn(rows, cols, generator=g) * (10.0 ** torch.randint(-3, 3, (rows, 1), generator=g).float())
        x[:, cols // 3] *= 25.0
        for j, (blk, _, _) in enumerate(special_blocks()):
            x.view(rows, nb, 32)[j % rows, (7 * j) % nb] = blk
        x = x.to(dtype)
        want, s = host_quant(x.float())
        codes, scale = quant_abi(x.to(DEV))
        assert tuple(codes.shape) == (rows, cols // 4 * 3) and tuple(scale.shape) == (rows, nb)
        assert torch.equal(scale.cpu(), s), (rows, (scale.cpu() != s).nonzero()[:8].tolist())
        bad = (codes.cpu() != want).nonzero()
        assert bad.numel() == 0, (rows, [(r, j, hex(codes[r, j].item()), hex(want[r, j].item())) for r, j in bad[:8].tolist()])
        _, s4 = quant_abi(x.to(DEV), entry="wanq_quant_rows_mx")
        assert torch.equal(s4, scale)


def test_special_blocks_land_where_the_hand_figures_say():
    from qdiff.base.base_quantizer import mx_unpack_e2m3

    blocks = special_blocks()
    x = torch.stack([b for b, _, _ in blocks]).reshape(1, -1)
    codes, scale = quant_abi(x.to(DEV))
    assert scale[0].tolist() == [s for _, s, _ in blocks]
    got = mx_unpack_e2m3(codes.cpu()).view(-1, 32).tolist()
    assert got == [c for _, _, c in blocks]
    assert torch.equal(codes, pack6(torch.tensor([c for _, _, c in blocks]).reshape(1, -1)))
    want, s = host_quant(x)
    assert torch.equal(codes.cpu(), want) and torch.equal(scale.cpu(), s)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", [64, 2112])
def test_gelu_form_quantises_this_librarys_own_gelu(cols, dtype):
    """act = 1 against the host expression applied to gelu_tanh_fast_f32(x) as the library itself computes it, the tolerance class of
    tests/test_gpu_mx.py::test_gelu_form_quantises_this_librarys_own_gelu: the GELU is held fixed, everything behind it is bit-equal"""
    from viditq_extension import fused, qgemm

    rows = 6
    g = torch.Generator().manual_seed(cols)
    x16 = (torch.randn(rows, cols, generator=g) * 3).to(torch.bfloat16 if dtype == torch.float32 else dtype).to(DEV)
    eye = torch.eye(64, dtype=x16.dtype, device=DEV)
    gel = qgemm.fp_linear(x16.view(-1, 64).contiguous(), eye, None, torch.float32, gelu=True).view(rows, cols)
    want, s = host_quant(gel.cpu(), gelu=False)
    codes, scale = quant_abi(x16.to(dtype).contiguous(), gelu=True)
    assert torch.equal(scale.cpu(), s) and torch.equal(codes.cpu(), want)
    c2, s2 = fused.quant_rows_mx(x16.to(dtype), FP6, gelu=True)
    assert torch.equal(c2, codes) and torch.equal(s2, scale)


# ---- probes ---------------------------------------------------------------------------------------------------------------------------
def pattern6(rows, K):
    """codes[r, k] = 1 + (5 r + 11 k) % 63: the 63 non-zero e2m3 codes (-0 among them), different between neighbouring k and neighbouring
    rows -> (packed codes on the GPU, their values)"""
    r, k = torch.meshgrid(torch.arange(rows), torch.arange(K), indexing="ij")
    code = 1 + (5 * r + 11 * k) % 63
    val = torch.tensor(E2M3)[code & 31] * (1 - 2 * (code >> 5)).float()
    return pack6(code), val


def probe_sides(K, w_fmt, swapped):
    """-> a, w, the expected [M, N] output for unit scales.  Plain: token row m is the single code 1.0 at k = m (M = K) and the 16 weight
    rows are patterned, y[m, n] = w[n, m].  Swapped: weight row n is the single code 1.0 at k = n (N = K) and 16 token rows are
    patterned, y[m, n] = a[m, n]"""
    if not swapped:
        a = e2m3(torch.eye(K))
        if w_fmt == FP6:
            w, wv = pattern6(16, K)
        else:
            _, w, wv = probe_operands_e2m1(K)
        return a, w, wv.T.contiguous()
    a, av = pattern6(16, K)
    return a, codes_of(torch.eye(K), w_fmt), av


@WFMTS
@pytest.mark.parametrize("swapped", [False, True], ids=["tokens_one_hot", "weights_one_hot"])
@pytest.mark.parametrize("K", [256, 384])
def test_probe_a_k_map_and_bit_order(K, swapped, w_fmt):
    """every code position of a fragment's six registers, all four lane groups, two and three K-tiles, rows in every 16-row block and
    in two and three row (channel) tiles, on the weight side and on the token side"""
    a, w, want = probe_sides(K, w_fmt, swapped)
    out = call_abi(a, w, unit(a.shape[0], K), unit(w.shape[0], K), w_fmt, torch.float32).cpu()
    assert torch.equal(out, want), (out != want).nonzero()[:8].tolist()


@WFMTS
@pytest.mark.parametrize("swapped", [False, True], ids=["tokens_one_hot", "weights_one_hot"])
@pytest.mark.parametrize("K", [256, 384])
def test_probe_b_both_scale_maps(K, swapped, w_fmt):
    """probe A with sa[m, b] and sw[n, b] drawn from {126, 127, 128} by the patterns of tests/test_gpu_mx4.py: every output is the unit-scale
    value times 2^(sa - 127 + sw - 127) with the bytes of the one-hot element's block"""
    a, w, base = probe_sides(K, w_fmt, swapped)
    M, N, nb = a.shape[0], w.shape[0], K // 32
    m, b = torch.meshgrid(torch.arange(M), torch.arange(nb), indexing="ij")
    sa = (126 + (m + 2 * b) % 3).to(torch.uint8)
    n, b = torch.meshgrid(torch.arange(N), torch.arange(nb), indexing="ij")
    sw = (126 + (2 * n + b) % 3).to(torch.uint8)
    out = call_abi(a, w, sa.to(DEV), sw.to(DEV), w_fmt, torch.float32).cpu()
    if not swapped:   # the product's one k is m
        blk = torch.arange(M) // 32
        e = (sa[torch.arange(M), blk].int() - 127)[:, None] + (sw[:, blk].int() - 127).T
    else:             # ... is n
        blk = torch.arange(N) // 32
        e = (sa[:, blk].int() - 127) + (sw[torch.arange(N), blk].int() - 127)[None, :]
    want = base * torch.ldexp(torch.ones(M, N), e)
    assert torch.equal(out, want), (out != want).nonzero()[:8].tolist()


def int_operands(M, N, K, w_fmt, seed):
    """integer values on both sides, e2m3 {0, +-1 .. +-7}, e2m1 {0, +-1, 2, 3, 4, 6}; scale exponents in {-1, 0, 1} per (row, block):
    |a w| 2^(ea + ew) <= 196 and a multiple of 2^-2, so every partial sum is exact in fp32 below 2^24"""
    g = torch.Generator().manual_seed(seed)

    def side(rows, fmt):
        ints = torch.arange(8).float() if fmt == FP6 else torch.tensor([0.0, 1, 2, 3, 4, 6])
        v = ints[torch.randint(0, len(ints), (rows, K), generator=g)] * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float()
        return codes_of(v, fmt), torch.randint(126, 129, (rows, K // 32), generator=g).to(torch.uint8).to(DEV)

    (a, sa), (w, sw) = side(M, FP6), side(N, w_fmt)
    return a, w, sa, sw, deq64(a, sa, FP6) @ deq64(w, sw, w_fmt).T


@WFMTS
@pytest.mark.parametrize("N", [8, 136])
@pytest.mark.parametrize("K", [128, 256, 1536])
def test_probe_c_integer_operands_equal_the_float64_product_in_every_output_type(K, N, w_fmt):
    for M in (1, 127, 129, 130):
        a, w, sa, sw, acc = int_operands(M, N, K, w_fmt, K + M + N)
        assert torch.equal(acc.float().double(), acc) and float(acc.abs().max()) < 65504 and bool(acc.any())
        for out_dtype in OUTS:
            assert torch.equal(call_abi(a, w, sa, sw, w_fmt, out_dtype), acc.float().to(out_dtype)), (M, out_dtype)


# ---- epilogues ------------------------------------------------------------------------------------------------------------------------
@WFMTS
@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_bias_gate_and_residual_exactly_in_every_output_type(out_dtype, w_fmt):
    """|gate| in {1/2, 1, 2}, integer bias (fp32, fp16 and bf16 vectors) and residual: every step is exact in fp32, so the output is the
    float64 value rounded once into the output type; out of place and with `out` aliasing `residual`"""
    M, N, K = 130, 136, 256
    a, w, sa, sw, acc = int_operands(M, N, K, w_fmt, 7)
    g = gen_for(11)
    bias = torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
    gate = (2.0 ** torch.randint(-1, 2, (N,), device=DEV, generator=g).float()) * (torch.randint(0, 2, (N,), device=DEV, generator=g) * 2 - 1)
    res = torch.randint(-16, 17, (M, N), device=DEV, generator=g).to(out_dtype)
    for b in (None, bias, bias.half(), bias.bfloat16()):
        y = acc + (0.0 if b is None else b.double())
        assert torch.equal(y.float().double(), y)
        assert torch.equal(call_abi(a, w, sa, sw, w_fmt, out_dtype, b), y.float().to(out_dtype))
        yr = res.double() + y * gate.double()
        assert torch.equal(yr.float().double(), yr)
        for inplace in (False, True):
            r = res.clone()
            out = call_abi(a, w, sa, sw, w_fmt, out_dtype, b, False, gate, r, inplace)
            assert torch.equal(out, yr.float().to(out_dtype)), (b is None, inplace)
            assert torch.equal(r, res)


@WFMTS
@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
def test_gelu_epilogue_on_exact_pre_activations(out_dtype, w_fmt):
    """the pre-activation is exact (sparse small integers, power-of-two scales), so the error is the GELU's alone: bound_case of
    tests/test_gpu_fp8.py with S = 0, then gate + residual and the store"""
    M, N, K = 130, 136, 128
    g0 = torch.Generator().manual_seed(5)
    ints = torch.tensor([0.0, 1, 2, 3, 4])
    av = ints[torch.randint(0, 5, (M, K), generator=g0)] * (torch.randint(0, 2, (M, K), generator=g0) * 2 - 1) * (torch.rand(M, K, generator=g0) < 0.1)
    wv = ints[torch.randint(0, 3, (N, K), generator=g0)] * (torch.randint(0, 2, (N, K), generator=g0) * 2 - 1)
    a, w = e2m3(av.float()), codes_of(wv.float(), w_fmt)
    sa = torch.randint(125, 127, (M, K // 32), generator=g0).to(torch.uint8).to(DEV)
    sw = torch.randint(125, 128, (N, K // 32), generator=g0).to(torch.uint8).to(DEV)
    acc = deq64(a, sa, FP6) @ deq64(w, sw, w_fmt).T
    assert torch.equal(acc.float().double(), acc)
    g = gen_for(13)
    bias = torch.randint(-2, 3, (N,), device=DEV, generator=g).float() / 4
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
    zero = torch.zeros_like(acc)
    for gres in (False, True):
        out = call_abi(a, w, sa, sw, w_fmt, out_dtype, bias, True, gate if gres else None, res.clone() if gres else None)
        y, tol = bound_case(zero, acc, ones(M), ones(N), bias, True, gate if gres else None, res, out_dtype, 0)
        err = (out.double() - y).abs()
        assert not (err > tol).any(), (gres, (err / tol).max().item())


def test_m_zero_and_wrapper_refusals_carry_the_entrys_text():
    from viditq_extension import _C, fused, qgemm

    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)  # noqa: E731
    t = z(16, 96)
    guard = torch.full((8, 16), 7.0, device=DEV, dtype=torch.bfloat16)
    rc = _C.lib.wanq_gemm_mx6(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, guard.data_ptr(), 1, None, 2, None, None, 0, 0, 16, 128, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((guard == 7.0).all())       # M == 0: accepted, nothing launched, nothing written
    rc = _C.lib.wanq_gemm_mx6(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, t.data_ptr(), 1, None, 2, None, None, 0, 8, 16, 64, None)
    assert rc != 0 and b"wanq_gemm_mx6: K=64 must be a positive multiple of 128" in _C.lib.wanq_last_error()
    rc = _C.lib.wanq_gemm_mx6(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, t.data_ptr(), 1, None, 2, None, None, 0, 8, 16, 128, None)
    assert rc != 0 and b"wanq_gemm_mx6: w_fmt=0 must be WANQ_MX_E2M3 or WANQ_MX_E2M1" in _C.lib.wanq_last_error()
    with pytest.raises(RuntimeError, match=r"mx6_linear: K=192 must be a positive multiple of 128"):
        qgemm.mx6_linear(z(8, 144), z(16, 144), z(8, 6), z(16, 6))
    with pytest.raises(RuntimeError, match=r"mx6_linear: w_fmt='mxfp8_e4m3' must be one of"):
        qgemm.mx6_linear(z(8, 96), z(16, 128), z(8, 4), z(16, 4), FP8)
    with pytest.raises(RuntimeError, match=r"w_q must have shape \(16, 64\)"):
        qgemm.mx6_linear(z(8, 96), z(16, 96), z(8, 4), z(16, 4), FP4)
    with pytest.raises(RuntimeError, match=r"w_q must have shape \(16, 96\)"):
        qgemm.mx6_linear(z(8, 96), z(16, 64), z(8, 4), z(16, 4), FP6)
    with pytest.raises(RuntimeError, match=r"a_scale must have shape"):
        qgemm.mx6_linear(z(8, 96), z(16, 96), z(8, 3), z(16, 4))
    with pytest.raises(RuntimeError, match=r"no had32 form"):
        fused.quant_rows_mx(torch.zeros(2, 64, device=DEV), FP6, had32=True)
    out = qgemm.mx6_linear(z(8, 96), z(16, 96), z(8, 4), z(16, 4), FP6, torch.arange(16, device=DEV).float())
    assert out.dtype == torch.bfloat16 and torch.equal(out.float(), torch.arange(16, device=DEV).float().expand(8, 16))
    assert _C.lib.wanq_quant_rows_mx6(t.data_ptr(), 2, t.data_ptr(), t.data_ptr(), 0, 64, 0, None) == 0   # rows == 0: nothing launched


# ---- random codes, determinism --------------------------------------------------------------------------------------------------------
def random_operands(M, N, K, w_fmt, gen):
    """random e2m3 codes (every byte pattern is four finite codes), random e2m3 / e2m1 weight codes and random scale bytes, the scale
    ranges of tests/test_gpu_mx.py::random_operands"""
    a = torch.randint(0, 256, (M, K // 4 * 3), device=DEV, generator=gen, dtype=torch.uint8)
    w = torch.randint(0, 256, (N, K // 4 * 3 if w_fmt == FP6 else K // 2), device=DEV, generator=gen, dtype=torch.uint8)
    sa = torch.randint(117, 124, (M, K // 32), device=DEV, generator=gen, dtype=torch.uint8)
    sw = torch.randint(116, 123, (N, K // 32), device=DEV, generator=gen, dtype=torch.uint8)
    return a, w, sa, sw


@WFMTS
@pytest.mark.parametrize("M,N,K", [(130, 136, 256), (300, 264, 1536), (257, 128, 8960)])
def test_random_codes_and_scale_bytes_within_the_mx_bound(M, N, K, w_fmt):
    g = gen_for(M + N + K)
    a, w, sa, sw = random_operands(M, N, K, w_fmt, g)
    a64, w64 = deq64(a, sa, FP6), deq64(w, sw, w_fmt)
    acc, S = a64 @ w64.T, a64.abs() @ w64.abs().T
    assert float(S.max()) < 3e4                                                                               # every output inside fp16
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    plain = call_abi(a, w, sa, sw, w_fmt, torch.float32)
    raw = ((plain.double() - acc).abs() / ((1.01 * K + 3) * 2.0 ** -24 * S)).max().item()
    print(f"MX6 GEMM {w_fmt} ({M}, {N}, {K}): worst err / ((1.01 K + 3) u S) against float64, fp32 output, no bias: {raw:.3e}")
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(a, w, sa, sw, w_fmt, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None, inplace=gres)
            y, tol = bound_case(MX_ACC * S, acc, ones(M), ones(N), bias, gelu, gate if gres else None, res, out_dtype, K)
            err = (out.double() - y).abs()
            worst[(str(out_dtype)[6:], gelu, gres)] = round((err / tol).max().item(), 4)
    print(f"MX6 GEMM {w_fmt} ({M}, {N}, {K}): worst err / (MX_ACC = {MX_ACC:.0f} bound) {max(worst.values()):.4f} {worst}")
    assert max(worst.values()) <= 1.0, worst


@WFMTS
def test_repeated_calls_and_rows_in_launches_of_another_size_are_bit_equal(w_fmt):
    M, N, K = 300, 136, 512
    g = gen_for(9)
    a, w, sa, sw = random_operands(M, N, K, w_fmt, g)
    bias = torch.randn(N, device=DEV, generator=g)
    full = call_abi(a, w, sa, sw, w_fmt, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, w, sa, sw, w_fmt, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 299), (77, 100), (130, 170)):
        part = call_abi(a[off:off + m].contiguous(), w, sa[off:off + m].contiguous(), sw, w_fmt, torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)
    f32 = call_abi(a, w, sa, sw, w_fmt, torch.float32)
    moved = torch.cat([a[200:201], a[:130]]).contiguous(), torch.cat([sa[200:201], sa[:130]]).contiguous()   # row 200 placed at m = 0
    assert torch.equal(call_abi(moved[0], w, moved[1], sw, w_fmt, torch.float32)[0], f32[200])


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
def test_simulation_and_kernel_mode_layers_run_the_same_entries_under_the_plain_bound(path, w_fmt):
    """K = 256, N = 128, M = 130: the simulation-mode layer, the two entries called directly and HipLinearMx give the same bits; against
    the float64 product of the decoded operands the error stays inside the plain bound of K - 1 fp32 additions"""
    from viditq_extension import fused, qgemm
    from wan.quant_wanx_hip import HipLinearMx, _FpSrc

    K, N, M = 256, 128, 130
    ql, gen = _sim_layer(path, K, N, "blocks.0.ffn.0")
    wc, ws = host_quant(ql.fp_module.weight.data.cpu(), w_fmt)
    assert ql.mx == w_fmt and ql.mx_act == FP6 and ql.mx_had32 is False and ql.kind == "mx"
    assert tuple(ql._codes.shape) == (N, K // 4 * 3 if w_fmt == FP6 else K // 2)
    assert torch.equal(ql._codes.cpu(), wc) and torch.equal(ql.w_quantizer.scale_u8.cpu(), ws)
    x = torch.randn(1, M, K, generator=gen).to(torch.bfloat16).to(DEV)
    x[:, :, 9] *= 20
    out = ql(x)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, M, N)
    q, s = fused.quant_rows_mx(x[0], FP6)
    hq, hs = host_quant(x[0].float().cpu())
    assert torch.equal(q.cpu(), hq) and torch.equal(s.cpu(), hs)
    bias = ql.bias.detach().float()
    assert torch.equal(out[0], qgemm.mx6_linear(q, ql._codes, s, ql.w_quantizer.scale_u8, w_fmt, bias, torch.bfloat16))
    hl = HipLinearMx.from_quantized(ql, "blocks.0.ffn.0")
    assert hl.a_fmt == FP6 and hl.mx == w_fmt and hl.act_form == "mxfp6" and hl.mx_fmt.tolist() == [2 if w_fmt == FP6 else 1, 2]
    assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.scale_u8)
    assert torch.equal(hl(q, s, torch.bfloat16), out[0])
    src = _FpSrc(x[0])
    assert torch.equal(src.rows("mxfp6")[0], q) and src.rows("mxfp6")[0] is src.rows("mxfp6")[0]
    a64, w64 = deq64(q, s, FP6), deq64(ql._codes, ql.w_quantizer.scale_u8, w_fmt)
    assert torch.equal(w64.float(), ql.weight.data)
    y, tol = bound_case(a64.abs() @ w64.abs().T, a64 @ w64.T, ones(M), ones(N), bias, False, None, None, torch.bfloat16, K)
    err = (out[0].double() - y).abs()
    print(f"MX6 layer {w_fmt} vs the host expression: worst err / plain bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()
    fpy = ql.fp_module(x.float())
    print(f"MX6 layer {w_fmt} vs the floating-point layer (one outlier channel): rel err {rel_l2(out.float(), fpy):.3f}")


# ---- block and model level ------------------------------------------------------------------------------------------------------
@CFGS
def test_kernel_mode_model_matches_simulation_mode_and_the_checkpoint_round_trips(tmp_path, caplog, path, w_fmt):
    """The tiny 2-block model of tests/test_gpu_mx.py (dim 256, ffn 512, 2 heads of 128, 130 tokens) under each config: kernel mode against
    simulation mode under the bar of tests/test_gpu_mx4.py -- rel Frobenius error below 1e-2 and below 0.5 x (quantised vs
    floating-point model) + 5e-3.  Then quantize_and_save_weight -> hardware_forward_refactor(load_path=...) gives the output of the
    model built directly, bit for bit; the file holds codes [N, 3 K / 4] (e2m3 weights) and records the formats, and a model built
    under another pair refuses it by layer name"""
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearMx

    t = torch.tensor([700], device=DEV)
    model, fp, seq_len, ctx, lat0 = _tiny_model(qcfg.load(path))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref_fp = fp([lat0], t, [ctx], seq_len)[0].float().clone()
    sim = model([lat0], t, [ctx], seq_len)[0].float().clone()
    model.hardware_forward_refactor()
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearMx)]
    assert len(lins) == 20 and all(m.a_fmt == FP6 and m.mx == w_fmt and not m.had32 for m in lins)
    hw = model([lat0], t, [ctx], seq_len)[0].float().clone()
    assert torch.isfinite(sim).all() and torch.isfinite(hw).all()
    err, noise = rel_l2(hw, sim), rel_l2(sim, ref_fp)
    print(f"MX6 model {w_fmt}, kernel mode vs simulation mode: rel err {err:.3e}; simulation mode vs the floating-point model {noise:.3e}")
    assert noise > 0 and err < 1e-2 and err < 0.5 * noise + 5e-3

    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    assert sd["blocks.0.ffn.2.weight"].dtype == torch.uint8
    assert tuple(sd["blocks.0.ffn.2.weight"].shape) == (256, 512 // 4 * 3 if w_fmt == FP6 else 256)
    assert tuple(sd["blocks.0.ffn.2.scale_weight"].shape) == (256, 16)
    assert sd["blocks.0.ffn.2.mx_fmt"].tolist() == [2 if w_fmt == FP6 else 1, 2] and "blocks.0.ffn.2.mx_had32" not in sd
    fresh, *_ = _tiny_model(qcfg.load(path))
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=file)
    assert any("loaded 80 tensors" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, [ctx], seq_len)[0].float(), hw)
    other, *_ = _tiny_model(qcfg.load(YAML46 if w_fmt == FP6 else YAML44))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved with mx_fmt \[[12], 2\]"):
        other.hardware_forward_refactor(load_path=file)


@pytest.mark.parametrize("path", [YAML48, YAML44], ids=["w4a8", "w4a4"])
def test_an_existing_w4a8_and_w4a4_checkpoint_still_loads(tmp_path, path):
    from qdiff import config as qcfg

    t = torch.tensor([700], device=DEV)
    model, _, seq_len, ctx, lat0 = _tiny_model(qcfg.load(path))
    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    assert not any(k.endswith(".mx_fmt") for k in sd)
    hw = model.hardware_forward_refactor()([lat0], t, [ctx], seq_len)[0].float().clone()
    fresh, *_ = _tiny_model(qcfg.load(path))
    assert torch.equal(fresh.hardware_forward_refactor(load_path=file)([lat0], t, [ctx], seq_len)[0].float(), hw)
    six, *_ = _tiny_model(qcfg.load(YAML46))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved with no mx_fmt"):
        six.hardware_forward_refactor(load_path=file)
