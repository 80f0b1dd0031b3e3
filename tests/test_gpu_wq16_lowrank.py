"""The low-rank branch of the weight-only GEMM (csrc/gemm_wq16.hip, wanq_gemm_wq16_lowrank / qgemm.wq16_lowrank_linear) and what is
built on it: `weight.low_rank` in simulation mode, HipLinearWq16's factors, the integer checkpoint, graph replay, adapters.

  y0 = what wanq_gemm_wq16 / wanq_gemm_wq16_grouped has before GELU;  lr[m,n] = sum_r t[m,r] b[n,r];  y = epilogue(y0 + lr)

The kernel tests call through the C ABI into an output window between two guard regions that hold a NaN pattern and are checked
after every launch (as tests/test_gpu_wq16.py).  Shapes: M in {1, 130} (a ragged second M-tile), N in {8, 136} (a ragged second
N-tile), K in {64, 128} (one and two K-tiles; with groups of 64, one and two groups), R in {64, 128} (one and two low-rank tiles).

Exact probes: integer a, t in [-4, 4], integer c + zp (|c + zp| <= 255), integer b in [-8, 8], sw a power of two in [2^-9, 2^-3]:
|acc| <= 4 * 255 * 128 < 2^17 and |lr| <= 4 * 8 * 128 = 2^12 are integers, y0 is a multiple of 2^-9 below 2^14 and y0 + lr one
below 2^15: every fp32 intermediate has at most 24 significant bits, so the output must EQUAL the float64 definition (16-bit outputs:
its nearest-even rounding).  The tests assert that premise on the float64 value itself.

Bound on random data: that of tests/test_gpu_wq16.py plus the same per-product term for the branch,
  |y - y64| <= |sw| 2^-14 (|a| |c + zp|^T) + 2^-14 (|t| |b|^T) + 2^-23 |y|        for an fp32 output,
(grouped: sum_g |sw[g]| 2^-14 (|a_g| |c_g + zp_g|^T)), times 1.13 plus 3e-6 |gelu(y)| through GELU, times |gate| through
gate + residual; a 16-bit output one more unit of its type.  y64 is computed from the rounded t the kernel was given."""
import ctypes
import logging
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
DT = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
_ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}
EPI_GELU, EPI_GATE_RES = 1, 2
GUARD = 4096  # elements; the window stays 16-byte aligned in every type
GROUP = 64

MS, NS, KS, RS = (1, 130), (8, 136), (64, 128), (64, 128)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
W4S = pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
FORMS = pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])


def gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))


# ---- operands ---------------------------------------------------------------------------------------------------------
class Problem:
    """codes as the kernel reads them, sw / zp as passed ([N], grouped [K / 64, N]) and the float64 view of them:
    acc64(a) = sum_g sw[g] a_g (c_g + zp_g)^T and its absolute-value twin for the bound"""

    def __init__(self, N, K, w4, grouped, g, sw_pow2):
        from viditq_extension import qgemm

        ng = K // GROUP if grouped else 1
        if w4:
            q = torch.randint(-8, 8, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)
            self.codes = qgemm.pack_w4(q.contiguous(), bias=8)
            zp = torch.randint(0, 16, (ng, N), device=DEV, generator=g).float() - 8.0  # the W4A8 convention: zero_point - 8
            c = q.double() + 8.0
        else:
            q = torch.randint(-128, 128, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)
            self.codes = q.contiguous()
            zp = torch.randint(-127, 129, (ng, N), device=DEV, generator=g).float()
            c = q.double()
        if sw_pow2:
            sw = 2.0 ** torch.randint(-9, -2, (ng, N), device=DEV, generator=g).float()
        else:
            sw = (torch.rand(ng, N, device=DEV, generator=g) * 0.01 + 1e-3) * K ** -0.5
        self.N, self.K, self.w4, self.grouped, self.ng = N, K, w4, grouped, ng
        self.sw = sw.contiguous() if grouped else sw[0].contiguous()
        self.zp = zp.contiguous() if grouped else zp[0].contiguous()
        # [ng, N, K / ng]: the integer weight of each group, and its scale
        self.wint = c.view(N, ng, K // ng).permute(1, 0, 2) + zp.double()[:, :, None]
        self.sw64 = sw.double()

    def acc64(self, a, absolute=False):
        a = a.double().view(a.shape[0], self.ng, self.K // self.ng).permute(1, 0, 2)
        w, s = (self.wint.abs(), self.sw64.abs()) if absolute else (self.wint, self.sw64)
        return (torch.bmm(a.abs() if absolute else a, w.transpose(1, 2)) * s[:, None, :]).sum(0)


class Window:
    """an [M, N] output between two guard regions of one flat allocation, everything preset to a NaN pattern"""

    def __init__(self, M, N, dtype):
        self.M, self.N = M, N
        self.flat = torch.full((2 * GUARD + M * N,), float("nan"), dtype=dtype, device=DEV)
        self.out = self.flat[GUARD:GUARD + M * N].view(M, N)
        assert self.out.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[GUARD + self.M * self.N:]).all())


def call_abi(pb, a, tb, out_dtype, bias=None, gelu=False, gate=None, residual=None):
    """tb = (t, b): wanq_gemm_wq16_lowrank; tb = None: wanq_gemm_wq16 / wanq_gemm_wq16_grouped on the same operands.  Through the C
    ABI into a guarded window; -> the [M, N] output (guards checked).  A residual is updated in place, in the window."""
    from viditq_extension import _C

    M, K = a.shape
    win = Window(M, pb.N, out_dtype)
    if residual is not None:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    head = (a.data_ptr(), pb.codes.data_ptr(), DT[a.dtype], 4 if pb.w4 else 8, pb.sw.data_ptr(), pb.zp.data_ptr())
    tail = (win.out.data_ptr(), DT[out_dtype], None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
            None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, pb.N, K,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if tb is not None:
        t, b = tb
        assert t.is_contiguous() and b.is_contiguous() and tuple(t.shape) == (M, b.shape[1]) and b.shape[0] == pb.N
        rc = _C.lib.wanq_gemm_wq16_lowrank(*head, GROUP if pb.grouped else 0, t.data_ptr(), b.data_ptr(), t.shape[1], *tail)
    elif pb.grouped:
        rc = _C.lib.wanq_gemm_wq16_grouped(*head, GROUP, *tail)
    else:
        rc = _C.lib.wanq_gemm_wq16(*head, *tail)
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


def ints(shape, lo, hi, dtype, g):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g).to(dtype)


def assert_exact(out, y64, what):
    assert torch.equal(y64, y64.float().double()), "the probe's premise: the answer is an fp32 number"
    assert torch.equal(out.double(), y64.to(out.dtype).double()), what


# ---- A. exact probes -----------------------------------------------------------------------------------------------------
@FORMS
@W4S
@DTYPES
def test_exact_probe_equals_the_float64_definition(dtype, w4, grouped):
    g = torch.Generator(device=DEV).manual_seed(11 + 2 * w4 + grouped)
    for K in KS:
        for N in NS:
            pb = Problem(N, K, w4, grouped, g, sw_pow2=True)
            for R in RS:
                b = ints((N, R), -8, 8, dtype, g)
                for M in MS:
                    a, t = ints((M, K), -4, 4, dtype, g), ints((M, R), -4, 4, dtype, g)
                    y64 = pb.acc64(a) + t.double() @ b.double().T
                    for out_dtype in (torch.float32, dtype):
                        assert_exact(call_abi(pb, a, (t, b), out_dtype), y64, (M, N, K, R, out_dtype))


@FORMS
@W4S
@DTYPES
def test_one_hot_t_rows_return_the_b_column(dtype, w4, grouped):
    """row m of t = e_(m mod R): rows 0 .. R - 1 of the first M-tile walk every rank index of both low-rank tiles, the ragged rows
    128, 129 the first two again; b[n, r] = ((7 n + 3 r) mod 17) - 8, so the output row is y0 + b[:, m mod R] exactly -- a rank
    index that reaches another fragment slot, or another tile, returns another column (columns r and r' are equal only when
    r = r' mod 17: no swap of two 8-rank fragment slots, 32-deep steps or 64-deep tiles maps every index onto such a twin)."""
    g = torch.Generator(device=DEV).manual_seed(23 + 2 * w4 + grouped)
    M, K = 130, 128
    for N in NS:
        pb = Problem(N, K, w4, grouped, g, sw_pow2=True)
        a = ints((M, K), -4, 4, dtype, g)
        for R in RS:
            n, r = torch.arange(N, device=DEV)[:, None], torch.arange(R, device=DEV)[None, :]
            b = (((7 * n + 3 * r) % 17) - 8).to(dtype).contiguous()
            if N >= 17:
                assert len({tuple(c.tolist()) for c in b.T[:17]}) == 17
            t = torch.zeros(M, R, device=DEV, dtype=dtype)
            t[torch.arange(M), torch.arange(M) % R] = 1
            y64 = pb.acc64(a) + b.double().T[torch.arange(M, device=DEV) % R]
            assert_exact(call_abi(pb, a, (t, b), torch.float32), y64, (N, R))
            for m in (1, 65):  # one row alone: rank index m - 1 from a launch of its own
                assert_exact(call_abi(pb, a[:m].contiguous(), (t[:m].contiguous(), b), torch.float32), y64[:m], (N, R, m))


@FORMS
@W4S
@DTYPES
def test_one_hot_b_rows_return_the_t_column(dtype, w4, grouped):
    """the mirror: row n of b = e_(n mod R) (N = 136 walks every rank index, the ragged channels 128 .. 135 the first eight again),
    t[m, r] = ((7 m + 3 r) mod 17) - 8 scaled into [-4, 4] by halving: the output column is y0 + t[:, n mod R] exactly."""
    g = torch.Generator(device=DEV).manual_seed(31 + 2 * w4 + grouped)
    K = 128
    for N in NS:
        pb = Problem(N, K, w4, grouped, g, sw_pow2=True)
        for R in RS:
            b = torch.zeros(N, R, device=DEV, dtype=dtype)
            b[torch.arange(N), torch.arange(N) % R] = 1
            for M in MS:
                a = ints((M, K), -4, 4, dtype, g)
                m, r = torch.arange(M, device=DEV)[:, None], torch.arange(R, device=DEV)[None, :]
                t = ((((7 * m + 3 * r) % 17) - 8).to(torch.float32) * 0.5).to(dtype).contiguous()  # halves are exact in both types
                y64 = pb.acc64(a) + t.double()[:, torch.arange(N, device=DEV) % R]
                assert_exact(call_abi(pb, a, (t, b), torch.float32), y64, (M, N, R))


# ---- B. a zero branch changes nothing ------------------------------------------------------------------------------------
@FORMS
@W4S
@DTYPES
def test_a_zero_branch_is_bit_equal_to_the_entry_without_it(dtype, w4, grouped):
    g = torch.Generator(device=DEV).manual_seed(41 + 2 * w4 + grouped)
    M, N, K, R = 130, 136, 128, 128
    pb = Problem(N, K, w4, grouped, g, sw_pow2=False)
    a = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    rt, rb = torch.randn(M, R, device=DEV, generator=g).to(dtype), torch.randn(N, R, device=DEV, generator=g).to(dtype)
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    for out_dtype in (torch.float32, torch.bfloat16, torch.float16):
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for bs, gelu, gres in ((None, False, False), (bias, False, False), (bias.to(dtype), True, False), (None, False, True),
                               (bias, True, True)):
            kw = dict(bias=bs, gelu=gelu, gate=gate if gres else None, residual=res if gres else None)
            want = call_abi(pb, a, None, out_dtype, **kw)
            assert torch.isfinite(want).all()
            for tb in ((torch.zeros_like(rt), rb), (rt, torch.zeros_like(rb))):
                assert torch.equal(call_abi(pb, a, tb, out_dtype, **kw), want), (out_dtype, bs is not None, gelu, gres)
            assert not torch.equal(call_abi(pb, a, (rt, rb), out_dtype, **kw), want)


# ---- C. random data within the stated bound ---------------------------------------------------------------------------------
@FORMS
@W4S
@DTYPES
def test_random_data_within_the_stated_bound(dtype, w4, grouped):
    g = torch.Generator(device=DEV).manual_seed(53 + 2 * w4 + grouped)
    worst = 0.0
    for M, N, K, R in ((130, 136, 128, 128), (130, 136, 64, 64), (1, 8, 128, 64)):
        pb = Problem(N, K, w4, grouped, g, sw_pow2=False)
        a = torch.randn(M, K, device=DEV, generator=g).to(dtype)
        t = (torch.randn(M, R, device=DEV, generator=g) * 0.5).to(dtype)
        b = (torch.randn(N, R, device=DEV, generator=g) * R ** -0.5).to(dtype)
        bias = torch.randn(N, device=DEV, generator=g) * 0.1
        gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
        lr, lr_abs = t.double() @ b.double().T, t.double().abs() @ b.double().abs().T
        for out_dtype in (torch.float32, dtype):
            res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
            for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
                out = call_abi(pb, a, (t, b), out_dtype, bias, gelu, gate if gres else None, res if gres else None)
                y = pb.acc64(a) + lr
                s = 2.0 ** -14 * (pb.acc64(a, absolute=True) + lr_abs) + 2.0 ** -23 * y.abs()
                y = y + bias.double()
                if gelu:
                    s = s * 1.13 + 3e-6 * gelu64(y).abs()
                    y = gelu64(y)
                if gres:
                    y = res.double() + y * gate.double()
                    s = s * gate.double().abs()
                tol = s + y.abs() * _ULP[out_dtype] + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
                err = (out.double() - y).abs()
                ratio = (err / tol).max().item()
                worst = max(worst, ratio)
                print(f"{(M, N, K, R)} w4={w4} grouped={grouped} {dtype} -> {out_dtype} gelu={gelu} gres={gres}: worst err / bound {ratio:.3f}")
                assert not (err > tol).any(), f"{int((err > tol).sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}"
    print(f"worst err / bound {worst:.3f}")


# ---- D. determinism -----------------------------------------------------------------------------------------------------------
@FORMS
@W4S
def test_rows_are_bit_equal_in_any_launch(w4, grouped):
    g = torch.Generator(device=DEV).manual_seed(67 + 2 * w4 + grouped)
    M, N, K, R = 130, 136, 128, 128
    pb = Problem(N, K, w4, grouped, g, sw_pow2=False)
    a = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    t, b = torch.randn(M, R, device=DEV, generator=g).to(torch.bfloat16), torch.randn(N, R, device=DEV, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, generator=g)
    full = call_abi(pb, a, (t, b), torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(pb, a, (t, b), torch.bfloat16, bias, True))
    # row m, last of a launch of M = 1 + m: a SAMPLE of the rows, at the edges of the fragment blocks and of the M-tiles (first and
    # last row of the first 16-row block's wave half, last row of the first tile, both rows of the ragged second tile), not every m
    for m in (0, 1, 63, 127, 128, 129):
        part = call_abi(pb, a[:m + 1].contiguous(), (t[:m + 1].contiguous(), b), torch.bfloat16, bias, True)
        assert torch.equal(part[m], full[m]), m
    one = call_abi(pb, a[129:].contiguous(), (t[129:].contiguous(), b), torch.bfloat16, bias, True)
    assert torch.equal(one[0], full[129])  # and first of a launch of its own


def test_the_branch_sum_is_the_bf16_gemms():
    """lr is summed in wanq_gemm_bf16's order: with zero activations y0 = 0 and the fp32 output is bit-equal to fp_linear(t, b)"""
    from viditq_extension import qgemm

    g = torch.Generator(device=DEV).manual_seed(71)
    M, N, K, R = 130, 136, 64, 128
    pb = Problem(N, K, False, False, g, sw_pow2=False)
    a = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    t, b = torch.randn(M, R, device=DEV, generator=g).to(torch.bfloat16), torch.randn(N, R, device=DEV, generator=g).to(torch.bfloat16)
    assert torch.equal(call_abi(pb, a, (t, b), torch.float32), qgemm.fp_linear(t, b, out_dtype=torch.float32))


# ---- E. layers --------------------------------------------------------------------------------------------------------------------
def _ql(N, K, weight, seed=0, bias=True):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    g = torch.Generator().manual_seed(seed)
    fp = torch.nn.Linear(K, N, bias=bias)
    fp.weight.data.copy_(torch.randn(N, K, generator=g) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=g) * 0.1)
    fp = fp.to(DEV)
    return QuantizedLinear(K, N, bias, DEV, qcfg.create({"weight": weight}), fp, "lin"), fp


@pytest.mark.parametrize("weight", [{"n_bits": 4, "sym": False, "group_size": 64, "low_rank": 32}, {"n_bits": 8, "sym": False, "low_rank": 64}],
                         ids=["W4 g64 r32", "W8 r64"])
@DTYPES
def test_simulation_and_kernel_mode_layers_are_bit_equal(weight, dtype):
    """and both are the float64 definition on the layer's own codes and 16-bit factors, within the bound of C"""
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import HipLinearWq16, _to_hip_linear

    N, K, T = 136, 256, 130
    ql, fp = _ql(N, K, weight)
    x = torch.randn(1, T, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(dtype)
    hl = _to_hip_linear(ql, None, False, dtype, "hip", "lin")
    assert isinstance(hl, HipLinearWq16) and hl.lr_a.dtype == dtype and hl.low_rank == weight["low_rank"]
    sim, hw = ql(x), hl(x[0])
    assert sim.dtype == dtype and torch.equal(sim[0], hw)
    a16, b16 = ql.low_rank_operands(dtype, x.device)
    t = qgemm.fp_linear(x[0], a16)
    w_hat = ql.weight.data.double()
    y = x[0].double() @ w_hat.T + t.double() @ b16.double().T
    # (W_hat = (c + zp) sw elementwise in fp32: its own rounding, one part in 2^24 per product, is inside the 2^-14 term)
    s = 2.0 ** -14 * (x[0].double().abs() @ w_hat.abs().T + t.double().abs() @ b16.double().abs().T) + 2.0 ** -23 * y.abs()
    y = y + ql.bias.double()
    err = (hw.double() - y).abs()
    tol = s + y.abs() * _ULP[dtype] + (2.0 ** -24 if dtype == torch.float16 else 0.0)
    print(f"{weight} {dtype}: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()
    plain, _ = _ql(N, K, {k: v for k, v in weight.items() if k != "low_rank"})
    assert not torch.equal(plain(x), sim)
    assert (sim.float() - fp(x.float())).norm() < (plain(x).float() - fp(x.float())).norm()  # LoRC moves the layer towards FP
    # GELU and gate + residual stay fused in kernel mode: against the unfused tail on an fp32 output
    gate = torch.rand(N, device=DEV) * 2 - 1
    res = torch.randn(T, N, device=DEV)
    y32 = hl(x[0], torch.float32)
    fused = hl(x[0], torch.float32, gelu=True, gate=gate, residual=res.clone())
    want = res.double() + gelu64(y32.double()) * gate.double()
    assert ((fused.double() - want).abs() <= 1e-5 * (1 + want.abs())).all()


def test_an_adapter_moves_the_output_and_detaching_restores_the_bits():
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import _to_hip_linear

    N, K, T, r = 136, 256, 130, 16
    dtype = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(T, K, device=DEV, generator=g).to(dtype)
    a, b = torch.randn(r, K, device=DEV, generator=g) * K ** -0.5, torch.randn(N, r, device=DEV, generator=g) * 0.5
    for weight in ({"n_bits": 4, "sym": False, "group_size": 64}, {"n_bits": 4, "sym": False, "group_size": 64, "low_rank": 32}):
        ql, _ = _ql(N, K, weight)
        hl = _to_hip_linear(ql, None, False, dtype, "hip", "lin")
        for lin in (ql, hl):
            before = lin(x).clone()
            lin.set_low_rank(a, b, scale=2.0)
            a16, b16 = lin.low_rank_operands(dtype, x.device)
            assert tuple(a16.shape) == (64, K)
            after = lin(x)
            # the float64 definition on the layer's dequantised codes and on the factors the GEMM was given, within C's bound
            t = qgemm.fp_linear(x, a16)
            w_hat = ql.weight.data.double()
            y = x.double() @ w_hat.T + t.double() @ b16.double().T
            s = 2.0 ** -14 * (x.double().abs() @ w_hat.abs().T + t.double().abs() @ b16.double().abs().T) + 2.0 ** -23 * y.abs()
            y = y + ql.bias.double()
            err = (after.double() - y).abs()
            tol = s + y.abs() * _ULP[dtype]
            print(f"adapter on {type(lin).__name__} {weight}: worst err / bound {(err / tol).max().item():.3f}")
            assert not (err > tol).any()
            assert not torch.equal(after, before)
            r0 = weight.get("low_rank", 0)
            assert torch.equal(b16[:, r0:r0 + r], (b * 2.0).to(dtype)) and torch.equal(a16[r0:r0 + r], a.to(dtype))
            lin.set_low_rank(None)
            assert torch.equal(lin(x), before)
        with pytest.raises(ValueError, match=r"lin: set_low_rank.*above the GEMM's 256"):
            hl.set_low_rank(torch.zeros(257, K, device=DEV), torch.zeros(N, 257, device=DEV))


def test_graph_replay_of_a_layer_forward_is_bit_equal_to_eager():
    from wan.quant_wanx_hip import _to_hip_linear

    N, K, T = 136, 256, 130
    ql, _ = _ql(N, K, {"n_bits": 4, "sym": False, "group_size": 64, "low_rank": 32})
    hl = _to_hip_linear(ql, None, False, torch.bfloat16, "hip", "lin")
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(T, K, device=DEV, generator=g).to(torch.bfloat16)
    eager = hl(x).clone()
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hl(static_x)  # warm-up: the factor cache is filled outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = hl(static_x)
    x2 = torch.randn(T, K, device=DEV, generator=g).to(torch.bfloat16)
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, hl(x2)) and not torch.equal(static_y, eager)


# ---- the model: kernel mode against simulation mode, the checkpoint ---------------------------------------------------------------
def _tiny_model(config, build=True):
    from qdiff import config as qcfg
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    quant_config = qcfg.load(os.path.join(PKG, "quant_configs", config))
    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=512, ffn_dim=1024, num_heads=4, num_layers=2, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 3, 20, 18)
    seq_len = seq_len_for(shape)
    ctx = [torch.randn(24, 64, device=DEV, generator=g) * 0.1]
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, quant_config)
    model.quant_layer_refactor()
    model.set_init_done()
    if build:
        model.hardware_forward_refactor()
    return model, seq_len, ctx, lat0


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_kernel_mode_model_against_simulation_mode_and_checkpoint_round_trip(tmp_path, caplog):
    """quant_configs/lowrank/w4a16_g128_lr32_all_linears.yaml on a two-block model of tiny dims: kernel mode against simulation mode by the
    rule of tests/test_gpu_wq16.py (rel < 0.03), both differ from the config without the key, and the integer checkpoint carries
    the factors: save -> hardware_forward_refactor(load_path=...) of a fresh model is bit-equal."""
    from wan.quant_wanx_hip import HipLinearWq16

    model, seq_len, ctx, lat0 = _tiny_model("lowrank/w4a16_g128_lr32_all_linears.yaml")
    lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearWq16)]
    assert len(lins) == 20 and all(m.low_rank == 32 and tuple(m.lr_a.shape) == (64, m.in_features) and m.lr_a.dtype == torch.bfloat16
                                   and m.group_size == 128 and m.w_bits == 4 for m in lins)
    t = torch.tensor([700], device=DEV)
    hw = model([lat0], t, ctx, seq_len)[0].clone()
    assert torch.isfinite(hw).all()
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.0.lr_a"].dtype == torch.float32 and tuple(sd["blocks.0.ffn.0.lr_a"].shape) == (64, 512)
    assert tuple(sd["blocks.1.ffn.2.lr_b"].shape) == (512, 64)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q: the reference's int_weight\.pt format has no low-rank"):
        model.quantize_and_save_weight(None, reference_format=True)
    model.software_forward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        sim = model([lat0], t, ctx, seq_len)[0].float()
    plain, *_ = _tiny_model("w4a16_g128_all_linears.yaml")
    hw_plain = plain([lat0], t, ctx, seq_len)[0]
    print(f"lr32: kernel vs simulation {_rel(hw, sim):.3e}; kernel with the key vs without {_rel(hw, hw_plain):.3e}")
    assert torch.isfinite(sim).all() and _rel(hw, sim) < 0.03
    assert not torch.equal(hw, hw_plain)

    fresh, *_ = _tiny_model("lowrank/w4a16_g128_lr32_all_linears.yaml", build=False)
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=path)
    # weight, scale_weight, zp_weight, bias, lr_a and lr_b of 20 layers
    assert any("loaded 120 tensors" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, ctx, seq_len)[0], hw)
    # the loader's rules for optional buffers: missing with a buffer, present without one
    sd_missing = {k: v for k, v in sd.items() if k != "blocks.1.ffn.2.lr_b"}
    torch.save(sd_missing, str(tmp_path / "missing.pt"))
    with pytest.raises(KeyError, match=r"missing blocks\.1\.ffn\.2\.lr_b"):
        fresh.hardware_forward_refactor(load_path=str(tmp_path / "missing.pt"))
    plain_fresh, *_ = _tiny_model("w4a16_g128_all_linears.yaml", build=False)
    with pytest.raises(KeyError, match=r"blocks\.0\.self_attn\.q\.lr_a present but the model's layer has no lr_a"):
        plain_fresh.hardware_forward_refactor(load_path=path)
