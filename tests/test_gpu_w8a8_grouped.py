"""The group-wise int8 GEMM (csrc/gemm_i8_grouped.hip, wanq_gemm_w8a8_grouped / qgemm.w8a8_grouped_linear) and what is built on it:
simulation mode of a QuantizedLinear with `weight.group_size` and an `act:` section, kernel mode's grouped HipLinearW8A8, the integer
checkpoint, with quant_configs/w4a8_g128_all_linears.yaml.

Contract (include/wanq_hip.h):  part_g = sum_{k in group g} a[m,k] (u[n,k] + zp[g,n])  (int32);  acc = fma((float)part_g, sw[g,n], acc),
g ascending from 0;  y = fma(acc, sa[m], bias[n]);  GELU;  y = fma(y, gate[n], residual[m,n]);  one rounding.  sw, zp fp32 [K / g, N].
Expected values are computed here, in float64 (torch on the GPU for the products, which are exact integer sums below 2^53).

Exact probes: small integer activations, integer u + zp, sw and sa powers of two -- every partial sum, every fma and the result are
exactly representable in fp32 (asserted from the inputs), so any summation order gives the same bits and the output must EQUAL the
float64 evaluation.  The kernel writes into a window between two NaN guard regions (tests/test_gpu_wq16.py's Window).

Bound on random data (profiles/PARITY_NOTES.md, "Group-wise int8 GEMM"), u = 2^-24, G = K / g,
T = sa[m] sum_g |part_g| sw[g,n] + |bias[n]|:
    |y - y64| <= 1.01 (G + 1) u T                      G fmas into the accumulator and the final fma
through GELU:  1.13 e + bound (B) of PARITY_NOTES at the pre-activation (1.13 >= sup |gelu'|; tests/test_gpu_gemm_probes.py's gelu_bound);
through gate + residual:  |gate| e + u |out|            one fp32 rounding of the result;
the store:  + u_out |out|, u_out = 2^-8 (bf16), 2^-11 (fp16), 0 (fp32); fp16 below 2^-14 is spaced 2^-24 apart: + 2^-25."""
import ctypes
import logging
import os

import pytest
import torch

from test_gpu_gemm_probes import gelu_bound, gelu_ref
from test_gpu_wq16 import DEV, DT, EPI_GATE_RES, EPI_GELU, PKG, Window

pytestmark = pytest.mark.gpu
YAML = os.path.join(PKG, "quant_configs", "w4a8_g128_all_linears.yaml")
U32 = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
OUTS = (torch.float32, torch.bfloat16, torch.float16)


# ---- operands ---------------------------------------------------------------------------------------------------------
def gen_for(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def pack(u):
    """unsigned nibbles u [N, K] (0..15) -> the packed codes the kernel reads"""
    from viditq_extension import qgemm

    return qgemm.pack_w4(u.to(torch.int8).contiguous(), bias=0)


def make_w(N, K, gs, w4, gen, scales="pow2"):
    """-> (codes as the kernel reads them, wint = u + zp[g(k), n] float64 [N, K], sw fp32 [G, N], zp fp32 [G, N] or None (w8))"""
    G = K // gs
    if w4:
        u = torch.randint(0, 16, (N, K), device=DEV, generator=gen)
        zp = -torch.randint(0, 16, (G, N), device=DEV, generator=gen).float()   # u + zp in [-15, 15], as StaticQuantizer gives
        codes, wint = pack(u), u.double() + zp.double().T.repeat_interleave(gs, dim=1)
    else:
        c = torch.randint(-127, 128, (N, K), device=DEV, generator=gen)
        codes, wint, zp = c.to(torch.int8).contiguous(), c.double(), None
    if scales == "pow2":
        sw = 2.0 ** torch.randint(-3, 4, (G, N), device=DEV, generator=gen).float()
    elif scales == "odd":     # a distinct non-power-of-two per (group, channel)
        sw = (1.0 + (torch.arange(G * N, device=DEV).float().view(G, N) * 2 + 1) / 4096.0) * 0.37
    else:                     # the size of a quantised weight's steps
        sw = (torch.rand(G, N, device=DEV, generator=gen) * 0.01 + 1e-3) * K ** -0.5
    return codes, wint, sw.contiguous(), None if zp is None else zp.contiguous()


def parts64(a, wint, gs):
    """[G, M, N] float64: the exact integer partial sums"""
    a64 = a.double()
    return torch.stack([a64[:, g * gs:(g + 1) * gs] @ wint[:, g * gs:(g + 1) * gs].T for g in range(wint.shape[1] // gs)])


def call_abi(a, codes, w4, sw, zp, gs, sa, out_dtype, bias=None, gelu=False, gate=None, residual=None, inplace=False):
    """wanq_gemm_w8a8_grouped through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape
    N = codes.shape[0]
    win = Window(M, N, out_dtype)
    if residual is not None and inplace:
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_w8a8_grouped(
        a.data_ptr(), codes.data_ptr(), 4 if w4 else 8, sw.data_ptr(), None if zp is None else zp.data_ptr(), gs, win.out.data_ptr(),
        DT[out_dtype], sa.data_ptr(), DT[sa.dtype], None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
        None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


def i8(t):
    return t.to(torch.int8).contiguous()


KG = [(128, 128), (256, 128), (384, 128), (512, 256), (512, 512)]
W4S = pytest.mark.parametrize("w4", [True, False], ids=["w4", "w8"])


# ---- 1. exact probes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,gs", KG)
@W4S
def test_exact_integer_probe_equals_the_float64_contract(K, gs, w4):
    """a in [-2, 2], sw in 2^-3 .. 2^3, sa in 2^-2 .. 2^2 (fp32 and fp16 vectors): sums of multiples of 2^-5 below 2^24 units"""
    gen = gen_for(K + gs + w4)
    for N in (8, 136):
        codes, wint, sw, zp = make_w(N, K, gs, w4, gen)
        for M in (1, 127, 129, 130):
            a = torch.randint(-2, 3, (M, K), device=DEV, generator=gen)
            sa = 2.0 ** torch.randint(-2, 3, (M,), device=DEV, generator=gen).float()
            p = parts64(a, wint, gs)
            assert float((p.abs() * sw.double()[:, None, :]).sum(0).max()) * 4 * 32 < 2.0 ** 24
            y64 = (p * sw.double()[:, None, :]).sum(0) * sa.double()[:, None]
            for vec in (torch.float32, torch.float16):
                out = call_abi(i8(a), codes, w4, sw, zp, gs, sa.to(vec), torch.float32)
                assert torch.equal(out.double(), y64), (M, N, K, gs, vec)


@pytest.mark.parametrize("K,gs", KG)
@W4S
def test_one_hot_rows_pin_nibble_order_group_and_channel(K, gs, w4):
    """a[m, k0(m)] = 1: out[m, n] = fp32((u[n, k0] + zp[g(k0), n]) sw[g(k0), n]) sa[m] -- one fp32 rounding (the fold's fma onto 0), sa a
    power of two.  k0 runs over EVERY k, so each nibble position, K-tile, LDS stage and group is hit; u, zp random and sw distinct
    per (group, channel), so a value from another k, group or channel differs."""
    gen = gen_for(5 * K + gs + w4)
    for N in (8, 136):
        codes, wint, sw, zp = make_w(N, K, gs, w4, gen, "odd")
        for M in (1, 127, 129, 130):
            k_of = (torch.arange(M, device=DEV) * 37 + M) % K if M < K else torch.arange(M, device=DEV) % K
            a = torch.zeros(M, K, device=DEV, dtype=torch.int8)
            a[torch.arange(M, device=DEV), k_of] = 1
            sa = 2.0 ** torch.randint(-2, 3, (M,), device=DEV, generator=gen).float()
            out = call_abi(a, codes, w4, sw, zp, gs, sa, torch.float32)
            expect = (wint.float()[:, k_of].T * sw[k_of // gs]) * sa[:, None]
            assert torch.equal(out, expect), (M, N, K, gs)
    # all k at once (M = K rows), N = 136
    codes, wint, sw, zp = make_w(136, K, gs, w4, gen, "odd")
    out = call_abi(torch.eye(K, device=DEV, dtype=torch.int8), codes, w4, sw, zp, gs, torch.ones(K, device=DEV), torch.float32)
    assert torch.equal(out, wint.float().T * sw.repeat_interleave(gs, dim=0))


def test_borrow_isolation_between_neighbouring_nibbles():
    """nibbles 0, 15, 0, 15, ... under zp = -15 (group 0) and zp = 0 (group 1): the int8 operands must be -15, 0 | 0, 15 -- a borrow
    or carry between bytes of the per-byte add would change a neighbour"""
    N, K, gs = 8, 256, 128
    u = (torch.arange(K, device=DEV) % 2 * 15).repeat(N, 1)
    zp = torch.stack([torch.full((N,), -15.0, device=DEV), torch.zeros(N, device=DEV)]).contiguous()
    sw = torch.ones(2, N, device=DEV)
    out = call_abi(torch.eye(K, device=DEV, dtype=torch.int8), pack(u), True, sw, zp, gs, torch.ones(K, device=DEV), torch.float32)
    assert out[[0, 1, 128, 129]].tolist() == [[-15.0] * N, [0.0] * N, [0.0] * N, [15.0] * N]
    expect = torch.tensor([-15.0, 0.0] * 64 + [0.0, 15.0] * 64, device=DEV)[:, None].expand(K, N)
    assert torch.equal(out, expect)
    # every (nibble, zero point) pair of the documented range, one per channel: u + zp in [-15, 15]
    u = torch.arange(16, device=DEV).repeat_interleave(16)[:, None].expand(256, 128).contiguous()      # channel n: nibble n // 16
    zp = -(torch.arange(256, device=DEV) % 16).float()[None, :].contiguous()                            # channel n: zp -(n % 16)
    out = call_abi(torch.eye(128, device=DEV, dtype=torch.int8), pack(u), True, torch.ones(1, 256, device=DEV), zp, 128,
                   torch.ones(128, device=DEV), torch.float32)
    assert torch.equal(out, (u.float() + zp.T).T.contiguous())


@W4S
def test_no_leakage_between_groups(w4):
    """activations in group 1 only, sw of group 0 set to 2^10: group 0 contributes fma(0, 2^10, 0) = 0"""
    M, N, K, gs = 129, 136, 256, 128
    gen = gen_for(21 + w4)
    codes, wint, sw, zp = make_w(N, K, gs, w4, gen)
    sw[0] = 2.0 ** 10
    a = torch.randint(-2, 3, (M, K), device=DEV, generator=gen)
    a[:, :gs] = 0
    out = call_abi(i8(a), codes, w4, sw, zp, gs, torch.ones(M, device=DEV), torch.float32)
    assert torch.equal(out.double(), (a[:, gs:].double() @ wint[:, gs:].T) * sw[1].double())


def test_saturated_partial_sums_are_exact():
    """a = 127, u + zp = 15, (K, g) = (1024, 1024): part = 1950720 < 2^24, exact in fp32"""
    M, N, K = 130, 8, 1024
    out = call_abi(torch.full((M, K), 127, device=DEV, dtype=torch.int8), pack(torch.full((N, K), 15, device=DEV)), True,
                   torch.ones(1, N, device=DEV), torch.zeros(1, N, device=DEV), K, torch.ones(M, device=DEV), torch.float32)
    assert torch.equal(out, torch.full((M, N), 1950720.0, device=DEV))
    out = call_abi(torch.full((M, K), -127, device=DEV, dtype=torch.int8), pack(torch.zeros(N, K, device=DEV)), True,
                   torch.ones(1, N, device=DEV), torch.full((1, N), -15.0, device=DEV), K, torch.ones(M, device=DEV), torch.float32)
    assert torch.equal(out, torch.full((M, N), 1950720.0, device=DEV))


def test_w8_symmetric_codes_of_plus_and_minus_127():
    M, N, K, gs = 129, 136, 384, 128
    gen = gen_for(33)
    c = torch.randint(0, 2, (N, K), device=DEV, generator=gen) * 254 - 127
    a = torch.randint(-2, 3, (M, K), device=DEV, generator=gen)
    a[:, ::64] = 127   # and the largest activation against them, twice per K-tile
    sw = 2.0 ** torch.randint(-3, 4, (K // gs, N), device=DEV, generator=gen).float()
    out = call_abi(i8(a), i8(c), False, sw, None, gs, torch.ones(M, device=DEV), torch.float32)
    p = parts64(a, c.double(), gs)
    assert float((p.abs() * sw.double()[:, None, :]).sum(0).max()) * 8 < 2.0 ** 24   # sums of multiples of 2^-3, exact in fp32
    assert torch.equal(out.double(), (p * sw.double()[:, None, :]).sum(0))


@pytest.mark.parametrize("out_dtype", OUTS, ids=["f32", "bf16", "f16"])
@W4S
def test_bias_gate_and_residual_exactly_in_every_output_type(out_dtype, w4):
    """integer bias (fp32 and fp16 vectors), gate +-{1/2, 1, 2}, integer residual, out of place and in place: every step exact in fp32,
    so the output is the float64 value rounded once into the output type"""
    M, N, K, gs = 130, 136, 256, 128
    gen = gen_for(41 + w4)
    codes, wint, _, zp = make_w(N, K, gs, w4, gen)
    sw = 2.0 ** torch.randint(-3, 1, (K // gs, N), device=DEV, generator=gen).float()
    a = torch.randint(-1, 2, (M, K), device=DEV, generator=gen) * (torch.rand(M, K, device=DEV, generator=gen) < 0.1)
    sa = 2.0 ** torch.randint(-2, 1, (M,), device=DEV, generator=gen).float()
    bias = torch.randint(-8, 9, (N,), device=DEV, generator=gen).float()
    gate = (2.0 ** torch.randint(-1, 2, (N,), device=DEV, generator=gen).float()) * (torch.randint(0, 2, (N,), device=DEV, generator=gen) * 2 - 1)
    res = torch.randint(-16, 17, (M, N), device=DEV, generator=gen).to(out_dtype)
    y64 = (parts64(a, wint, gs) * sw.double()[:, None, :]).sum(0) * sa.double()[:, None]
    for b in (None, bias, bias.half()):
        y = y64 + (0.0 if b is None else b.double())
        assert torch.equal(y.float().double(), y)
        assert torch.equal(call_abi(i8(a), codes, w4, sw, zp, gs, sa, out_dtype, b), y.float().to(out_dtype))
        yr = res.double() + y * gate.double()
        assert torch.equal(yr.float().double(), yr)
        for inplace in (False, True):
            r = res.clone()
            out = call_abi(i8(a), codes, w4, sw, zp, gs, sa, out_dtype, b, False, gate, r, inplace)
            assert torch.equal(out, yr.float().to(out_dtype)), (b is None, inplace)
            assert torch.equal(r, res)  # the out-of-place residual is not written (in place: `r` is copied into the window)


# ---- 2. random data under the derived bound ---------------------------------------------------------------------------------
def bound_case(a, wint, sw, gs, sa, bias, gelu, gate, res, out_dtype):
    """(y64, tol) of the header's bound"""
    p = parts64(a, wint, gs)
    G = p.shape[0]
    acc = (p * sw.double()[:, None, :]).sum(0)
    T = sa.double()[:, None] * (p.abs() * sw.double()[:, None, :]).sum(0) + bias.double().abs()
    y = acc * sa.double()[:, None] + bias.double()
    e = 1.01 * (G + 1) * U32 * T
    if gelu:
        e = 1.13 * e + gelu_bound(y) * (1 + 2.0 ** -10)
        y = gelu_ref(y)
    if gate is not None:
        y = res.double() + y * gate.double()
        e = gate.double().abs() * e + U32 * y.abs()
    return y, e + U_OUT[out_dtype] * y.abs() * (1 + 2.0 ** -10) + TINY[out_dtype]


@pytest.mark.parametrize("M,N,K,gs", [(130, 136, 256, 128), (777, 264, 512, 128), (520, 1536, 1536, 128)])
@W4S
def test_random_data_and_epilogues_within_the_derived_bound(M, N, K, gs, w4):
    gen = gen_for(M + N + K + w4)
    codes, wint, sw, zp = make_w(N, K, gs, w4, gen, "real")
    a = torch.randint(-127, 128, (M, K), device=DEV, generator=gen)
    sa = torch.rand(M, device=DEV, generator=gen) * 0.02 + 1e-3
    bias = torch.randn(N, device=DEV, generator=gen) * 0.1
    gate = torch.rand(N, device=DEV, generator=gen) * 2 - 1
    worst = {}
    for out_dtype in OUTS:
        res = torch.randn(M, N, device=DEV, generator=gen).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(i8(a), codes, w4, sw, zp, gs, sa, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None,
                           inplace=gres)  # out aliases residual
            y, tol = bound_case(a, wint, sw, gs, sa, bias, gelu, gate if gres else None, res, out_dtype)
            err = (out.double() - y).abs()
            worst[(str(out_dtype)[6:], gelu, gres)] = round((err / tol).max().item(), 3)
            assert not (err > tol).any(), (out_dtype, gelu, gres, int((err > tol).sum()), (err / tol).max().item())
    print(f"w8a8_grouped {'w4' if w4 else 'w8'} ({M}, {N}, {K}, g {gs}): worst err / bound {max(worst.values()):.3f} {worst}")


@W4S
def test_repeated_calls_and_rows_in_launches_of_another_size_are_bit_equal(w4):
    M, N, K, gs = 300, 136, 512, 128
    gen = gen_for(9 + w4)
    codes, _, sw, zp = make_w(N, K, gs, w4, gen, "real")
    a = i8(torch.randint(-127, 128, (M, K), device=DEV, generator=gen))
    sa = torch.rand(M, device=DEV, generator=gen) * 0.02 + 1e-3
    bias = torch.randn(N, device=DEV, generator=gen)
    full = call_abi(a, codes, w4, sw, zp, gs, sa, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, codes, w4, sw, zp, gs, sa, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 299), (77, 100), (130, 170)):
        part = call_abi(a[off:off + m].contiguous(), codes, w4, sw, zp, gs, sa[off:off + m].contiguous(), torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)


# ---- 3. layer level ---------------------------------------------------------------------------------------------------------
def _sim_layer(gs, bits=4, sym=False, K=256, N=136):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    gen = torch.Generator().manual_seed(5)
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(torch.randn(N, K, generator=gen) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=gen) * 0.1)
    cfg = qcfg.load(YAML)
    cfg.weight.group_size, cfg.weight.n_bits, cfg.weight.sym = gs, bits, sym
    ql = QuantizedLinear(K, N, True, DEV, cfg, fp, module_name="blocks.0.ffn.0")
    x = torch.randn(1, 133, K, generator=gen).to(torch.bfloat16).to(DEV)
    return ql, x


@pytest.mark.parametrize("bits,sym", [(4, False), (8, True)])
def test_simulation_and_kernel_mode_layers_call_the_same_entry_on_the_same_operands(bits, sym):
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import HipLinearW8A8

    ql, x = _sim_layer(128, bits, sym)
    K, N, gs = 256, 136, 128
    assert ql.group_size == gs and ql.a_quantizer is not None and tuple(ql.w_quantizer.delta.shape) == (N, K // gs)
    codes, sw, zp, w4 = ql.weight_only_operands()
    assert w4 == (bits == 4) and tuple(sw.shape) == (K // gs, N) and (zp is None) == (bits == 8)
    out = ql(x)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, 133, N)
    q, s, _ = ql.a_quantizer.quantize_int8(x[0], want_sum=False)
    assert torch.equal(out[0], qgemm.w8a8_grouped_linear(q, codes, s, sw, zp, gs, ql.bias.detach().float(), torch.bfloat16, w4=w4))
    hl = HipLinearW8A8.from_quantized(ql, "blocks.0.ffn.0")
    assert hl.group_size == gs and hl.act_quantizer is None and tuple(hl.scale_weight.shape) == (K // gs, N)
    assert torch.equal(hl.weight, codes) and torch.equal(hl.scale_weight, sw) and (zp is None or torch.equal(hl.zp, zp))
    assert torch.equal(hl(q, s, None, torch.bfloat16), out[0])
    # F.linear(a_q s_a, W_hat, bias) on the layer's own dequantised weight, in float64: the header's bound, plus u T for the fp32
    # rounding of (c + zp) delta in weight.data (T here with |a| |u + zp| in place of |part|, which is no smaller)
    wint = (qgemm.unpack_w4(codes, bias=0) if w4 else codes).double() + (0.0 if zp is None else zp.double().T.repeat_interleave(gs, dim=1))
    y = (q.double() * s.double()[:, None]) @ ql.weight.data.double().T + ql.bias.double()
    Tabs = s.double()[:, None] * (parts64(q.abs(), wint.abs(), gs) * sw.double()[:, None, :]).sum(0) + ql.bias.double().abs()
    tol = (1.01 * (K // gs + 1) + 1) * U32 * Tabs + U_OUT[torch.bfloat16] * y.abs() * (1 + 2.0 ** -10)
    err = (out[0].double() - y).abs()
    print(f"grouped layer {bits} bit vs F.linear on the dequantised weight: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()


@pytest.mark.parametrize("gs,bits,sym,K", [(96, 4, False, 384), (128, 8, False, 256)])
def test_what_the_kernel_refuses_falls_back_to_the_references_expression(gs, bits, sym, K):
    ql, x = _sim_layer(gs, bits, sym, K=K)
    assert tuple(ql.w_quantizer.delta.shape) == (136, K // gs)
    want = torch.nn.functional.linear(ql.a_quantizer(x[0]).float(), ql.weight.data.float(), ql.bias.detach().float()).to(torch.bfloat16)
    assert torch.equal(ql(x)[0], want)


def test_kernel_mode_refusals_name_the_layer_and_the_key():
    from wan.quant_wanx_hip import HipLinearW8A8

    ql, _ = _sim_layer(96, K=384)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: weight\.group_size=96 has no kernel-mode form.*multiple of 128"):
        HipLinearW8A8.from_quantized(ql, "blocks.0.ffn.0")
    ql, _ = _sim_layer(128, 8, False)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: weight\.group_size=128 with 8-bit asymmetric weights \(weight\.sym"):
        HipLinearW8A8.from_quantized(ql, "blocks.0.ffn.0")
    ql, _ = _sim_layer(128)
    ql.a_quantizer.sym = False
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: weight\.group_size=128 with this `act:` section"):
        HipLinearW8A8.from_quantized(ql, "blocks.0.ffn.0")


# ---- 4. block and model level ---------------------------------------------------------------------------------------------------
def _tiny_model(cfg):
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 3, 20, 18)
    ctx = torch.randn(24, 64, device=DEV, generator=g) * 0.1
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, cfg)
    model.quant_layer_refactor()
    model.set_init_done()
    return model, seq_len_for(shape), ctx, lat0


def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_kernel_mode_matches_simulation_mode_like_the_per_channel_config_and_the_checkpoint_round_trips(tmp_path, caplog):
    """Kernel mode against simulation mode of the same config, for the new config and for the same config without `group_size` (per-
    channel W4A8), on the same weights and inputs.  The two distances come from the same rounding chain with another scale
    granularity: the grouped one may not exceed twice the per-channel one (the factor covers the G-fold longer fp32 chain).  Then
    quantize_and_save_weight -> hardware_forward_refactor(load_path=...) gives the output of the model built directly, bit for bit."""
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import HipLinearW8A8

    t = torch.tensor([700], device=DEV)
    dist, keep = {}, None
    for grouped in (True, False):
        cfg = qcfg.load(YAML)
        if not grouped:
            del cfg.weight["group_size"]
        model, seq_len, ctx, lat0 = _tiny_model(cfg)
        sim = model([lat0], t, [ctx], seq_len)[0].clone()
        model.hardware_forward_refactor()
        lins = [m for m in model.hip_blocks.modules() if isinstance(m, HipLinearW8A8)]
        assert len(lins) == 20 and all(m.group_size == (128 if grouped else None) for m in lins)
        hw = model([lat0], t, [ctx], seq_len)[0].clone()
        assert torch.isfinite(sim).all() and torch.isfinite(hw).all()
        dist[grouped] = rel_l2(hw, sim)
        if grouped:
            keep = (model, hw, seq_len, ctx, lat0)
    print(f"kernel mode vs simulation mode, rel L2: w4a8 g128 {dist[True]:.3e}, w4a8 per channel {dist[False]:.3e}")
    assert dist[True] <= 2 * dist[False]

    model, want, seq_len, ctx, lat0 = keep
    assert all(tuple(m.scale_weight.shape) == (m.in_features // 128, m.out_features) for m in model.hip_blocks.modules()
               if isinstance(m, HipLinearW8A8))
    sim_l = model.blocks[0].ffn[2]   # kernel mode took the simulation layer's parameters over, transposed
    assert torch.equal(model.hip_blocks[0].ffn2.scale_weight, sim_l.w_quantizer.delta.t())
    assert torch.equal(model.hip_blocks[0].ffn2.zp_gemm, sim_l.w_quantizer.zero_point.t() - 8.0)
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.2.weight"].dtype == torch.uint8 and tuple(sd["blocks.0.ffn.2.scale_weight"].shape) == (4, 256)
    assert tuple(sd["blocks.0.ffn.2.zp_weight"].shape) == (4, 256)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q.*weight\.group_size"):
        model.quantize_and_save_weight(None, reference_format=True)
    fresh, *_ = _tiny_model(qcfg.load(YAML))
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=path)
    assert any("loaded 80 tensors" in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh([lat0], t, [ctx], seq_len)[0], want)
    bad = dict(sd)
    bad["blocks.1.ffn.0.scale_weight"] = sd["blocks.1.ffn.0.scale_weight"][0].clone()   # a per-channel vector
    torch.save(bad, path)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0\.scale_weight is \(512,\)"):
        _tiny_model(qcfg.load(YAML))[0].hardware_forward_refactor(load_path=path)
