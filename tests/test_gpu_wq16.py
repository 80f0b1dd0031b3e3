"""The weight-only quantised GEMM (csrc/gemm_wq16.hip, wanq_gemm_wq16 / qgemm.wq16_linear) and what is built on it: simulation
mode of a QuantizedLinear without an activation quantiser, kernel mode's HipLinearWq16, the integer checkpoint, graph replay.

The kernel tests call through the C ABI into an output window between two guard regions that hold a NaN pattern and are checked
after every launch.  Probes are exact: with integer activations in [-4, 4], integer c + zp (|c + zp| <= 255), K <= 1536 and sw a
power of two, |sum| <= 4 * 255 * 1536 < 2^24, so every fp32 intermediate is exact in any order and the output must EQUAL the float64
definition (16-bit outputs: its nearest-even rounding).

Bound on random data (the bound of tests/test_gpu_fp_gemm.py with w := c + zp, scaled by |sw[n]|):
  |y - y64| <= |sw[n]| 2^-14 (|a| |c + zp|^T)[m,n] + 2^-23 |y|   for an fp32 output,
times 1.13 plus 3e-6 |gelu(y)| through GELU, times |gate| through gate + residual; a 16-bit output one more unit of its type."""
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

MS, NS, KS = (1, 127, 129, 300), (8, 136, 264), (64, 128, 192, 1536)


def gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))


# ---- operands ---------------------------------------------------------------------------------------------------------
def make_codes(N, K, w4, g, zp_kind="asym"):
    """-> (codes as the kernel reads them, integer weight c + zp as float64 [N, K], zp fp32 [N] as passed or None)"""
    from viditq_extension import qgemm

    if w4:
        q = torch.randint(-8, 8, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)  # signed codes, stored + 8
        codes = qgemm.pack_w4(q.contiguous(), bias=8)
        zero = torch.randint(0, 16, (N,), device=DEV, generator=g).float() if zp_kind == "asym" else None  # qdiff zero point
        zp = None if zero is None else zero - 8.0                          # the W4A8 convention: zero_point - 8
        wint = (q.double() + 8.0) + (0.0 if zp is None else zp.double()[:, None])
    else:
        q = torch.randint(-128, 128, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)
        codes = q.contiguous()
        zp = torch.randint(-127, 129, (N,), device=DEV, generator=g).float() if zp_kind == "asym" else None
        wint = q.double() + (0.0 if zp is None else zp.double()[:, None])
    return codes, wint, zp


class Window:
    """an [M, N] output between two guard regions of one flat allocation, everything preset to a NaN pattern"""

    def __init__(self, M, N, dtype):
        self.M, self.N, self.dtype = M, N, dtype
        self.flat = torch.full((2 * GUARD + M * N,), float("nan"), dtype=dtype, device=DEV)
        self.out = self.flat[GUARD:GUARD + M * N].view(M, N)
        assert self.out.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[GUARD + self.M * self.N:]).all())


def call_abi(a, codes, w4, sw, zp, out_dtype, bias=None, gelu=False, gate=None, residual=None, into=None):
    """wanq_gemm_wq16 through the C ABI into a guarded window; -> the [M, N] output (guards checked)"""
    from viditq_extension import _C

    M, K = a.shape
    N = codes.shape[0]
    win = Window(M, N, out_dtype)
    if residual is not None and into == "inplace":
        win.out.copy_(residual)
        residual = win.out
    epi = (EPI_GELU if gelu else 0) | (EPI_GATE_RES if gate is not None else 0)
    rc = _C.lib.wanq_gemm_wq16(a.data_ptr(), codes.data_ptr(), DT[a.dtype], 4 if w4 else 8, sw.data_ptr(), None if zp is None else zp.data_ptr(),
                               win.out.data_ptr(), DT[out_dtype], None if bias is None else bias.data_ptr(), DT[bias.dtype] if bias is not None else 2,
                               None if gate is None else gate.data_ptr(), None if residual is None else residual.data_ptr(), epi, M, N, K,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _C.lib.wanq_last_error()
    torch.cuda.synchronize()
    assert win.guards_intact(), "a guard region next to the output was written"
    return win.out


def int_acts(M, K, dtype, g):
    return torch.randint(-4, 5, (M, K), device=DEV, generator=g).to(dtype)


# ---- 1. exact probe -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_exact_probe_equals_the_float64_definition(K, w4, dtype):
    g = torch.Generator(device=DEV).manual_seed(K + 7 * w4)
    for N in NS:
        for zp_kind in ("asym", "null"):
            codes, wint, zp = make_codes(N, K, w4, g, zp_kind)
            sw = (2.0 ** torch.randint(-9, -2, (N,), device=DEV, generator=g).float()).contiguous()
            for M in MS:
                a = int_acts(M, K, dtype, g)
                y64 = (a.double() @ wint.T) * sw.double()
                assert float(y64.abs().max()) < 2.0 ** 24
                for out_dtype in (torch.float32, dtype):
                    out = call_abi(a, codes, w4, sw, zp, out_dtype)
                    assert torch.equal(out.double(), y64.to(out_dtype).double()), (M, N, K, zp_kind, out_dtype)


# ---- 2. twin of the merged bf16 / fp16 GEMM -----------------------------------------------------------------------------
@pytest.mark.parametrize("MNK", [(300, 264, 192), (129, 136, 1536)])
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bit_equal_to_the_bf16_gemm_on_the_dequantised_integers(MNK, w4, dtype):
    from viditq_extension import qgemm

    M, N, K = MNK
    g = torch.Generator(device=DEV).manual_seed(M + w4)
    codes, wint, zp = make_codes(N, K, w4, g)
    w16 = wint.to(dtype).contiguous()
    assert torch.equal(w16.double(), wint)  # c + zp is exact in the 16-bit type
    a = (torch.randn(M, K, device=DEV, generator=g) * 2.0 ** -9).to(dtype)  # pre-activations of a few units: GELU's curved part
    ones = torch.ones(N, device=DEV)
    bias = (torch.randn(N, device=DEV, generator=g) * 3).to(dtype)
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    for out_dtype in (torch.float32, dtype):
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for b, gelu, gres in ((None, False, False), (bias, False, False), (None, True, False), (bias, True, False), (None, False, True),
                              (bias, True, True)):
            twin = qgemm.fp_linear(a, w16, b, out_dtype, gelu=gelu, gate=gate if gres else None, residual=res.clone() if gres else None)
            out = call_abi(a, codes, w4, ones, zp, out_dtype, b, gelu, gate if gres else None, res.clone() if gres else None,
                           "inplace" if gres else None)
            assert torch.equal(out, twin), (out_dtype, b is not None, gelu, gres)


# ---- 3. random data against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("MNK", [(300, 264, 192), (129, 136, 1536), (127, 8, 64)])
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_random_data_within_the_stated_bound(MNK, w4, dtype):
    M, N, K = MNK
    g = torch.Generator(device=DEV).manual_seed(N + K + w4)
    codes, wint, zp = make_codes(N, K, w4, g)
    a = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    sw = (torch.rand(N, device=DEV, generator=g) * 0.01 + 1e-3) * K ** -0.5
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    gate = torch.rand(N, device=DEV, generator=g) * 2 - 1
    for out_dtype in (torch.float32, dtype):
        res = torch.randn(M, N, device=DEV, generator=g).to(out_dtype)
        for gelu, gres in ((False, False), (True, False), (False, True), (True, True)):
            out = call_abi(a, codes, w4, sw, zp, out_dtype, bias, gelu, gate if gres else None, res.clone() if gres else None)
            y = (a.double() @ wint.T) * sw.double()
            s = (a.double().abs() @ wint.abs().T) * sw.double().abs() * 2.0 ** -14 + 2.0 ** -23 * y.abs()
            y = y + bias.double()
            if gelu:
                s = s * 1.13 + 3e-6 * gelu64(y).abs()
                y = gelu64(y)
            if gres:
                y = res.double() + y * gate.double()
                s = s * gate.double().abs()
            tol = s + y.abs() * _ULP[out_dtype] + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
            err = (out.double() - y).abs()
            print(f"{MNK} w4={w4} {dtype} -> {out_dtype} gelu={gelu} gres={gres}: worst err / bound {(err / tol).max().item():.3f}")
            assert not (err > tol).any(), f"{int((err > tol).sum())} elements out of bound; worst excess {(err - tol).max().item():.3e}"


# ---- 4. one-hot activations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_hot_rows_return_the_weight_column(w4, dtype):
    """row m of a = e_(64 + m): a whole 64-column K-tile (the second) plus the first column of the next; the output row is
    sw (c[:, k] + zp) exactly -- a transposed or mis-swizzled fragment, or a wrong nibble order, returns another column"""
    N, K, k0, M = 136, 192, 64, 65
    g = torch.Generator(device=DEV).manual_seed(5 + w4)
    codes, wint, zp = make_codes(N, K, w4, g)
    sw = (2.0 ** torch.randint(-6, 1, (N,), device=DEV, generator=g).float()).contiguous()
    a = torch.zeros(M, K, device=DEV, dtype=dtype)
    a[torch.arange(M), k0 + torch.arange(M)] = 1
    out = call_abi(a, codes, w4, sw, zp, torch.float32)
    expect = (wint[:, k0:k0 + M] * sw.double()[:, None]).T
    assert torch.equal(out.double(), expect)
    assert len({tuple(c.tolist()) for c in wint[:, k0:k0 + M].T}) == M  # the columns are pairwise different: the probe can tell them apart


# ---- 5. rows bit-equal in any launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w4", [False, True], ids=["w8", "w4"])
def test_rows_are_bit_equal_in_any_launch(w4):
    M, N, K = 300, 264, 1536
    g = torch.Generator(device=DEV).manual_seed(9)
    codes, _, zp = make_codes(N, K, w4, g)
    a = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    sw = torch.rand(N, device=DEV, generator=g) * 0.01
    bias = torch.randn(N, device=DEV, generator=g)
    full = call_abi(a, codes, w4, sw, zp, torch.bfloat16, bias, True)
    assert torch.equal(full, call_abi(a, codes, w4, sw, zp, torch.bfloat16, bias, True))
    for m, off in ((1, 0), (1, 128), (1, 299), (77, 100), (129, 171)):
        part = call_abi(a[off:off + m].contiguous(), codes, w4, sw, zp, torch.bfloat16, bias, True)
        assert torch.equal(part, full[off:off + m]), (m, off)
    gate = torch.rand(N, device=DEV, generator=g)
    r = torch.randn(M, N, device=DEV, generator=g)
    rf = call_abi(a, codes, w4, sw, zp, torch.float32, None, False, gate, r.clone(), "inplace")
    rp = call_abi(a[100:177].contiguous(), codes, w4, sw, zp, torch.float32, None, False, gate, r[100:177].clone(), "inplace")
    assert torch.equal(rp, rf[100:177])


# ---- 6. simulation mode -----------------------------------------------------------------------------------------------------
def _sim_case(bits, T, K, N, seed):
    """CPU draw and float64 reference from the oracle's static-quantiser codes; -> (w, b, x bf16, y64, tol, |fp - y64| excess)"""
    from oracle import qdiff_ref as qr

    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    x = torch.randn(1, T, K, generator=g).to(torch.bfloat16)
    delta, zp = qr.static_quant_params(w.numpy(), bits, False)
    q = qr.static_quantize(w.numpy(), delta, zp, bits, False)
    wint = torch.from_numpy(q).double() + torch.from_numpy(zp).double()[:, None]
    sw = torch.from_numpy(delta).double()
    x2 = x[0].double()
    y = (x2 @ wint.T) * sw
    tol = (x2.abs() @ wint.abs().T) * sw * 2.0 ** -14 + 2.0 ** -23 * y.abs()
    y = y + b.double()
    tol = tol + y.abs() * 2.0 ** -7  # bf16 output
    fp = x2 @ w.to(torch.bfloat16).double().T + b.double()  # what the unquantised fp_module computes, before its own rounding
    return w, b, x, y, tol, ((fp - y).abs() - 2 * tol).max().item()


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("TKN", [(33, 64, 48), (130, 192, 136)])
def test_simulation_mode_runs_the_quantised_weight(bits, TKN):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    T, K, N = TKN
    w, b, x, y, tol, fp_excess = _sim_case(bits, T, K, N, seed=3)
    assert fp_excess > 0, "the draw must separate the quantised weight from the unquantised one by more than twice the bound"
    fp = torch.nn.Linear(K, N).to(DEV)
    fp.weight.data.copy_(w)
    fp.bias.data.copy_(b)
    ql = QuantizedLinear(K, N, True, DEV, qcfg.create({"weight": {"n_bits": bits, "sym": False}}), fp)
    assert ql.a_quantizer is None and ql.w_quantizer is not None
    out = ql(x.to(DEV))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (1, T, N)
    err = (out[0].double().cpu() - y).abs()
    print(f"W{bits} [{T}, {K}] -> {N}: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        today = fp(x.to(DEV))
    assert ((today[0].double().cpu() - y).abs() > tol).any()  # the unquantised layer, which this config used to run
    ql.quant_mode = False
    assert torch.equal(ql(x.to(DEV).float()), fp(x.to(DEV).float()))


# ---- 7. kernel-mode block -----------------------------------------------------------------------------------------------------
def _make_block(dim, ffn, heads, seed):
    from wan.modules.model import WanAttentionBlock

    torch.manual_seed(seed)
    blk = WanAttentionBlock("t2v_cross_attn", dim, ffn, heads, cross_attn_norm=True)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.normal_(m.bias, std=0.05)
    blk.norm3.weight.data.uniform_(0.5, 1.5)
    blk.norm3.bias.data.normal_(std=0.1)
    for nm in (blk.self_attn.norm_q, blk.self_attn.norm_k, blk.cross_attn.norm_q, blk.cross_attn.norm_k):
        nm.weight.data.uniform_(0.5, 1.5)
    return blk


class _Lin16:
    """oracle Linear: float64 x16 @ W^T + b on the activation rounded to the block's 16-bit type"""

    def __init__(self, w64, bias, act_dtype):
        self.w, self.b, self.dt = w64.double(), bias.double(), act_dtype

    def __call__(self, x):
        return (x.to(self.dt).double() @ self.w.T + self.b).float()


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _wq_config(bits):
    from qdiff import config as qcfg

    return qcfg.create({"weight": {"n_bits": bits, "sym": False}})


def _quantise_block(blk, bits):
    from qdiff.base.quant_model import quant_layer_refactor_
    from qdiff.utils import apply_func_to_submodules

    apply_func_to_submodules(blk, torch.nn.Linear, quant_layer_refactor_, name=None, parent_module=None, quant_config=_wq_config(bits),
                             full_name=None, remain_fp_regex=None)
    return blk


@pytest.mark.parametrize("bits,act_dtype", [(8, torch.bfloat16), (4, torch.bfloat16), (8, torch.float16)])
def test_kernel_mode_block_weight_only_vs_float64_oracle(bits, act_dtype):
    from oracle import qdiff_ref as qr
    from oracle import wan_ref as wr
    from wan import ops
    from wan.quant_wanx_hip import HipLinearWq16, WanAttentionBlockWithHipKernel, _FpSrc

    dim, ffn, heads, grid, pad, lc = 256, 512, 2, (3, 6, 10), 4, 40
    blk = _make_block(dim, ffn, heads, 0)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    n_tok = grid[0] * grid[1] * grid[2]
    L = n_tok + pad
    g = torch.Generator().manual_seed(1)
    x = torch.randn(L, dim, generator=g)
    x[:, 5] *= 12.0
    x[n_tok:] = 0
    e0 = torch.randn(1, 6, dim, generator=g) * 0.3
    ctx = torch.randn(lc, dim, generator=g)
    freqs = wr.rope_freqs(dim // heads)
    norm_w = {k: sd[k + ".weight"].float() for k in ("self_attn.norm_q", "self_attn.norm_k", "cross_attn.norm_q", "cross_attn.norm_k")}
    norm3 = (sd["norm3.weight"].float(), sd["norm3.bias"].float())

    def oracle(weight_of):
        lin = {nm: _Lin16(weight_of(sd[nm + ".weight"]), sd[nm + ".bias"], act_dtype) for nm in wr.LINEARS}
        return wr.BlockRef(lin, norm_w, sd["modulation"], heads, 1e-6, norm3)(x, e0, grid, n_tok, ctx, freqs)[:n_tok]

    def w_hat(w):
        deq, _, _ = qr.static_fake_quant(w.numpy(), bits, False)
        return torch.from_numpy(deq)

    ref_fp = oracle(lambda w: w.to(act_dtype))   # the FP block holds its weights in the activation dtype
    ref_wq = oracle(w_hat)
    rope = ops.rope_table(freqs, grid, DEV)

    def run(hb):
        return hb(x.to(DEV).clone(), e0.to(DEV), rope, n_tok, _FpSrc(ctx.to(DEV), act_dtype)).float().cpu()[:n_tok]

    blk = blk.to(DEV)
    err_fp = _rel(run(WanAttentionBlockWithHipKernel.from_float(blk, None, act_dtype=act_dtype, fp_gemm="hip")), ref_fp)
    hb = WanAttentionBlockWithHipKernel.from_float(_quantise_block(blk, bits), None, act_dtype=act_dtype)
    lins = [getattr(a, l) for a in (hb.self_attn, hb.cross_attn) for l in "qkvo"] + [hb.ffn0, hb.ffn2]
    assert all(isinstance(l, HipLinearWq16) and l.w_bits == bits for l in lins)
    assert lins[0].weight.dtype == (torch.uint8 if bits == 4 else torch.int8)
    err_wq = _rel(run(hb), ref_wq)
    line = (f"weight-only block W{bits}A16 {str(act_dtype).split('.')[-1]} (dim {dim}): rel err vs its float64 oracle {err_wq:.3e}; "
            f"the FP block (fp_gemm=hip) vs its own {err_fp:.3e}; ratio {err_wq / err_fp:.2f}")
    print(line)
    assert err_wq <= 1.5 * err_fp


# ---- 8. checkpoint round trip, 10. graph replay -------------------------------------------------------------------------------
def _tiny_weight_only_model(bits, build=True):
    from wan.configs import seq_len_for
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    quant_config = _load_cfg(bits)
    torch.manual_seed(0)
    with torch.device(DEV):
        fp = WanModel(dim=512, ffn_dim=1024, num_heads=4, num_layers=2, text_dim=64, freq_dim=64).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    torch.nn.init.xavier_uniform_(fp.head.head.weight, generator=g)
    shape = (16, 3, 20, 18)
    seq_len = seq_len_for(shape)
    ctx = [torch.randn(24, 64, device=DEV, generator=g) * 0.1 for _ in range(2)]
    lat0 = torch.randn(shape, device=DEV, generator=g)
    model = QuantWanModel.from_float(fp, quant_config)
    model.quant_layer_refactor()
    model.set_init_done()
    if build:
        model.hardware_forward_refactor()
    return model, shape, seq_len, ctx, lat0, g


def _load_cfg(bits):
    from qdiff import config as qcfg

    return qcfg.load(os.path.join(PKG, "quant_configs", f"w{bits}a16_all_linears.yaml"))


@pytest.mark.parametrize("bits", [8, 4])
def test_checkpoint_round_trip_is_bit_equal(bits, tmp_path, caplog):
    from wan.quant_wanx_hip import HipLinearWq16

    model, shape, seq_len, ctx, lat0, g = _tiny_weight_only_model(bits)
    n_wo = sum(isinstance(m, HipLinearWq16) for m in model.hip_blocks.modules())
    assert n_wo == 20  # all ten Linears of both blocks
    t = torch.tensor([700], device=DEV)
    want = model([lat0], t, [ctx[0]], seq_len)[0].clone()
    assert torch.isfinite(want).all()
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    assert sd["blocks.0.ffn.0.weight"].dtype == (torch.uint8 if bits == 4 else torch.int8) and "blocks.0.ffn.0.act_premul" not in sd
    fresh, *_ = _tiny_weight_only_model(bits, build=False)
    with caplog.at_level(logging.INFO, logger="wan.quant_wanx"):
        fresh.hardware_forward_refactor(load_path=path)
    # weight, scale_weight, zp_weight and bias of 20 layers
    assert any("loaded 80 tensors" in r.getMessage() and "80 of them into weight-only layers" in r.getMessage() for r in caplog.records)
    for m in fresh.hip_blocks.modules():  # prove that the file is what the blocks compute with
        if isinstance(m, HipLinearWq16):
            assert m.weight.dtype == (torch.uint8 if bits == 4 else torch.int8)
    assert torch.equal(fresh([lat0], t, [ctx[0]], seq_len)[0], want)
    if bits == 8:  # the reference's int_weight.pt format stays W8A8 only: such a file is refused for these layers, by name
        ref_path = str(tmp_path / "ref.pt")
        model.quantize_and_save_weight(ref_path, reference_format=True)
        with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q.*W8A8 only"):
            fresh.hardware_forward_refactor(load_path=ref_path)


def test_graph_replay_of_a_weight_only_model_is_bit_equal_to_eager():
    from wan.graph import GraphedPasses

    model, shape, seq_len, ctx, lat0, g = _tiny_weight_only_model(4)
    gp = GraphedPasses(model, lat0, ctx, seq_len)
    for step in range(3):
        lat = torch.randn(shape, device=DEV, generator=g)
        t = torch.tensor([900 - 300 * step], device=DEV)
        eager = [model([lat], t, [c], seq_len)[0].clone() for c in ctx]
        outs = gp(lat, t)
        torch.cuda.synchronize()
        for e, o in zip(eager, outs):
            assert torch.isfinite(e).all() and torch.equal(e, o)


def test_transformed_layers_without_act_are_refused_by_name():
    from qdiff import config as qcfg
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from wan.quant_wanx_hip import _to_hip_linear

    fp = torch.nn.Linear(64, 64).to(DEV)
    ql = QuarotQuantizedLinear(64, 64, True, DEV, qcfg.create({"weight": {"n_bits": 8, "sym": False}, "quarot": {"layer_name_regex": ""}}), fp)
    with pytest.raises(NotImplementedError, match=r"blocks\.3\.self_attn\.q.*QuarotQuantizedLinear"):
        _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.3.self_attn.q")


# ---- 9. the entry scripts, and two ranks with sharded weights ---------------------------------------------------------------------
def _entry(script, *args, cwd):
    """one entry script in a fresh child process under its own time limit, on a truncated 1.3B backbone (2 blocks) at a tiny size"""
    import subprocess
    import sys

    cmd = [sys.executable, os.path.join(PKG, script), "--task", "t2v-1.3B", "--size", "832*480", "--frame_num", "5", "--num_layers", "2",
           "--sample_steps", "2", "--base_seed", "42", "--output_dir", str(cwd), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd, timeout=300)
    assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


def test_entry_point_chain_with_the_w4a16_config(tmp_path):
    """fp_generate -> ptq_wanx -> quant_generate with quant_configs/w4a16_all_linears.yaml: no calibration step and no calibration
    file (the config has no transform to fit), quant params of the 20 weight quantisers and of no activation quantiser, packed
    nibbles in int_weight.pt, kernel mode loads them into its weight-only layers; the latent is finite and is not the FP latent.
    Simulation mode (--hardware false) runs the same GEMM on the same codes inside the unmodified block: the bar between the two
    modes is that of tests/test_gpu_entrypoints.py (3e-2)."""
    qc = os.path.join(PKG, "quant_configs", "w4a16_all_linears.yaml")
    _entry("fp_generate.py", cwd=tmp_path)
    fp = torch.load(tmp_path / "fp_latent_0.pt", weights_only=True)
    assert fp.shape == (16, 2, 60, 104) and torch.isfinite(fp).all()
    _entry("ptq_wanx.py", "--quant_config", qc, cwd=tmp_path)
    qp = torch.load(tmp_path / "checkpoint" / "quant_params.pth", weights_only=True)
    assert sum(k.endswith("w_quantizer") for k in qp) == 20 and not any(k.endswith("a_quantizer") for k in qp)
    assert qp["blocks.0.ffn.2.w_quantizer"]["delta"].shape == (1536, 1)
    iw = torch.load(tmp_path / "checkpoint" / "int_weight.pt", weights_only=True)
    assert iw["blocks.0.ffn.0.weight"].dtype == torch.uint8 and tuple(iw["blocks.0.ffn.0.weight"].shape) == (8960, 1536 // 2)
    assert iw["blocks.1.self_attn.q.weight"].dtype == torch.uint8 and "blocks.0.ffn.0.act_premul" not in iw
    log = _entry("quant_generate.py", "--quant_config", qc, cwd=tmp_path)
    assert "loaded 80 tensors" in log and "80 of them into weight-only layers" in log
    hw = torch.load(tmp_path / "quant_latent_0.pt", weights_only=True)
    assert hw.shape == fp.shape and torch.isfinite(hw).all() and not torch.equal(hw, fp)
    _entry("quant_generate.py", "--quant_config", qc, "--hardware", "false", "--save_file", str(tmp_path / "sim.pt"), cwd=tmp_path)
    sim = torch.load(tmp_path / "sim.pt", weights_only=True)
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    print(f"w4a16: kernel-mode vs fp {rel(hw, fp):.3e}; simulation-mode vs fp {rel(sim, fp):.3e}; kernel vs simulation {rel(hw, sim):.3e}")
    assert torch.isfinite(sim).all() and not torch.equal(sim, fp) and rel(hw, sim) < 0.03


def test_two_ranks_with_sharded_weight_only_blocks_match_one_rank():
    """--dit_fsdp with weight-only blocks, by the two-rank rehearsal on one GPU (tests/sp_rehearsal_worker.py): the packed codes of
    HipLinearWq16 shard through wan/distributed/fsdp.py like every kernel-mode Linear's `weight`, and the layer reads the gathered
    view at call time -- sharded blocks under Ulysses are bit-equal to the unsharded ones, and (rows do not depend on M or on
    their place in a launch) the sequence-parallel output is bit-equal to one rank's."""
    import socket
    import subprocess
    import sys

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_CONFIG="w4a16_all_linears.yaml")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"weight-only rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    print(r.stdout[-1500:])
    assert r.stdout.count("fsdp_rel=0.000e+00") == 2, r.stdout[-2000:]
    assert r.stdout.count("sp_rel=0.000e+00") == 2, r.stdout[-2000:]
