"""CPU-only checks of the weight-only GEMM's low-rank entry (wanq_gemm_wq16_lowrank) and of what is wired to it: the symbol is in
the header and in the binding at ABI version 6; bad arguments are refused on the host with the rule in the message; the config key
`weight.low_rank` parses and is refused, by layer name and key, wherever the branch has no form; the LoRC fit (float64 SVD) has the
stated shapes, padding, determinism and error; the host forward matches its float64 definition; `set_low_rank` attaches and removes
an adapter; the integer checkpoint carries the factors.

Bounds.  The fit: with the factors rounded to the 16-bit type and multiplied in float64, ||E - B16 A16||_F must be below ||E||_F and
at most (1 + 2^-10) times the float64 SVD's tail ||(sigma_(r+1), ...)||_2 (the rounding of the factors is orthogonal noise of
relative size 2^-8 / sqrt(3) per factor on a part of norm <= ||E||: far inside the cap, which only keeps a broken fit from passing).
The host forward computes three products in the activation type T (unit roundoff u: 2^-8 for bf16, 2^-24 for fp32): x W_hat^T + bias
rounded to T, t = x A^T rounded to T, t B^T rounded to T, and their sum rounded to T.  Against the float64 value of the same
expression on the same (rounded) operands,
  |y - y64| <= u (|y0| + |lr| + |y|) + u (|t64| |B|^T) + gamma (|x| |W_hat|^T + |bias| + (|x| |A|^T) |B|^T)
with gamma the accumulation term of the products: torch accumulates 16-bit products in fp32, so gamma = K 2^-24 there and for
fp32 alike (a worst-case bound, K the longest sum)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")
HEADER = os.path.join(ROOT, "include", "wanq_hip.h")
ENTRY = "wanq_gemm_wq16_lowrank"

F16, BF16, F32 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import importlib.util

        spec = importlib.util.spec_from_file_location("wanq_build", os.path.join(PKG, "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = ctypes.CDLL(LIB)
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    getattr(lib, ENTRY).argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = ctypes.addressof(buf)
    yield ctypes.c_void_p((addr + 15) // 16 * 16), buf  # 16-byte aligned host memory: never dereferenced by a refused call


def call(lib, ptr, **kw):
    """the entry on a well-formed [8, 128] x [16, 128] problem with R = 64, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, dtype=BF16, w_bits=8, sw=ptr, zp=None, group_size=0, t=ptr, b=ptr, R=64, out=ptr, out_dtype=BF16, bias=None,
             bias_dtype=F32, gate=None, residual=None, epi=0, M=8, N=16, K=128)
    a.update(kw)
    rc = getattr(lib, ENTRY)(a["a"], a["w"], a["dtype"], a["w_bits"], a["sw"], a["zp"], a["group_size"], a["t"], a["b"], a["R"], a["out"],
                             a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"], a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_version_stays_6_and_the_symbol_is_in_header_and_binding(lib):
    from viditq_extension import _C

    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;]*)\)\s*;", text)
    assert m, "the header declares the entry"
    assert len(m.group(1).split(",")) == 21 and len(_C.PROTOTYPES[ENTRY]) == 21
    assert "int group_size" in m.group(1) and "int R" in m.group(1)


@pytest.mark.parametrize("which", ["t", "b"])
def test_null_factors_are_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: None})
    assert rc == 1 and msg == b"wanq_gemm_wq16_lowrank: t and b must be non-NULL"


@pytest.mark.parametrize("which", ["a", "w", "out", "sw"])
def test_null_operands_are_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: None})
    assert rc == 1 and ENTRY.encode() in msg and b"non-NULL" in msg


@pytest.mark.parametrize("R", [0, 32, 96, 320])
def test_rank_rule_is_refused(lib, p, R):
    rc, msg = call(lib, p[0], R=R)
    assert rc == 2 and msg == b"wanq_gemm_wq16_lowrank: R=%d must be 64, 128, 192 or 256" % R


@pytest.mark.parametrize("R", [64, 128, 192, 256])
def test_every_accepted_rank_passes_the_checks(lib, p, R):
    assert call(lib, p[0], R=R, M=0)[0] == 0


@pytest.mark.parametrize("which", ["t", "b"])
def test_misaligned_factors_are_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: ctypes.c_void_p(p[0].value + 8)})
    assert rc == 1 and msg == b"wanq_gemm_wq16_lowrank: t and b must be 16-byte aligned"


def test_group_rules_are_the_grouped_entrys(lib, p):
    for g in (32, 96, -64):
        rc, msg = call(lib, p[0], group_size=g)
        assert rc == 2 and msg == b"wanq_gemm_wq16_lowrank: group_size=%d must be a positive multiple of 64" % g
    assert call(lib, p[0], group_size=64, K=192, M=0)[0] == 0  # three groups of 64 (M = 0: nothing is launched)
    rc, msg = call(lib, p[0], group_size=128, K=192)
    assert rc == 2 and msg == b"wanq_gemm_wq16_lowrank: K=192 must be a multiple of group_size=128"
    rc, msg = call(lib, p[0], K=96)
    assert rc == 2 and msg == b"wanq_gemm_wq16_lowrank: K=96 must be a positive multiple of 64"
    rc, msg = call(lib, p[0], N=12)
    assert rc == 2 and b"N=12" in msg
    rc, msg = call(lib, p[0], w_bits=3)
    assert rc == 1 and b"w_bits=3" in msg
    rc, msg = call(lib, p[0], dtype=F32)
    assert rc == 1 and b"operand dtype 2" in msg


def test_m_zero_is_ok_and_launches_nothing(lib, p):
    assert call(lib, p[0], M=0)[0] == 0
    assert call(lib, p[0], M=0, group_size=128)[0] == 0


def test_python_refusal_names_the_rule_and_cpu_tensors_are_refused():
    from viditq_extension import qgemm

    assert qgemm.wq16_lowrank_refusal(1, 1536, 1536, None, 64) is None
    assert qgemm.wq16_lowrank_refusal(1, 1536, 1536, 0, 256) is None
    assert qgemm.wq16_lowrank_refusal(1, 8960, 1536, 128, 128) is None
    for R in (0, 32, 96, 320):
        assert f"R={R}" in qgemm.wq16_lowrank_refusal(1, 16, 64, None, R)
    assert "group_size=32" in qgemm.wq16_lowrank_refusal(1, 16, 64, 32, 64)
    assert "K=96" in qgemm.wq16_lowrank_refusal(1, 16, 96, None, 64)
    x, c = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.wq16_lowrank_linear(x, c, torch.ones(16), None, None, torch.zeros(4, 64, dtype=torch.bfloat16),
                                  torch.zeros(16, 64, dtype=torch.bfloat16))


# ---- the config key and its refusals ------------------------------------------------------------------------------------------
def _torch_weight_kernels(monkeypatch):
    """torch stand-ins for the HIP kernels of the weight quantiser (row statistics, codes + dequant, nibble packing: the equations
    of qdiff/base/base_quantizer.py), so that a layer can be built on the CPU"""
    from viditq_extension import fused, qgemm

    def row_minmax(w):
        return w.amin(dim=1), w.amax(dim=1), w.abs().amax(dim=1)

    def weight_quant(w, delta, zp, lo, hi, want_codes=True, want_dequant=True):
        q = (torch.round(w / delta[:, None]) - zp[:, None]).clamp(lo, hi)
        return q.to(torch.int8), (q + zp[:, None]) * delta[:, None]

    def pack_w4(codes, bias=8):  # (the layout is the GEMM's business; the host layers only store and unpack it)
        u = (codes.to(torch.int16) + bias).to(torch.uint8)
        return (u[:, 0::2] | (u[:, 1::2] << 4)).contiguous()

    def unpack_w4(packed, bias=8):
        lo, hi = (packed & 15).to(torch.int16) - bias, (packed >> 4).to(torch.int16) - bias
        return torch.stack([lo, hi], dim=2).reshape(packed.shape[0], -1).to(torch.int8)

    monkeypatch.setattr(fused, "row_minmax", row_minmax)
    monkeypatch.setattr(fused, "weight_quant", weight_quant)
    monkeypatch.setattr(qgemm, "pack_w4", pack_w4)
    monkeypatch.setattr(qgemm, "unpack_w4", unpack_w4)


def _layer(cfg, N, K, seed=0, cls=None, name="blocks.1.ffn.0", bias=True):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    g = torch.Generator().manual_seed(seed)
    fp = torch.nn.Linear(K, N, bias=bias)
    fp.weight.data.copy_(torch.randn(N, K, generator=g))
    if bias:
        fp.bias.data.copy_(torch.randn(N, generator=g) * 0.1)
    return (cls or QuantizedLinear)(K, N, bias, fp.weight.device, qcfg.create(cfg), fp, name), fp


def test_shipped_config_parses():
    from qdiff import config as qcfg

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "lowrank", "w4a16_g128_lr32_all_linears.yaml"))
    ref = qcfg.load(os.path.join(PKG, "quant_configs", "w4a16_g128_all_linears.yaml"))
    assert cfg.weight.low_rank == 32 and cfg.weight.group_size == 128 and cfg.weight.n_bits == 4 and cfg.weight.sym is False
    assert cfg.get("act", None) is None and cfg.remain_fp_regex == ref.remain_fp_regex
    assert {k: v for k, v in cfg.weight.items() if k != "low_rank"} == dict(ref.weight)


@pytest.mark.parametrize("case", ["act", "format", "bit list", "smooth_quant", "quarot", "viditq", "zero", "bool", "too large", "padded"])
def test_low_rank_is_refused_by_layer_name_and_key(monkeypatch, case):
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    _torch_weight_kernels(monkeypatch)
    w = {"n_bits": 4, "sym": False, "low_rank": 32}
    cfg, cls, exc, N, K = {
        "act": ({"weight": w, "act": {"n_bits": 8, "sym": True}}, None, NotImplementedError, 96, 128),
        "format": ({"weight": dict(w, n_bits=8, sym=True, format="fp8_e4m3")}, None, NotImplementedError, 96, 128),
        "bit list": ({"weight": dict(w, n_bits=[4, 8], i_bitwidth=0)}, None, NotImplementedError, 96, 128),
        "smooth_quant": ({"weight": w, "smooth_quant": {"layer_name_regex": "", "alpha": 0.5}}, SQQuantizedLinear, NotImplementedError, 96, 128),
        "quarot": ({"weight": w, "quarot": {"layer_name_regex": ""}}, QuarotQuantizedLinear, NotImplementedError, 64, 64),
        "viditq": ({"weight": w, "viditq": {"layer_name_regex": "", "alpha": 0.5}}, ViDiTQuantizedLinear, NotImplementedError, 64, 64),
        "zero": ({"weight": dict(w, low_rank=0)}, None, ValueError, 96, 128),
        "bool": ({"weight": dict(w, low_rank=True)}, None, ValueError, 96, 128),
        "too large": ({"weight": dict(w, low_rank=97)}, None, ValueError, 96, 128),
        "padded": ({"weight": dict(w, low_rank=257)}, None, ValueError, 320, 384),
    }[case]
    from qdiff.base.base_quantizer import StaticQuantizer

    def quantised(self, w):
        raise AssertionError("the layer is refused before any weight is quantised")

    monkeypatch.setattr(StaticQuantizer, "codes_and_dequant", quantised)
    with pytest.raises(exc, match=r"blocks\.1\.ffn\.0: weight\.low_rank"):
        _layer(cfg, N, K, cls=cls)


# ---- the fit ------------------------------------------------------------------------------------------------------------------
FITS = [(96, 128, 32, {"n_bits": 4, "sym": False}, torch.bfloat16), (136, 256, 32, {"n_bits": 4, "sym": False, "group_size": 64}, torch.bfloat16),
        (136, 256, 64, {"n_bits": 8, "sym": False}, torch.float16)]


@pytest.mark.parametrize("N,K,r,w,dt16", FITS, ids=["96x128 r32 W4", "136x256 r32 W4 g64", "136x256 r64 W8"])
def test_fit_shapes_padding_determinism_and_error(monkeypatch, N, K, r, w, dt16):
    _torch_weight_kernels(monkeypatch)
    ql, fp = _layer({"weight": dict(w, low_rank=r)}, N, K)
    again, _ = _layer({"weight": dict(w, low_rank=r)}, N, K)
    rp = (r + 63) // 64 * 64
    assert ql.low_rank == r and ql.lr_a.dtype == ql.lr_b.dtype == torch.float32
    assert tuple(ql.lr_a.shape) == (rp, K) and tuple(ql.lr_b.shape) == (N, rp)
    assert not ql.lr_a[r:].any() and not ql.lr_b[:, r:].any() and ql.lr_a[:r].any() and ql.lr_b[:, :r].any()
    assert torch.equal(ql.lr_a, again.lr_a) and torch.equal(ql.lr_b, again.lr_b)
    assert "lr_a" in dict(ql.named_buffers()) and "lr_b" in dict(ql.named_buffers())
    w_hat = ql.weight.data.double()
    assert not torch.equal(w_hat, fp.weight.data.double())  # weight.data stays W_hat, without the branch ...
    codes, wq = ql.int_weight.double(), ql.w_quantizer
    deq = ((codes.reshape(wq.delta.numel(), -1) + wq.zero_point.double().reshape(-1, 1)) * wq.delta.double().reshape(-1, 1)).reshape(N, K)
    assert torch.equal(w_hat, deq.float().double())           # ... the dequantised codes
    E = fp.weight.data.double() - w_hat
    a16, b16 = ql.low_rank_operands(dt16)
    assert a16.dtype == dt16 and tuple(a16.shape) == (rp, K) and tuple(b16.shape) == (N, rp)
    assert torch.equal(a16, ql.lr_a.to(dt16)) and torch.equal(b16, ql.lr_b.to(dt16))
    assert ql.low_rank_operands(dt16)[0] is a16  # cast once and kept
    left = (E - b16.double() @ a16.double()).norm().item()
    tail = torch.linalg.svdvals(E)[r:].norm().item()
    print(f"{N}x{K} r={r} {dt16}: ||E||_F {E.norm().item():.5f}  left {left:.5f}  float64 tail {tail:.5f}  left / tail {left / tail:.6f}")
    assert left < E.norm().item()
    assert left <= (1 + 2.0 ** -10) * tail
    ql.refresh()  # re-derived with the codes, to the same bits
    assert torch.equal(ql.lr_a, again.lr_a) and torch.equal(ql.lr_b, again.lr_b)


# ---- the host forward -------------------------------------------------------------------------------------------------------------
def _host_bound(x, w_hat, bias, a, b, y, dt):
    """float64 value of the host expression on these operands, and the bound of this file's docstring"""
    u = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}[dt]
    x, w_hat, bias, a, b = (t.double() for t in (x, w_hat, bias, a, b))
    y0 = x @ w_hat.T + bias
    t64 = x @ a.T
    t = t64.to(dt).double()
    lr = t @ b.T
    gamma = max(x.shape[1], a.shape[0]) * 2.0 ** -24
    tol = u * (y0.abs() + lr.abs() + (y0 + lr).abs()) + u * (t64.abs() @ b.abs().T) \
        + gamma * (x.abs() @ w_hat.abs().T + bias.abs() + (x.abs() @ a.abs().T) @ b.abs().T)
    return y0 + lr, tol


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,K,r,w,_", FITS, ids=["96x128 r32 W4", "136x256 r32 W4 g64", "136x256 r64 W8"])
def test_host_forward_matches_its_float64_definition(monkeypatch, N, K, r, w, _, dt):
    _torch_weight_kernels(monkeypatch)
    ql, fp = _layer({"weight": dict(w, low_rank=r)}, N, K)
    x = torch.randn(2, 5, K, generator=torch.Generator().manual_seed(1)).to(dt)
    y = ql(x)
    assert y.dtype == dt and tuple(y.shape) == (2, 5, N)
    a, b = ql.low_rank_operands(dt)
    w_hat, bias = ql.weight.data.to(dt), ql.bias.data.to(dt)
    assert torch.equal(y, F.linear(x, w_hat, bias) + F.linear((x @ a.t()).to(dt), b))
    y64, tol = _host_bound(x.reshape(-1, K), w_hat, bias, a, b, y, dt)
    err = (y.reshape(-1, N).double() - y64).abs()
    print(f"{N}x{K} r={r} {dt}: worst err / bound {(err / tol).max().item():.3f}")
    assert not (err > tol).any()
    plain = F.linear(x, w_hat, bias)
    assert ((plain.reshape(-1, N).double() - y64).abs() > tol).any()  # the branch is more than the bound: it is really added


def test_the_branch_moves_the_output_towards_the_fp_layer(monkeypatch):
    _torch_weight_kernels(monkeypatch)
    w = {"n_bits": 4, "sym": False}
    ql, fp = _layer({"weight": dict(w, low_rank=32)}, 96, 128)
    plain, _ = _layer({"weight": w}, 96, 128)
    x = torch.randn(64, 128, generator=torch.Generator().manual_seed(2))
    assert (ql(x) - fp(x)).norm() < (plain(x) - fp(x)).norm()


# ---- set_low_rank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lorc", [None, 32], ids=["adapter alone", "behind LoRC"])
def test_set_low_rank_attaches_and_removes_an_adapter(monkeypatch, lorc):
    _torch_weight_kernels(monkeypatch)
    N, K, r = 96, 128, 8
    w = {"n_bits": 4, "sym": False}
    ql, _ = _layer({"weight": dict(w, low_rank=lorc) if lorc else w}, N, K)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, K, generator=g)
    a, b = torch.randn(r, K, generator=g) * 0.1, torch.randn(N, r, generator=g) * 0.1
    before = ql(x).clone()
    assert ql.set_low_rank(a, b, scale=0.5) is ql
    a16, b16 = ql.low_rank_operands(torch.float32)
    r0 = lorc or 0
    assert tuple(a16.shape) == (64, K) and torch.equal(a16[r0:r0 + r], a) and torch.equal(b16[:, r0:r0 + r], b * 0.5)
    assert not a16[r0 + r:].any() and not b16[:, r0 + r:].any()
    if lorc:
        assert torch.equal(a16[:r0], ql.lr_a[:r0]) and torch.equal(b16[:, :r0], ql.lr_b[:, :r0])
    w_eff = ql.weight.data.double() + 0.5 * b.double() @ a.double() + (ql.lr_b.double() @ ql.lr_a.double() if lorc else 0.0)
    want = F.linear(x.double(), w_eff, ql.bias.data.double())
    err = (ql(x).double() - want).abs()
    tol = 2.0 ** -18 * (x.double().abs() @ w_eff.abs().T + 1.0)  # fp32 products of K = 128 and r <= 64 terms, regrouped
    assert not (err > tol).any() and not torch.equal(ql(x), before)
    ql.set_low_rank(None)
    assert torch.equal(ql(x), before)
    if not lorc:
        assert ql.low_rank_operands(torch.float32) is None and "lr_a" not in dict(ql.named_buffers())


def test_set_low_rank_refuses_a_rank_overflow_and_bad_shapes_by_name(monkeypatch):
    _torch_weight_kernels(monkeypatch)
    N, K = 320, 384
    ql, _ = _layer({"weight": {"n_bits": 8, "sym": False, "low_rank": 200}}, N, K, name="blocks.0.self_attn.o")
    ql.set_low_rank(torch.zeros(56, K), torch.zeros(N, 56))  # 256 in all: the largest the GEMM takes
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.o: set_low_rank.*rank 57.*low_rank=200.*320.*256"):
        ql.set_low_rank(torch.zeros(57, K), torch.zeros(N, 57))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.o: set_low_rank takes a \[r, 384\] and b \[320, r\]"):
        ql.set_low_rank(torch.zeros(8, K + 1), torch.zeros(N, 8))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.o: set_low_rank takes"):
        ql.set_low_rank(torch.zeros(8, K), torch.zeros(N, 9))
    w8a8, _ = _layer({"weight": {"n_bits": 8, "sym": True}, "act": {"n_bits": 8, "sym": True}}, 96, 128, name="blocks.0.self_attn.q")
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q: set_low_rank needs a plain weight-only"):
        w8a8.set_low_rank(torch.zeros(8, 128), torch.zeros(96, 8))


# ---- a layer without the key ------------------------------------------------------------------------------------------------------
def test_a_layer_without_the_key_is_todays_layer(monkeypatch):
    from qdiff.base.quant_layer import QuantizedLinear

    _torch_weight_kernels(monkeypatch)
    w = {"n_bits": 4, "sym": False, "group_size": 64}
    ql, fp = _layer({"weight": w}, 136, 256)
    assert ql.low_rank is None and ql.low_rank_operands(torch.float32) is None
    assert not any(n.startswith("lr_") for n, _ in ql.named_buffers()) and not any(k.startswith("lr_") for k in ql.state_dict())
    called = []
    monkeypatch.setattr(QuantizedLinear, "_forward_low_rank", lambda self, x: called.append(1))
    x = torch.randn(3, 256, generator=torch.Generator().manual_seed(4))
    assert torch.equal(ql(x), F.linear(x, ql.weight, ql.bias)) and not called
    with_key, _ = _layer({"weight": dict(w, low_rank=32)}, 136, 256)
    assert torch.equal(with_key.weight.data, ql.weight.data) and torch.equal(with_key.int_weight, ql.int_weight)


# ---- the checkpoint ---------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = torch.nn.ModuleList()


def _tiny_quant_model(monkeypatch, weight):
    """a QuantWanModel stand-in on the host: quantize_and_save_weight walks named_modules() and state_dict() only"""
    from qdiff import config as qcfg
    from wan.quant_wanx import QuantWanModel

    _torch_weight_kernels(monkeypatch)
    net = _Net()
    net.lin, _ = _layer({"weight": weight}, 96, 128, name="lin")
    net.q_cfg = qcfg.create({"weight": weight})
    return net, QuantWanModel.quantize_and_save_weight


def test_checkpoint_keys_on_the_host_and_the_reference_format_refusal(monkeypatch):
    net, save = _tiny_quant_model(monkeypatch, {"n_bits": 8, "sym": False, "low_rank": 32})
    sd = save(net)
    assert sorted(k for k in sd if k.startswith("lin.")) == ["lin.bias", "lin.lr_a", "lin.lr_b", "lin.scale_weight", "lin.weight", "lin.zp_weight"]
    assert sd["lin.lr_a"].dtype == sd["lin.lr_b"].dtype == torch.float32
    assert torch.equal(sd["lin.lr_a"], net.lin.lr_a) and torch.equal(sd["lin.lr_b"], net.lin.lr_b)
    assert tuple(sd["lin.lr_a"].shape) == (64, 128) and tuple(sd["lin.lr_b"].shape) == (96, 64)
    with pytest.raises(NotImplementedError, match=r"lin: the reference's int_weight\.pt format has no low-rank branch"):
        save(net, reference_format=True)
    plain, save = _tiny_quant_model(monkeypatch, {"n_bits": 8, "sym": False})
    assert not any("lr_" in k for k in save(plain))


def test_kernel_mode_layer_buffers_follow_the_key():
    from wan.quant_wanx_hip import HipLinearWq16

    m = HipLinearWq16(128, 96, True, False, 4, "lin", 64)
    assert list(m.state_dict().keys()) == ["weight", "scale_weight", "zp_weight", "zp_gemm", "bias"] and m.lr_a is None and m.lr_b is None
    assert m.sharded == ("weight",)
    m = HipLinearWq16(128, 96, True, False, 4, "lin", 64, low_rank=32, act_dtype=torch.float16)
    assert list(m.state_dict().keys()) == ["weight", "scale_weight", "zp_weight", "zp_gemm", "bias", "lr_a", "lr_b"]
    assert m.lr_a.dtype == m.lr_b.dtype == torch.float16 and tuple(m.lr_a.shape) == (64, 128) and tuple(m.lr_b.shape) == (96, 64)
    assert m.sharded == ("weight",)  # the factors are replicated under --dit_fsdp
    with pytest.raises(ValueError, match=r"lin: set_low_rank.*padded rank of 320"):
        m.set_low_rank(torch.zeros(225, 128), torch.zeros(96, 225))


def test_factors_are_handed_over_without_a_copy_and_a_cast_copy_follows_the_buffers(monkeypatch):
    """kernel mode without an adapter multiplies the buffers themselves; where a cast or an adapter needs a copy, the copy is made
    again after an in-place write or a load into lr_a / lr_b"""
    from wan.quant_wanx_hip import HipLinearWq16

    m = HipLinearWq16(128, 96, True, False, 4, "lin", 64, low_rank=32, act_dtype=torch.bfloat16)
    a16, b16 = m.low_rank_operands(torch.bfloat16)
    assert a16 is m.lr_a and b16 is m.lr_b
    m.set_low_rank(torch.ones(8, 128), torch.ones(96, 8))
    with_adapter = m.low_rank_operands(torch.bfloat16)[0]
    assert with_adapter is not m.lr_a and not with_adapter[:32].any() and with_adapter[32:40].all()
    m.load_state_dict(dict(m.state_dict(), lr_a=torch.full((64, 128), 2.0)))
    assert (m.low_rank_operands(torch.bfloat16)[0][:32] == 2).all()
    _torch_weight_kernels(monkeypatch)
    ql, _ = _layer({"weight": {"n_bits": 4, "sym": False, "low_rank": 32}}, 96, 128)
    assert ql.low_rank_operands(torch.float32)[0] is ql.lr_a
    before = ql.low_rank_operands(torch.bfloat16)[0].clone()
    ql.lr_a.mul_(2.0)
    assert torch.equal(ql.low_rank_operands(torch.bfloat16)[0], before * 2)
