"""CPU-only checks of the W4A4 MX Linear's low-rank branch (wanq_quant_rows_mx4_project, wanq_gemm_mx4_lowrank): header, binding and
host-side refusals; the config key on the MX pairs; the host forward; the checkpoint; kernel mode's layer.
Bound of the host forward.  y = Q(x) W_hat^T + t B^T + bias in fp32, t = round_T(round_T(x) A^T) as the host computed it, rounded once
to the output type: against float64 on the same operands |y - y64| <= (K + R) 2^-24 (sum |a w| + sum |t b| + |bias|) + u_out |y64|."""
import ctypes
import os
import re

import pytest
import torch

from test_wq16_lowrank_abi import BF16, F16, F32, HEADER, LIB, PKG, _Net, _layer, p  # noqa: F401  (p: the aligned-buffer fixture)

PROJECT, GEMM = "wanq_quant_rows_mx4_project", "wanq_gemm_mx4_lowrank"
MX4 = {"n_bits": 4, "sym": True, "format": "mxfp4_e2m1"}


@pytest.fixture(scope="module")
def lib():
    from viditq_extension import _C  # (builds the library when it is missing)

    lib = ctypes.CDLL(LIB)
    for e in (PROJECT, GEMM):
        getattr(lib, e).argtypes = _C.PROTOTYPES[e]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


def project(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=F32, q=ptr, scale=ptr, a16=ptr, dtype16=BF16, R=64, t=ptr, ldt=64, rows=8, cols=128, act=0, had32=0)
    a.update(kw)
    return getattr(lib, PROJECT)(*a.values(), None), lib.wanq_last_error()


def gemm(lib, ptr, **kw):
    a = dict(a=ptr, w=ptr, sa=ptr, sw=ptr, t=ptr, ldt=64, b=ptr, dtype16=BF16, R=64, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32,
             gate=None, residual=None, epi=0, M=8, N=16, K=128)
    a.update(kw)
    return getattr(lib, GEMM)(*a.values(), None), lib.wanq_last_error()


CALLS = pytest.mark.parametrize("call,entry", [(project, PROJECT), (gemm, GEMM)], ids=["project", "gemm"])


def test_abi_version_stays_6_and_both_symbols_are_in_header_and_binding(lib):
    from viditq_extension import _C

    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6
    with open(HEADER) as f:
        text = f.read()
    for entry, n in ((PROJECT, 14), (GEMM, 20)):
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;]*)\)\s*;", text)
        assert m and len(m.group(1).split(",")) == n and len(_C.PROTOTYPES[entry]) == n
        assert "int ldt" in m.group(1) and "int R" in m.group(1) and "int dtype16" in m.group(1)


@pytest.mark.parametrize("call,which", [(project, "x"), (project, "q"), (project, "scale"), (project, "a16"), (project, "t"),
                                        (gemm, "a"), (gemm, "w"), (gemm, "sa"), (gemm, "sw"), (gemm, "out"), (gemm, "t"), (gemm, "b")])
def test_null_operands_are_refused(lib, p, call, which):
    rc, msg = call(lib, p[0], **{which: None})
    assert rc == 1 and b"non-NULL" in msg and {"scale": b"scale_u8", "sa": b"sa_u8", "sw": b"sw_u8"}.get(which, which.encode()) in msg


@CALLS
@pytest.mark.parametrize("R,ldt,rule", [(0, 320, "R"), (32, 320, "R"), (96, 320, "R"), (320, 320, "R"), (64, 56, "ldt"), (128, 132, "ldt")])
def test_rank_and_pitch_rules_are_refused(lib, p, call, entry, R, ldt, rule):
    rc, msg = call(lib, p[0], R=R, ldt=ldt)
    want = b"R=%d must be a multiple of 64 in [64, 256]" % R if rule == "R" else b"ldt=%d must be a multiple of 8 and at least R=%d" % (ldt, R)
    assert rc == 2 and msg == entry.encode() + b": " + want


@pytest.mark.parametrize("call,which", [(project, "t"), (project, "a16"), (gemm, "t"), (gemm, "b")])
def test_misaligned_factors_are_refused(lib, p, call, which):
    rc, msg = call(lib, p[0], **{which: ctypes.c_void_p(p[0].value + 8)})
    assert rc == 1 and which.encode() in msg and b"16-byte aligned" in msg


def test_shape_and_dtype_rules_and_the_empty_launch(lib, p):
    for cols in (64, 192, 16512):
        rc, msg = project(lib, p[0], cols=cols)
        assert rc == 2 and b"cols=%d must be a multiple of 128" % cols in msg
    for call in (project, gemm):
        rc, msg = call(lib, p[0], dtype16=F32)
        assert rc == 1 and b"dtype16=2 must be BF16 or F16" in msg
        assert call(lib, p[0], dtype16=F16, R=256, ldt=264, **({"rows": 0} if call is project else {"M": 0}))[0] == 0
    rc, msg = project(lib, p[0], x_dtype=7)
    assert rc == 1 and b"bad x dtype 7" in msg


@pytest.mark.parametrize("had", [False, True], ids=["plain", "had32"])
def test_shipped_configs_parse_the_pair_takes_the_key_and_the_checkpoint_carries_the_factors(had):
    from qdiff import config as qcfg
    from wan.quant_wanx import QuantWanModel

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "lowrank", f"w4a4_mxfp4_{'had32_' if had else ''}lr32_all_linears.yaml"))
    ref = qcfg.load(os.path.join(PKG, "quant_configs", "mx", f"w4a4_mxfp4_{'had32_' if had else ''}all_linears.yaml"))
    assert cfg.weight.low_rank == 32 and {k: v for k, v in cfg.weight.items() if k != "low_rank"} == dict(ref.weight)
    assert dict(cfg.act) == dict(ref.act) and cfg.remain_fp_regex == ref.remain_fp_regex
    sections = {"weight": dict(MX4, low_rank=32), "act": MX4, **({"mx": {"block_hadamard": True}} if had else {})}
    net = _Net()
    net.lin, net.q_cfg = _layer(sections, 136, 384, name="lin")[0], qcfg.create(sections)
    ql, fp = net.lin, net.lin.fp_module
    sd = QuantWanModel.quantize_and_save_weight(net)
    assert sorted(k for k in sd if k.startswith("lin.")) == ["lin.bias", "lin.lr_a", "lin.lr_b"] + ["lin.mx_had32"] * had + ["lin.scale_weight", "lin.weight"]
    assert sd["lin.lr_a"].dtype == sd["lin.lr_b"].dtype == torch.float32 and torch.equal(sd["lin.lr_a"], ql.lr_a)
    with pytest.raises(NotImplementedError, match=r"lin: the reference's int_weight\.pt format"):
        QuantWanModel.quantize_and_save_weight(net, reference_format=True)
    plain, _ = _layer(dict(sections, weight=MX4), 136, 384)
    assert ql.low_rank == 32 and ql.mx_had32 is had and tuple(ql.lr_a.shape) == (64, 384) and tuple(ql.lr_b.shape) == (136, 64)
    assert torch.equal(ql._codes, plain._codes) and torch.equal(ql.weight.data, plain.weight.data)
    x = torch.randn(64, 384, generator=torch.Generator().manual_seed(2))
    assert (ql(x) - fp(x)).norm() < (plain(x) - fp(x)).norm()


@pytest.mark.parametrize("case", ["mxfp8 act", "mxfp6", "w4a8 mxfp4"])
def test_low_rank_is_still_refused_on_the_other_mx_pairs(case):
    w, a = {"mxfp8 act": ({"n_bits": 8, "sym": True, "format": "mxfp8_e4m3"},) * 2,
            "mxfp6": ({"n_bits": 6, "sym": True, "format": "mxfp6_e2m3fn"},) * 2,
            "w4a8 mxfp4": (MX4, {"n_bits": 8, "sym": True, "format": "mxfp8_e4m3"})}[case]
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: weight\.low_rank with an `act:` section is not supported"):
        _layer({"weight": dict(w, low_rank=32), "act": a}, 136, 384)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("had", [False, True], ids=["plain", "had32"])
def test_host_forward_matches_its_float64_definition(had, dt):
    from qdiff.base.base_quantizer import mx_decode

    N, K = 136, 384
    ql, _ = _layer({"weight": dict(MX4, low_rank=32), "act": MX4, **({"mx": {"block_hadamard": True}} if had else {})}, N, K)
    x = torch.randn(2, 5, K, generator=torch.Generator().manual_seed(1)).to(dt)
    y = ql(x)
    assert y.dtype == dt and tuple(y.shape) == (2, 5, N)
    T = dt if dt != torch.float32 else torch.bfloat16
    a16, b16 = ql.low_rank_operands(T)
    x2 = x.reshape(-1, K)
    a_q, a_s = ql.a_quantizer.codes_and_scale(x2)
    a64, w64, bias = mx_decode(a_q, a_s, "mxfp4_e2m1", torch.float64), ql.weight.data.double(), ql.bias.data.double()
    t = (x2.to(T).float() @ a16.float().t()).to(T).double()
    y64 = a64 @ w64.T + t @ b16.double().T + bias
    u_out = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt]
    tol = (K + 64) * 2.0 ** -24 * (a64.abs() @ w64.abs().T + t.abs() @ b16.double().abs().T + bias.abs()) + u_out * y64.abs()
    err = (y.reshape(-1, N).double() - y64).abs()
    assert not (err > tol).any()
    assert ((a64 @ w64.T + bias - y64).abs() > tol).any()  # the branch is more than the bound: it is really added


def test_kernel_mode_layer_buffers_follow_the_key():
    from wan.quant_wanx_hip import HipLinearMx

    m = HipLinearMx(384, 136, True, "mxfp4_e2m1", "lin", "mxfp4_e2m1")
    assert list(m.state_dict().keys()) == ["weight", "scale_weight", "bias"] and m.lr_a is None and not m.has_branch
    m = HipLinearMx(384, 136, True, "mxfp4_e2m1", "lin", "mxfp4_e2m1", True, low_rank=32, act_dtype=torch.float16)
    assert list(m.state_dict().keys()) == ["weight", "scale_weight", "bias", "mx_had32", "lr_a", "lr_b"] and m.has_branch
    assert m.lr_a.dtype == m.lr_b.dtype == torch.float16 and m.sharded == ("weight", "scale_weight")  # unchanged: the factors are replicated under --dit_fsdp
