"""CPU-only checks of the GPTQ weight solver (qdiff/base/gptq.py, csrc/gptq.hip) and of what is wired to it: the two entries are in
the header and in the binding at ABI version 6 and the header stays pedantic C99; bad arguments are refused on the host with the
rule in the message; the host model gptq_solve_host (fp32, blocked) picks the codes of a dense textbook restatement (float64, column
by column, no blocking); gptq_prepare's dead-channel and damping handling; the shipped configs parse; every refusal carries the
layer's name; a missing Hessian is a KeyError that names the file; a GPTQ'd layer's delta / zero_point are bit-equal to the
round-to-nearest layer's."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")
HEADER = os.path.join(ROOT, "include", "wanq_hip.h")
BLOCK, PROP = "wanq_gptq_block", "wanq_gptq_propagate"


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
    getattr(lib, BLOCK).argtypes = [vp, i64, vp, i64, vp, vp, i, i, i, vp, vp, i64, i, i, i, vp]
    getattr(lib, PROP).argtypes = [vp, i64, vp, i64, vp, i64, i, i, i, vp]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096)
    yield ctypes.cast(buf, ctypes.c_void_p)  # host memory: never dereferenced by a refused call (or by N = 0)


def block(lib, ptr, **kw):
    a = dict(w=ptr, w_stride=256, u=ptr, u_stride=256, delta=ptr, zp=ptr, group_size=0, qmin=-8, qmax=7, codes=ptr, err=ptr, N=4, K=256,
             c0=0, cols=128)
    a.update(kw)
    rc = getattr(lib, BLOCK)(a["w"], a["w_stride"], a["u"], a["u_stride"], a["delta"], a["zp"], a["group_size"], a["qmin"], a["qmax"],
                             a["codes"], a["err"], a["N"], a["K"], a["c0"], a["cols"], None)
    return rc, lib.wanq_last_error()


def prop(lib, ptr, **kw):
    a = dict(w=ptr, w_stride=256, u=ptr, u_stride=256, err=ptr, N=4, K=256, c0=0, cols=128)
    a.update(kw)
    rc = getattr(lib, PROP)(a["w"], a["w_stride"], a["u"], a["u_stride"], a["err"], a["N"], a["K"], a["c0"], a["cols"], None)
    return rc, lib.wanq_last_error()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_in_header_and_binding_at_abi_6(lib):
    from viditq_extension import _C

    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6
    text = open(HEADER).read()
    for entry, n in ((BLOCK, 16), (PROP, 10)):
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"the header declares {entry}"
        assert len(m.group(1).split(",")) == n and len(_C.PROTOTYPES[entry]) == n
        assert hasattr(lib, entry)
    assert "int group_size" in re.search(BLOCK + r"\s*\(([^;]*)\)", text).group(1)


def test_header_is_still_pedantic_c99(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return wanq_gptq_propagate(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   "wanq_gptq_block(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("which", ["w", "u", "delta", "zp", "codes", "err"])
def test_block_refuses_null_pointers(lib, p, which):
    rc, msg = block(lib, p, **{which: None})
    assert rc == 1 and BLOCK.encode() in msg and b"non-NULL" in msg and which.encode() in msg


@pytest.mark.parametrize("which", ["w", "u", "err"])
def test_propagate_refuses_null_pointers(lib, p, which):
    rc, msg = prop(lib, p, **{which: None})
    assert rc == 1 and msg == b"wanq_gptq_propagate: w, u and err must be non-NULL"


@pytest.mark.parametrize("call,name", [(block, BLOCK), (prop, PROP)], ids=["block", "propagate"])
def test_shape_rules_are_refused_with_the_rule(lib, p, call, name):
    for cols in (0, -1, 129, 256):
        rc, msg = call(lib, p, cols=cols)
        assert rc == 2 and msg == b"%s: cols=%d must be 1..128" % (name.encode(), cols)
    rc, msg = call(lib, p, c0=192, cols=128)
    assert rc == 2 and msg == b"%s: c0=192 + cols=128 must not exceed K=256" % name.encode()
    rc, msg = call(lib, p, c0=-2)
    assert rc == 2 and b"c0=-2" in msg
    rc, msg = call(lib, p, w_stride=255)
    assert rc == 2 and b"w_stride=255" in msg and b"at least K=256" in msg
    rc, msg = call(lib, p, N=-1)
    assert rc == 2 and b"N=-1" in msg


def test_group_rules_are_refused_with_the_rule(lib, p):
    rc, msg = block(lib, p, group_size=96)
    assert rc == 2 and msg == b"wanq_gptq_block: group_size=96 must divide K=256"
    rc, msg = block(lib, p, group_size=-32)
    assert rc == 2 and b"group_size=-32" in msg
    # two neighbouring columns per lane: a group boundary must not fall inside a pair
    rc, msg = block(lib, p, group_size=3, K=255, w_stride=255, u_stride=255, cols=64)
    assert rc == 2 and msg == b"wanq_gptq_block: group_size=3 and c0=0 must be even (a lane's pair of columns lies in one group)"
    rc, msg = block(lib, p, group_size=32, c0=33, cols=64)
    assert rc == 2 and msg == b"wanq_gptq_block: group_size=32 and c0=33 must be even (a lane's pair of columns lies in one group)"
    rc, msg = block(lib, p, qmin=-129)
    assert rc == 1 and b"qmin=-129" in msg
    rc, msg = block(lib, p, qmin=3, qmax=2)
    assert rc == 1 and b"int8 range" in msg


def test_n_zero_is_ok_and_launches_nothing(lib, p):
    assert block(lib, p, N=0)[0] == 0 and block(lib, p, N=0, group_size=32)[0] == 0 and block(lib, p, N=0, c0=33, cols=5)[0] == 0
    assert prop(lib, p, N=0)[0] == 0


def test_python_wrappers_refuse_cpu_tensors():
    from viditq_extension import fused

    w, u = torch.zeros(4, 64), torch.eye(64)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fused.gptq_block_(w, u, torch.ones(4), torch.zeros(4), None, -8, 7, torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, 64), 0, 64)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fused.gptq_propagate_(w, u, torch.zeros(4, 32), 0, 32)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fused.gram_accumulate_(torch.zeros(64, 64), torch.zeros(3, 64, dtype=torch.bfloat16))


# ---- torch stand-ins for the quantiser's HIP kernels, so that a layer can be built on the CPU ---------------------------------
def _torch_weight_kernels(monkeypatch):
    from viditq_extension import fused, qgemm

    def row_minmax(w):
        return w.amin(dim=1), w.amax(dim=1), w.abs().amax(dim=1)

    def weight_quant(w, delta, zp, lo, hi, want_codes=True, want_dequant=True):
        q = (torch.round(w / delta[:, None]) - zp[:, None]).clamp(lo, hi)
        return q.clamp(-128, 127).to(torch.int8), (q + zp[:, None]) * delta[:, None]

    def pack_w4(codes, bias=8):
        u = (codes.to(torch.int16) + bias).to(torch.uint8)
        return (u[:, 0::2] | (u[:, 1::2] << 4)).contiguous()

    def unpack_w4(packed, bias=8):
        lo, hi = (packed & 15).to(torch.int16) - bias, (packed >> 4).to(torch.int16) - bias
        return torch.stack([lo, hi], dim=2).reshape(packed.shape[0], -1).to(torch.int8)

    monkeypatch.setattr(fused, "row_minmax", row_minmax)
    monkeypatch.setattr(fused, "weight_quant", weight_quant)
    monkeypatch.setattr(qgemm, "pack_w4", pack_w4)
    monkeypatch.setattr(qgemm, "unpack_w4", unpack_w4)


def _xavier(N, K, g):
    a = (6.0 / (N + K)) ** 0.5
    return (torch.rand(N, K, generator=g) * 2 - 1) * a


def _correlated_hessian(K, rows, g):
    """H = X^T X (float64) of mildly correlated Gaussian inputs: x = z (I + M / sqrt(K)), z and M standard normal"""
    z = torch.randn(rows, K, generator=g, dtype=torch.float64)
    x = z @ (torch.eye(K, dtype=torch.float64) + torch.randn(K, K, generator=g, dtype=torch.float64) / K ** 0.5)
    return x.T @ x


def _layer(cfg, N, K, seed=0, cls=None, name="blocks.1.ffn.0"):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    fp = torch.nn.Linear(K, N, bias=True)
    fp.weight.data.copy_(_xavier(N, K, torch.Generator().manual_seed(seed)))
    return (cls or QuantizedLinear)(K, N, True, fp.weight.device, qcfg.create(cfg), fp, name), fp


GPTQ = {"layer_name_regex": "", "damp": 0.01, "block": 128}


# ---- the host model against the textbook ------------------------------------------------------------------------------------------
def _textbook(w, U, delta, zp, group_size, qmin, qmax):
    """GPTQ as the paper states it, dense: float64, one column after the other over the whole row, no blocks, no lazy updates"""
    W, U = w.double().clone(), U.double()
    N, K = W.shape
    codes = torch.empty(N, K, dtype=torch.int8)
    for j in range(K):
        g = j // group_size if group_size else 0
        d, z = delta[:, g].double(), zp[:, g].double()
        q = torch.clamp(torch.round(W[:, j] / d) - z, qmin, qmax)
        e = (W[:, j] - (q + z) * d) / U[j, j]
        W[:, j + 1:] -= e[:, None] * U[j, j + 1:][None, :]
        codes[:, j] = q.to(torch.int8)
    return codes


@pytest.mark.parametrize("group_size", [None, 32], ids=["per channel", "g32"])
@pytest.mark.parametrize("n_bits,sym", [(4, False), (4, True), (8, False)], ids=["W4 asym", "W4 sym", "W8 asym"])
@pytest.mark.parametrize("block", [128, 16], ids=["one block", "blocks of 16"])
def test_host_model_picks_the_textbook_codes(monkeypatch, group_size, n_bits, sym, block):
    from qdiff import config as qcfg
    from qdiff.base import gptq
    from qdiff.base.base_quantizer import StaticQuantizer

    _torch_weight_kernels(monkeypatch)
    g = torch.Generator().manual_seed(1)
    N, K = 24, 64
    w = _xavier(N, K, g)
    U, w0 = gptq.gptq_prepare(_correlated_hessian(K, 256, g), w, 0.01)
    assert torch.equal(w0, w) and U.dtype == torch.float32 and torch.equal(U, torch.triu(U))
    q = StaticQuantizer(qcfg.create({"n_bits": n_bits, "sym": sym, **({"group_size": group_size} if group_size else {})}))
    codes, deq = gptq.gptq_solve_host(w, U, q, block)
    qmin, qmax = gptq.stored_range(q)
    assert (qmin, qmax) == (-(2 ** (n_bits - 1)), 2 ** (n_bits - 1) - 1)
    want = _textbook(w, U, q.delta, q.zero_point, group_size, qmin, qmax)
    assert torch.equal(codes, want)
    G = K // group_size if group_size else 1
    assert torch.equal(deq, ((codes.float().view(N, G, -1) + q.zero_point.view(N, G, 1)) * q.delta.view(N, G, 1)).view(N, K))
    rtn = torch.clamp(torch.round(w.view(N, G, -1) / q.delta.view(N, G, 1)) - q.zero_point.view(N, G, 1), qmin, qmax).view(N, K)
    assert not torch.equal(codes, rtn.to(torch.int8))                       # GPTQ moved codes ...
    assert torch.equal(gptq.gptq_solve(w, U, q, block)[0], codes)           # ... and a weight in host memory takes the host path
    Hd = torch.linalg.inv(U.double().T @ U.double())                        # the solver's own, damped Hessian: H^-1 = U^T U
    rtn_deq = ((rtn.view(N, G, -1) + q.zero_point.view(N, G, 1)) * q.delta.view(N, G, 1)).view(N, K)
    o_g, o_r = gptq.objective(w, deq, Hd), gptq.objective(w, rtn_deq, Hd)
    print(f"g={group_size} W{n_bits} sym={sym} block={block}: objective GPTQ / round-to-nearest {(o_g.sum() / o_r.sum()).item():.3f}")
    assert o_g.sum() < o_r.sum()


# ---- gptq_prepare -----------------------------------------------------------------------------------------------------------------
def test_prepare_handles_dead_channels_and_damping():
    from qdiff.base import gptq

    H = torch.tensor([[4.0, 1.0, 0.0, 0.0], [1.0, 3.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 1.0]])
    w = torch.arange(8.0).view(2, 4) + 1
    U, w0 = gptq.gptq_prepare(H, w, damp=0.5)
    assert torch.equal(w0[:, 2], torch.zeros(2)) and torch.equal(w0[:, [0, 1, 3]], w[:, [0, 1, 3]])  # the dead channel's weight is zeroed
    assert torch.equal(w, torch.arange(8.0).view(2, 4) + 1) and H[2, 2] == 0                         # the inputs are not modified
    Hd = H.double().clone()
    Hd[2, 2] = 1.0                                                   # dead: H[i, i] = 1 ...
    Hd += 0.5 * torch.diagonal(Hd).mean() * torch.eye(4, dtype=torch.float64)   # ... then damp * mean(diag H) * I, the 1 included
    assert torch.diagonal(Hd).mean().item() == pytest.approx((4 + 3 + 1 + 1) / 4 * 1.5)
    assert U.dtype == torch.float32 and torch.equal(U, torch.triu(U)) and (torch.diagonal(U) > 0).all()
    assert torch.allclose(U.double().T @ U.double(), torch.linalg.inv(Hd), rtol=1e-6, atol=1e-7)    # H^-1 = U^T U
    assert U[2, 3] == 0 and U[0, 2] == 0 and U[1, 2] == 0            # the dead channel is coupled to nothing
    U0, _ = gptq.gptq_prepare(Hd, w, damp=0.0)
    assert torch.equal(U0, U)
    with pytest.raises(ValueError, match="H must be"):
        gptq.gptq_prepare(torch.eye(3), w)


# ---- the configs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", [("w4a16_g128_gptq_all_linears", "w4a16_g128_all_linears"), ("w4a8_g128_gptq_all_linears", "w4a8_g128_all_linears")])
def test_shipped_configs_parse(name, base):
    from qdiff import config as qcfg

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "gptq", name + ".yaml"))
    ref = qcfg.load(os.path.join(PKG, "quant_configs", base + ".yaml"))
    assert dict(cfg.gptq) == {"layer_name_regex": "", "damp": 0.01, "block": 128}
    assert dict(cfg.weight) == dict(ref.weight) and cfg.get("act", None) == ref.get("act", None)
    assert cfg.remain_fp_regex == ref.remain_fp_regex and cfg.calib_data.hessian_path.endswith(".pth")


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["viditq", "smooth_quant", "quarot", "fp8", "mxfp8", "mxfp4", "bit list", "no weight", "block", "damp"])
def test_gptq_is_refused_by_layer_name(monkeypatch, case):
    from qdiff.base.base_quantizer import StaticQuantizer
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    _torch_weight_kernels(monkeypatch)
    w, a8 = {"n_bits": 4, "sym": False}, {"n_bits": 8, "sym": True}
    cfg, cls, exc = {
        "viditq": ({"weight": w, "act": a8, "viditq": {"layer_name_regex": "", "alpha": 0.5}, "gptq": GPTQ}, ViDiTQuantizedLinear, NotImplementedError),
        "smooth_quant": ({"weight": w, "act": a8, "smooth_quant": {"layer_name_regex": "", "alpha": 0.5}, "gptq": GPTQ}, SQQuantizedLinear, NotImplementedError),
        "quarot": ({"weight": w, "act": a8, "quarot": {"layer_name_regex": ""}, "gptq": GPTQ}, QuarotQuantizedLinear, NotImplementedError),
        "fp8": ({"weight": dict(n_bits=8, sym=True, format="fp8_e4m3"), "act": dict(a8, format="fp8_e4m3"), "gptq": GPTQ}, None, NotImplementedError),
        "mxfp8": ({"weight": dict(n_bits=8, sym=True, format="mxfp8_e4m3"), "act": dict(a8, format="mxfp8_e4m3"), "gptq": GPTQ}, None, NotImplementedError),
        "mxfp4": ({"weight": dict(n_bits=4, sym=True, format="mxfp4_e2m1"), "act": dict(a8, format="mxfp8_e4m3"), "gptq": GPTQ}, None, NotImplementedError),
        "bit list": ({"weight": dict(w, n_bits=[4, 8], i_bitwidth=0), "gptq": GPTQ}, None, NotImplementedError),
        "no weight": ({"act": a8, "gptq": GPTQ}, None, NotImplementedError),
        "block": ({"weight": w, "gptq": dict(GPTQ, block=256)}, None, ValueError),
        "damp": ({"weight": w, "gptq": dict(GPTQ, damp=-1.0)}, None, ValueError),
    }[case]

    def quantised(self, w):
        raise AssertionError("the layer is refused before any weight is quantised")

    monkeypatch.setattr(StaticQuantizer, "codes_and_dequant", quantised)
    with pytest.raises(exc, match=r"blocks\.1\.ffn\.0: gptq"):
        _layer(cfg, 64, 64, cls=cls)


def test_a_layer_the_regex_does_not_name_is_todays_layer(monkeypatch):
    _torch_weight_kernels(monkeypatch)
    w = {"n_bits": 4, "sym": False, "group_size": 32}
    ql, _ = _layer({"weight": w, "gptq": dict(GPTQ, layer_name_regex=r"self_attn")}, 24, 64)
    plain, _ = _layer({"weight": w}, 24, 64)
    assert ql.gptq is None and plain.gptq is None
    assert torch.equal(ql.int_weight, plain.int_weight) and torch.equal(ql.weight.data, plain.weight.data)
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: requantize_gptq_ needs a `gptq:` section"):
        ql.requantize_gptq_(torch.eye(64))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = torch.nn.ModuleList()


def test_reference_format_refuses_a_gptq_layer_by_name(monkeypatch):
    from qdiff import config as qcfg
    from wan.quant_wanx import QuantWanModel

    _torch_weight_kernels(monkeypatch)
    cfg = {"weight": {"n_bits": 8, "sym": False}, "gptq": GPTQ}
    net = _Net()
    net.lin, _ = _layer(cfg, 24, 64, name="lin")
    net.q_cfg = qcfg.create(cfg)
    with pytest.raises(NotImplementedError, match=r"lin: the reference's int_weight\.pt format derives its codes"):
        QuantWanModel.quantize_and_save_weight(net, reference_format=True)
    sd = QuantWanModel.quantize_and_save_weight(net)
    assert sorted(k for k in sd if k.startswith("lin.")) == ["lin.bias", "lin.scale_weight", "lin.weight", "lin.zp_weight"]


def test_a_missing_hessian_is_a_keyerror_that_names_layer_and_file(monkeypatch):
    from qdiff import config as qcfg
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    cfg = {"weight": {"n_bits": 4, "sym": False}, "gptq": GPTQ}
    net = _Net()
    net.lin, _ = _layer(cfg, 24, 64, name="lin")
    net.other, _ = _layer(cfg, 24, 64, name="other")
    H = _correlated_hessian(64, 128, torch.Generator().manual_seed(3)).float()
    with pytest.raises(KeyError, match=r"other: no Hessian for this layer in /data/hessian\.pth"):
        gptq.requantize_model_(net, qcfg.create(cfg), {"lin": H}, "/data/hessian.pth")
    assert gptq.requantize_model_(net, qcfg.create(cfg), {"lin": H, "other": H}, "/data/hessian.pth") == 2
    with pytest.raises(ValueError, match=r"lin: the Hessian is \(32, 32\)"):
        net.lin.requantize_gptq_(torch.eye(32))


# ---- the layer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [{"n_bits": 4, "sym": False, "group_size": 32}, {"n_bits": 4, "sym": True}, {"n_bits": 8, "sym": False},
                               {"n_bits": 4, "sym": False, "group_size": 32, "low_rank": 8}], ids=["W4 g32", "W4 sym", "W8", "W4 g32 + LoRC"])
def test_a_gptq_layer_keeps_the_round_to_nearest_grid_and_lowers_the_objective(monkeypatch, w):
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    N, K = 40, 128
    ql, fp = _layer({"weight": w, "gptq": GPTQ}, N, K)
    rtn, _ = _layer({"weight": w}, N, K)
    assert torch.equal(ql.int_weight, rtn.int_weight)  # until the solver runs the layer is the round-to-nearest one
    H = _correlated_hessian(K, 512, torch.Generator().manual_seed(5)).float()
    assert ql.requantize_gptq_(H) is ql
    for a, b in ((ql.w_quantizer.delta, rtn.w_quantizer.delta), (ql.w_quantizer.zero_point, rtn.w_quantizer.zero_point)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))  # bit-equal
    assert not torch.equal(ql.int_weight, rtn.int_weight)
    wq, G = ql.w_quantizer, ql.w_quantizer.delta.numel() // N
    deq = ((ql.int_weight.float().view(N, G, -1) + wq.zero_point.view(N, G, 1)) * wq.delta.view(N, G, 1)).view(N, K)
    assert torch.equal(ql.weight.data, deq)            # weight.data is what the stored codes dequantise to
    o_g, o_r = gptq.objective(fp.weight.data, ql.weight.data, H), gptq.objective(fp.weight.data, rtn.weight.data, H)
    print(f"{w}: layer objective GPTQ / round-to-nearest {(o_g.sum() / o_r.sum()).item():.3f}, rows improved {(o_g < o_r).sum().item()} of {N}")
    assert o_g.sum() < o_r.sum()
    if "low_rank" in w:  # the LoRC branch is fitted on GPTQ's residual
        E = fp.weight.data.double() - ql.weight.data.double()
        left = (E - ql.lr_b.double() @ ql.lr_a.double()).norm()
        assert left < E.norm() and not torch.equal(ql.lr_a, rtn.lr_a)
    again, _ = _layer({"weight": w, "gptq": GPTQ}, N, K)
    again.set_codes_(ql._codes.clone())                # what simulation mode does with a GPTQ checkpoint's codes
    assert torch.equal(again.int_weight, ql.int_weight) and torch.equal(again.weight.data, ql.weight.data)
    ql.refresh()                                       # (re-deriving from the FP weight is round-to-nearest again)
    assert torch.equal(ql.int_weight, rtn.int_weight)
