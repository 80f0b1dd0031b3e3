"""CPU-only checks of the weight-only GEMM entry (wanq_gemm_wq16) and of what is wired to it: bad arguments are refused on the host
with a return code and a message naming the rule, before anything is launched; the Python wrapper refuses tensors that are not on
the GPU; the two weight-only configs parse, and a QuantizedLinear built from such a config has a weight quantiser and no activation
quantiser."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")

F16, BF16, F32 = 0, 1, 2
EPI_GELU, EPI_GATE_RES = 1, 2


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
    lib.wanq_gemm_wq16.argtypes = [vp, vp, i, i, vp, vp, vp, i, vp, i, vp, vp, i, i64, i, i, vp]
    lib.wanq_gemm_bf16.argtypes = [vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = ctypes.addressof(buf)
    yield ctypes.c_void_p((addr + 15) // 16 * 16), buf  # 16-byte aligned host memory: never dereferenced by a refused call


def call(lib, ptr, **kw):
    """wanq_gemm_wq16 on a well-formed [8, 64] x [16, 64] problem, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, dtype=BF16, w_bits=8, sw=ptr, zp=None, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None,
             residual=None, epi=0, M=8, N=16, K=64)
    a.update(kw)
    rc = lib.wanq_gemm_wq16(a["a"], a["w"], a["dtype"], a["w_bits"], a["sw"], a["zp"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"],
                            a["gate"], a["residual"], a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def call_bf16(lib, ptr, **kw):
    """wanq_gemm_bf16 on the same well-formed problem (no w_bits / sw / zp), with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, dtype=BF16, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0, M=8, N=16, K=64)
    a.update(kw)
    rc = lib.wanq_gemm_bf16(a["a"], a["w"], a["dtype"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"],
                            a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def test_abi_version_stays_6(lib):
    assert lib.wanq_abi_version() == 6


@pytest.mark.parametrize("which", ["a", "w", "out", "sw"])
def test_null_operands_are_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: None})
    assert rc == 1 and b"wanq_gemm_wq16" in msg and b"non-NULL" in msg


def test_operand_dtype_is_refused(lib, p):
    rc, msg = call(lib, p[0], dtype=F32)
    assert rc == 1 and b"operand dtype 2" in msg


@pytest.mark.parametrize("bits", [0, 2, 3, 16])
def test_w_bits_is_refused(lib, p, bits):
    rc, msg = call(lib, p[0], w_bits=bits)
    assert rc == 1 and b"w_bits=%d" % bits in msg and b"4 or 8" in msg


def test_out_and_bias_dtype_are_refused(lib, p):
    rc, msg = call(lib, p[0], out_dtype=3)
    assert rc == 1 and b"out dtype 3" in msg
    rc, msg = call(lib, p[0], bias=p[0], bias_dtype=4)
    assert rc == 1 and b"bias dtype 4" in msg


def test_epilogue_flags_are_refused(lib, p):
    rc, msg = call(lib, p[0], epi=4)
    assert rc == 1 and b"unknown epilogue flag" in msg
    rc, msg = call(lib, p[0], out_dtype=F32, gate=p[0], epi=EPI_GATE_RES)
    assert rc == 1 and b"needs gate and residual" in msg
    rc, msg = call(lib, p[0], out_dtype=F32, residual=p[0], epi=EPI_GATE_RES | EPI_GELU)
    assert rc == 1 and b"needs gate and residual" in msg


def test_shape_rules_are_refused_with_the_rule(lib, p):
    rc, msg = call(lib, p[0], N=12)
    assert rc == 2 and b"N=12" in msg and b"multiple of 8" in msg
    for K in (32, 96, 0):  # K % 32 == 0 is not enough here: whole 64-deep K-tiles only
        rc, msg = call(lib, p[0], K=K)
        assert rc == 2 and b"K=%d" % K in msg and b"multiple of 64" in msg
    rc, msg = call(lib, p[0], M=-1)
    assert rc == 2 and b"M=-1" in msg
    rc, msg = call(lib, p[0], M=2 ** 31)
    assert rc == 2 and b"out of range" in msg


@pytest.mark.parametrize("which", ["a", "w", "out", "sw", "zp", "residual"])
def test_misaligned_operands_are_refused(lib, p, which):
    off = ctypes.c_void_p(p[0].value + 8)
    rc, msg = call(lib, p[0], **{which: off})
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = call(lib, p[0], bias=ctypes.c_void_p(p[0].value + 4), bias_dtype=BF16)
    assert rc == 1 and b"aligned to 4 elements" in msg


@pytest.mark.parametrize("rule", ["operand dtype", "out dtype", "bias dtype", "unknown flag", "gate without residual", "N=12",
                                  "misaligned out"])
def test_common_rules_refuse_alike_in_both_16bit_entries(lib, p, rule):
    """One invalid argument set per rule the two entries share (csrc/gemm16_common.h): the same return code from wanq_gemm_bf16 and
    wanq_gemm_wq16, and the same message once the entry's own name is taken out."""
    bad = {"operand dtype": dict(dtype=F32), "out dtype": dict(out_dtype=3), "bias dtype": dict(bias=p[0], bias_dtype=4),
           "unknown flag": dict(epi=4), "gate without residual": dict(out_dtype=F32, gate=p[0], epi=EPI_GATE_RES), "N=12": dict(N=12),
           "misaligned out": dict(out=ctypes.c_void_p(p[0].value + 8))}[rule]
    rc_f, msg_f = call_bf16(lib, p[0], **bad)
    rc_q, msg_q = call(lib, p[0], **bad)
    assert rc_f == rc_q and rc_f in (1, 2)
    assert msg_f.startswith(b"wanq_gemm_bf16: ") and msg_q.startswith(b"wanq_gemm_wq16: ")
    assert msg_f.replace(b"wanq_gemm_bf16", b"") == msg_q.replace(b"wanq_gemm_wq16", b"")


def test_each_16bit_entry_names_its_own_k_multiple(lib, p):
    rc, msg = call_bf16(lib, p[0], K=16)
    assert rc == 2 and msg == b"wanq_gemm_bf16: K=16 must be a positive multiple of 32"
    rc, msg = call(lib, p[0], K=32)
    assert rc == 2 and msg == b"wanq_gemm_wq16: K=32 must be a positive multiple of 64"
    assert call_bf16(lib, p[0], K=32, M=0)[0] == 0  # 32 is a whole K for the floating-point entry


def test_m_zero_is_ok_and_launches_nothing(lib, p):
    rc, _ = call(lib, p[0], M=0)
    assert rc == 0


def test_wq16_linear_refuses_cpu_tensors():
    from viditq_extension import qgemm

    x, c = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.wq16_linear(x, c, torch.ones(16))
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.wq16_linear(x, torch.zeros(16, 32, dtype=torch.uint8), torch.ones(16), w4=True)


def test_wq16_linear_refusal_names_the_rule():
    from viditq_extension import qgemm

    for N, K in ((1536, 1536), (8960, 1536), (1536, 8960), (5120, 5120), (13824, 5120), (5120, 13824)):
        assert qgemm.wq16_linear_refusal(1, N, K) is None
    assert "N=12" in qgemm.wq16_linear_refusal(1, 12, 64)
    assert "K=96" in qgemm.wq16_linear_refusal(1, 16, 96) and "multiple of 64" in qgemm.wq16_linear_refusal(1, 16, 96)


def test_integer_weight_linears_keep_their_state_dict_keys():
    """HipLinearW8A8 and HipLinearWq16 register the same buffers in the same order (checkpoints and the --dit_fsdp views go by these
    keys); the lists are those of the classes before they shared a base."""
    from wan.quant_wanx_hip import HipLinearW8A8, HipLinearWq16

    expected = {  # (w_bits, sym, bias)
        (4, False, False): ["weight", "scale_weight", "zp_weight", "zp_gemm"],
        (4, False, True): ["weight", "scale_weight", "zp_weight", "zp_gemm", "bias"],
        (4, True, False): ["weight", "scale_weight", "zp_gemm"],
        (4, True, True): ["weight", "scale_weight", "zp_gemm", "bias"],
        (8, False, False): ["weight", "scale_weight", "zp_weight"],
        (8, False, True): ["weight", "scale_weight", "zp_weight", "bias"],
        (8, True, False): ["weight", "scale_weight"],
        (8, True, True): ["weight", "scale_weight", "bias"],
    }
    for cls in (HipLinearW8A8, HipLinearWq16):
        for (w_bits, sym, bias), keys in expected.items():
            m = cls(64, 16, bias, sym, w_bits)
            sd = m.state_dict()
            assert list(sd.keys()) == keys, (cls.__name__, w_bits, sym, bias)
            assert sd["weight"].dtype == (torch.uint8 if w_bits == 4 else torch.int8)
            assert tuple(sd["weight"].shape) == (16, 32 if w_bits == 4 else 64)
            assert all(v.dtype == torch.float32 and tuple(v.shape) == (16,) for k, v in sd.items() if k != "weight")
            assert (m.zp is m.zp_gemm) if w_bits == 4 else (m.zp is m.zp_weight)


@pytest.mark.parametrize("name,bits", [("w8a16_all_linears.yaml", 8), ("w4a16_all_linears.yaml", 4)])
def test_weight_only_configs_parse_and_have_no_act_section(name, bits):
    from qdiff import config as qcfg

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", name))
    ref = qcfg.load(os.path.join(PKG, "quant_configs", "w8a8_all_linears.yaml"))
    assert "act" not in cfg and cfg.get("act", None) is None
    assert cfg.weight.n_bits == bits and cfg.weight.sym is False
    assert cfg.remain_fp_regex == ref.remain_fp_regex
    assert all(cfg.get(k, None) is None for k in ("viditq", "smooth_quant", "quarot"))


def _torch_weight_kernels(monkeypatch):
    """torch stand-ins for the two HIP kernels of the weight quantiser (row statistics, codes + dequant: the equations of
    qdiff/base/base_quantizer.py), so that a layer can be built on the CPU"""
    from viditq_extension import fused

    def row_minmax(w):
        return w.amin(dim=1), w.amax(dim=1), w.abs().amax(dim=1)

    def weight_quant(w, delta, zp, lo, hi, want_codes=True, want_dequant=True):
        q = (torch.round(w / delta[:, None]) - zp[:, None]).clamp(lo, hi)
        return q.to(torch.int8), (q + zp[:, None]) * delta[:, None]

    monkeypatch.setattr(fused, "row_minmax", row_minmax)
    monkeypatch.setattr(fused, "weight_quant", weight_quant)


def test_bitwidth_refactor_of_a_weight_only_mixed_precision_config(monkeypatch):
    """A weight-only config with a bit-width list and `mixed_precision.weight` only (no `act` list, no activation quantiser): surgery,
    bitwidth_refactor, set_init_done and save / load of the quant params run, the matched layer is re-quantised at the new width
    and the other keeps its own; the forward is F.linear on the re-quantised weight."""
    from qdiff import config as qcfg
    from qdiff.base.mixed_precision_quantizer import MixedPrecisionStaticQuantizer
    from qdiff.base.quant_model import QuantModel

    _torch_weight_kernels(monkeypatch)
    cfg = qcfg.create({"weight": {"n_bits": [4, 8], "i_bitwidth": 1, "sym": False},
                       "mixed_precision": {"weight": {"layer_name_regex": ["", "ffn", ""]}}})

    class Net(QuantModel):
        def __init__(self):
            super().__init__()
            self.q_cfg = cfg
            self.attn = torch.nn.Linear(24, 16)
            self.ffn = torch.nn.Linear(24, 16)

    def build():
        torch.manual_seed(0)
        net = Net()
        net.quant_layer_refactor()
        return net

    net = build()
    for lin in (net.attn, net.ffn):
        assert lin.a_quantizer is None and isinstance(lin.w_quantizer, MixedPrecisionStaticQuantizer) and lin.w_quantizer.n_bits == 8
    w8 = net.ffn.weight.data.clone()
    net.bitwidth_refactor()
    net.set_init_done()
    assert net.attn.w_quantizer.n_bits == 8 and net.ffn.w_quantizer.n_bits == 4 and net.ffn.quant_mode
    codes = net.ffn.int_weight
    assert int(codes.min()) >= -8 and int(codes.max()) <= 7 and len(codes.unique()) > 8   # 4-bit codes, and the range is used
    assert len(net.attn.int_weight.unique()) > 16                                         # the other layer keeps 8 bits
    wq = net.ffn.w_quantizer
    assert torch.equal(net.ffn.weight.data, (codes.float() + wq.zero_point) * wq.delta) and not torch.equal(net.ffn.weight.data, w8)
    x = torch.randn(3, 24)
    assert torch.equal(net.ffn(x), torch.nn.functional.linear(x, net.ffn.weight, net.ffn.bias))
    params = net.save_quant_param_dict()
    assert sorted(params) == ["attn.w_quantizer", "ffn.w_quantizer"]  # no activation quantiser to save
    fresh = build()
    fresh.load_quant_param_dict(params)
    fresh.bitwidth_refactor()
    fresh.set_init_done()
    assert torch.equal(fresh.ffn.int_weight, codes) and torch.equal(fresh.ffn(x), net.ffn(x))


def test_quantized_linear_from_a_weight_only_config_has_no_act_quantizer(monkeypatch):
    """On the CPU, with torch standing in for the two HIP kernels of the weight quantiser (row statistics, codes + dequant: the
    equations of qdiff/base/base_quantizer.py): the layer has a weight quantiser and no activation quantiser, and its simulation
    forward is the reference's expression, F.linear on the dequantised weight -- not the unquantised fp_module."""
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer
    from qdiff.base.quant_layer import QuantizedLinear
    _torch_weight_kernels(monkeypatch)
    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "w8a16_all_linears.yaml"))
    torch.manual_seed(0)
    fp = torch.nn.Linear(24, 16)
    ql = QuantizedLinear(24, 16, True, fp.weight.device, cfg, fp)
    assert ql.a_quantizer is None and isinstance(ql.w_quantizer, StaticQuantizer) and ql.quant_mode
    assert ql.int_weight.dtype == torch.int8 and tuple(ql.int_weight.shape) == (16, 24)
    x = torch.randn(2, 5, 24)
    y = ql(x)
    assert torch.equal(y, torch.nn.functional.linear(x, ql.weight, ql.bias))
    assert not torch.equal(y, fp(x))
    ql.quant_mode = False
    assert torch.equal(ql(x), fp(x))
