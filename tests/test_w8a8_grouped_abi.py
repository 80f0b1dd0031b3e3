"""CPU-only checks of the group-wise int8 GEMM entry (wanq_gemm_w8a8_grouped) and of the host logic wired to it: the symbol is
declared, exported and prototyped and the header still compiles as C99; the ABI version stays 6; every refusal returns its code and
a message naming the rule before anything is launched; M = 0 is a no-op; qgemm.w8a8_grouped_linear_refusal agrees with the C entry.
Python side: quant_configs/w4a8_g128_all_linears.yaml parses; `weight.group_size` with an `act:` section is no longer refused when a
layer is built, unless its weight is in host memory (the kernel has no host form); a bit-width list and the transform classes still
are refused, by layer name and key; the buffers and the construction-time refusals of a grouped HipLinearW8A8.  The kernel itself: tests/test_gpu_w8a8_grouped.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
HEADER = os.path.join(ROOT, "include", "wanq_hip.h")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")
NAME = "wanq_gemm_w8a8_grouped"
F16, BF16, F32, I32 = 0, 1, 2, 3
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
ARGTYPES = [vp, vp, i, vp, vp, i, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import importlib.util

        spec = importlib.util.spec_from_file_location("wanq_build", os.path.join(PKG, "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = ctypes.CDLL(LIB)
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    yield ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16), buf  # host memory: never dereferenced by a refused call


def call(lib, ptr, **kw):
    """wanq_gemm_w8a8_grouped on a well-formed [8, 256] x [16, 256] 4-bit problem with groups of 128, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, w_bits=4, sw=ptr, zp=ptr, group_size=128, out=ptr, out_dtype=BF16, sa=ptr, tok_dtype=F32, bias=None,
             ch_dtype=F32, gate=None, residual=None, epi=0, M=8, N=16, K=256)
    a.update(kw)
    fn = getattr(lib, NAME)
    fn.argtypes = ARGTYPES
    rc = fn(a["a"], a["w"], a["w_bits"], a["sw"], a["zp"], a["group_size"], a["out"], a["out_dtype"], a["sa"], a["tok_dtype"], a["bias"],
            a["ch_dtype"], a["gate"], a["residual"], a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def test_symbol_is_declared_exported_and_prototyped(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", src)
    assert m, f"{NAME} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES), params
    assert params[:6] == ["const int8_t* a", "const void* w", "int w_bits", "const float* sw", "const float* zp", "int group_size"], params
    assert hasattr(lib, NAME), f"{NAME} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert NAME in _C.PROTOTYPES and list(_C.PROTOTYPES[NAME]) == ARGTYPES


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return (int)(sizeof(&%s) == 0); }\n' % NAME)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_version_stays_6(lib):
    assert lib.wanq_abi_version() == 6


@pytest.mark.parametrize("g", [0, 64, 192, -128])
def test_group_size_not_a_multiple_of_128_is_refused(lib, p, g):
    rc, msg = call(lib, p[0], group_size=g, K=384)  # (384 is a multiple of 64 and of 192: the group rule itself refuses)
    assert rc == WANQ_E_SHAPE and NAME.encode() in msg and b"group_size=%d" % g in msg and b"multiple of 128" in msg, (rc, msg)


def test_k_not_a_multiple_of_the_group_is_refused(lib, p):
    rc, msg = call(lib, p[0], K=384, group_size=256)
    assert rc == WANQ_E_SHAPE and NAME.encode() in msg and b"K=384" in msg and b"group_size=256" in msg, (rc, msg)
    rc, msg = call(lib, p[0], K=128, group_size=256)
    assert rc == WANQ_E_SHAPE and b"K=128" in msg and b"group_size=256" in msg, (rc, msg)


def test_n_not_a_multiple_of_8_is_refused(lib, p):
    for N in (12, 4, 0):
        rc, msg = call(lib, p[0], N=N)
        assert rc == WANQ_E_SHAPE and NAME.encode() in msg and b"N=%d" % N in msg and b"multiple of 8" in msg, (rc, msg)


def test_w_bits_and_the_8_bit_zero_point_are_refused(lib, p):
    for bits in (5, 0, 16):
        rc, msg = call(lib, p[0], w_bits=bits)
        assert rc == WANQ_E_ARG and NAME.encode() in msg and b"w_bits=%d" % bits in msg and b"4 or 8" in msg, (rc, msg)
    rc, msg = call(lib, p[0], w_bits=8)
    assert rc == WANQ_E_ARG and NAME.encode() in msg and b"w_bits=8" in msg and b"zp must be NULL" in msg and b"symmetric" in msg, (rc, msg)
    assert call(lib, p[0], w_bits=8, zp=None, M=0)[0] == WANQ_OK


def test_dtypes_are_refused(lib, p):
    rc, msg = call(lib, p[0], out_dtype=I32)
    assert rc == WANQ_E_ARG and NAME.encode() in msg and b"I32" in msg and b"no single integer accumulator" in msg, (rc, msg)
    rc, msg = call(lib, p[0], out_dtype=7)
    assert rc == WANQ_E_ARG and b"out dtype 7" in msg, (rc, msg)
    for bad in (BF16, I32, 9):
        rc, msg = call(lib, p[0], tok_dtype=bad)
        assert rc == WANQ_E_ARG and NAME.encode() in msg and b"tok dtype %d" % bad in msg and b"F16 or F32" in msg, (rc, msg)
    rc, msg = call(lib, p[0], bias=p[0], ch_dtype=BF16)
    assert rc == WANQ_E_ARG and b"ch dtype 1" in msg, (rc, msg)


def test_null_and_misaligned_operands_are_refused(lib, p):
    for which in ("a", "w", "sw", "out", "sa"):
        rc, msg = call(lib, p[0], **{which: None})
        assert rc == WANQ_E_ARG and NAME.encode() in msg and b"non-NULL" in msg, (which, rc, msg)
    for which in ("sw", "zp"):
        rc, msg = call(lib, p[0], **{which: ctypes.c_void_p(p[0].value + 8)})
        assert rc == WANQ_E_ARG and NAME.encode() in msg and b"sw and zp must be 16-byte aligned" in msg, (which, rc, msg)
    rc, msg = call(lib, p[0], out=ctypes.c_void_p(p[0].value + 8))
    assert rc == WANQ_E_ARG and b"a, w, out and residual must be 16-byte aligned" in msg, (rc, msg)
    rc, msg = call(lib, p[0], bias=ctypes.c_void_p(p[0].value + 4), ch_dtype=F16)
    assert rc == WANQ_E_ARG and b"gate and bias must be aligned to 4 elements" in msg, (rc, msg)
    rc, msg = call(lib, p[0], out_dtype=F32, gate=p[0], epi=2)
    assert rc == WANQ_E_ARG and b"WANQ_EPI_GATE_RES needs gate and residual" in msg, (rc, msg)
    rc, msg = call(lib, p[0], epi=4)
    assert rc == WANQ_E_ARG and b"unknown epilogue flag" in msg, (rc, msg)
    rc, msg = call(lib, p[0], M=-1)
    assert rc == WANQ_E_SHAPE and b"M=-1" in msg, (rc, msg)


@pytest.mark.parametrize("g,K", [(128, 128), (128, 256), (256, 512), (384, 384)])
def test_m_zero_is_ok_and_launches_nothing(lib, p, g, K):
    assert call(lib, p[0], M=0, K=K, group_size=g)[0] == WANQ_OK  # (no GPU here: a launch would fail)
    assert call(lib, p[0], M=0, K=K, group_size=g, zp=None)[0] == WANQ_OK


# ---- Python side ---------------------------------------------------------------------------------------------------------------
TABLE = [dict(), dict(group_size=0), dict(group_size=64), dict(group_size=192, K=384), dict(K=384, group_size=256), dict(K=128, group_size=256),
         dict(N=12), dict(N=0), dict(w_bits=5), dict(w_bits=8), dict(w_bits=8, zp=None), dict(K=1536, N=8960), dict(group_size=1536, K=1536)]


@pytest.mark.parametrize("kw", TABLE, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "ok" for kw in TABLE])
def test_python_refusal_agrees_with_the_c_entry(lib, p, kw):
    from viditq_extension import qgemm

    a = dict(N=16, K=256, group_size=128, w_bits=4, zp=p[0])
    a.update(kw)
    rc, msg = call(lib, p[0], M=0, **kw)
    why = qgemm.w8a8_grouped_linear_refusal(1, a["N"], a["K"], a["group_size"], a["w_bits"], a["zp"] is None)
    assert (rc == WANQ_OK) == (why is None), (rc, msg, why)
    if why is not None:  # the same rule: the message of the C entry carries the Python reason's first words
        assert why.split(" must ")[0].split(" takes ")[0].encode() in msg, (why, msg)


def test_wrapper_refuses_cpu_tensors_and_names_the_rules():
    from viditq_extension import qgemm

    x, c = torch.zeros(4, 256, dtype=torch.int8), torch.zeros(16, 128, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.w8a8_grouped_linear(x, c, torch.ones(4), torch.ones(2, 16), None, 128, w4=True)
    for N, K in ((1536, 1536), (8960, 1536), (1536, 8960), (5120, 5120), (13824, 5120), (5120, 13824)):
        assert qgemm.w8a8_grouped_linear_refusal(1, N, K, 128, 4, False) is None
    assert "group_size=96" in qgemm.w8a8_grouped_linear_refusal(1, 16, 384, 96, 4, False)
    assert "symmetric" in qgemm.w8a8_grouped_linear_refusal(1, 16, 256, 128, 8, False)
    assert qgemm.w8a8_grouped_linear_refusal(1, 16, 256, 128, 8, True) is None


def test_shipped_config_parses_and_is_the_weight_only_one_plus_an_act_section():
    from qdiff import config as qcfg

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "w4a8_g128_all_linears.yaml"))
    ref = qcfg.load(os.path.join(PKG, "quant_configs", "w4a16_g128_all_linears.yaml"))
    assert dict(cfg.weight) == {"n_bits": 4, "sym": False, "group_size": 128} == dict(ref.weight)
    assert dict(cfg.act) == {"n_bits": 8, "sym": True} and ref.get("act", None) is None
    assert cfg.remain_fp_regex == ref.remain_fp_regex and dict(cfg.model) == dict(ref.model)
    assert all(d % 128 == 0 for d in (1536, 8960, 5120, 13824))


class _Probe(Exception):
    pass


def _layer(cls, cfg, name, K=256, N=16, device="meta"):
    """(on the meta device by default: a layer whose weight is in host memory is refused for this combination, see below)"""
    from qdiff import config as qcfg

    fp = torch.nn.Linear(K, N, device=device)
    return cls(K, N, True, fp.weight.device, qcfg.create(cfg) if isinstance(cfg, dict) else cfg, fp, module_name=name)


def test_group_size_with_an_act_section_passes_the_construction_check(monkeypatch):
    """The weight quantiser has no host path, so without a GPU the layer is built, on the meta device, up to the point where it would
    quantise its weight: `_checked_group_size` has returned the group size by then.  A weight in host memory is refused by name: the
    group-wise int8 GEMM has no host form."""
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    def stop(self, w):
        raise _Probe(self.group_size)

    monkeypatch.setattr(QuantizedLinear, "_requantize", stop)
    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "w4a8_g128_all_linears.yaml"))
    with pytest.raises(_Probe) as e:
        _layer(QuantizedLinear, cfg, "blocks.1.ffn.0")
    assert e.value.args == (128,)
    with pytest.raises(_Probe):
        _layer(QuantizedLinear, {"weight": {"n_bits": 8, "sym": True, "group_size": 96}, "act": {"n_bits": 8, "sym": True}}, "l", K=384)
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: weight\.group_size together with an `act:` section needs .* on the GPU"):
        _layer(QuantizedLinear, cfg, "blocks.1.ffn.0", device="cpu")
    with pytest.raises(_Probe):  # weight-only group-wise layers are not concerned
        _layer(QuantizedLinear, {"weight": {"n_bits": 4, "sym": False, "group_size": 128}}, "l", device="cpu")


def test_what_has_no_group_wise_form_is_still_refused_by_layer_name_and_key():
    from qdiff.base.quant_layer import QuantizedLinear
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    name = "blocks.1.ffn.0"
    w, act = {"n_bits": 4, "sym": False, "group_size": 128}, {"n_bits": 8, "sym": True}
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: weight\.group_size.*MixedPrecisionStaticQuantizer"):
        _layer(QuantizedLinear, {"weight": dict(w, n_bits=[4, 8], i_bitwidth=1), "act": act}, name)
    for cls, key in ((SQQuantizedLinear, "smooth_quant"), (QuarotQuantizedLinear, "quarot"), (ViDiTQuantizedLinear, "viditq")):
        with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: weight\.group_size with " + cls.__name__):
            _layer(cls, {"weight": w, "act": act, key: {"alpha": 0.5, "layer_name_regex": ""}}, name)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0: weight\.group_size=96 does not divide in_features=256"):
        _layer(QuantizedLinear, {"weight": dict(w, group_size=96), "act": act}, name)


def test_grouped_kernel_mode_linear_holds_group_major_parameters_and_refuses_by_name():
    from wan.quant_wanx_hip import HipLinearW8A8

    m = HipLinearW8A8(256, 16, True, False, 4, group_size=128, name="blocks.0.self_attn.q")
    sd = m.state_dict()
    assert list(sd.keys()) == ["weight", "scale_weight", "zp_weight", "zp_gemm", "bias"]  # the keys of the per-channel layer
    assert tuple(sd["weight"].shape) == (16, 128) and sd["weight"].dtype == torch.uint8
    assert all(tuple(sd[k].shape) == (2, 16) and sd[k].dtype == torch.float32 for k in ("scale_weight", "zp_weight", "zp_gemm"))
    m8 = HipLinearW8A8(256, 16, False, True, 8, group_size=128)
    assert list(m8.state_dict().keys()) == ["weight", "scale_weight"] and tuple(m8.scale_weight.shape) == (2, 16)
    assert tuple(HipLinearW8A8(256, 16, True, False, 4).scale_weight.shape) == (16,)  # per channel, as before
    for g in (96, 64):
        with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q: weight\.group_size=%d has no kernel-mode form" % g):
            HipLinearW8A8(384, 16, True, False, 4, group_size=g, name="blocks.0.self_attn.q")
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q: weight\.group_size=128 with 8-bit asymmetric weights"):
        HipLinearW8A8(256, 16, True, False, 8, group_size=128, name="blocks.0.self_attn.q")
