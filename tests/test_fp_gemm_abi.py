"""CPU-only checks of the bf16 / fp16 GEMM entry (wanq_gemm_bf16): bad arguments are refused on the host with a return code and a
message naming the rule, before anything is launched, and the Python wrapper refuses tensors that are not on the GPU."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wan2.1-quantization_amd", "lib", "libwanq_hip.so")

F16, BF16, F32 = 0, 1, 2
EPI_GELU, EPI_GATE_RES = 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import importlib.util

        spec = importlib.util.spec_from_file_location("wanq_build", os.path.join(ROOT, "wan2.1-quantization_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = ctypes.CDLL(LIB)
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.wanq_gemm_bf16.argtypes = [vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = ctypes.addressof(buf)
    yield ctypes.c_void_p((addr + 15) // 16 * 16), buf  # 16-byte aligned host memory: never dereferenced by a refused call


def test_abi_version_stays_6(lib):
    assert lib.wanq_abi_version() == 6


def test_null_operands_are_refused(lib, p):
    ptr, _ = p
    rc = lib.wanq_gemm_bf16(None, ptr, BF16, ptr, BF16, None, F32, None, None, 0, 8, 16, 64, None)
    assert rc == 1 and b"non-NULL" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, None, BF16, None, F32, None, None, 0, 8, 16, 64, None)
    assert rc == 1 and b"non-NULL" in lib.wanq_last_error()


def test_shape_rules_are_refused_with_the_rule(lib, p):
    ptr, _ = p
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, BF16, None, F32, None, None, 0, 8, 12, 64, None)
    assert rc == 2 and b"N=12" in lib.wanq_last_error() and b"multiple of 8" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, BF16, None, F32, None, None, 0, 8, 16, 48, None)
    assert rc == 2 and b"K=48" in lib.wanq_last_error() and b"multiple of 32" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, BF16, None, F32, None, None, 0, -1, 16, 64, None)
    assert rc == 2 and b"M=-1" in lib.wanq_last_error()


def test_bad_dtypes_and_flags_are_refused(lib, p):
    ptr, _ = p
    rc = lib.wanq_gemm_bf16(ptr, ptr, F32, ptr, BF16, None, F32, None, None, 0, 8, 16, 64, None)  # fp32 operands
    assert rc == 1 and b"operand dtype 2" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, 3, None, F32, None, None, 0, 8, 16, 64, None)  # int32 output
    assert rc == 1 and b"out dtype 3" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, BF16, ptr, 4, None, None, 0, 8, 16, 64, None)  # int16 bias
    assert rc == 1 and b"bias dtype 4" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, BF16, None, F32, None, None, 4, 8, 16, 64, None)
    assert rc == 1 and b"unknown epilogue flag" in lib.wanq_last_error()


def test_gate_residual_needs_both(lib, p):
    ptr, _ = p
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, F32, None, F32, ptr, None, EPI_GATE_RES, 8, 16, 64, None)
    assert rc == 1 and b"needs gate and residual" in lib.wanq_last_error()
    rc = lib.wanq_gemm_bf16(ptr, ptr, BF16, ptr, F32, None, F32, None, ptr, EPI_GATE_RES | EPI_GELU, 8, 16, 64, None)
    assert rc == 1 and b"needs gate and residual" in lib.wanq_last_error()


def test_misaligned_operands_are_refused(lib, p):
    ptr, _ = p
    off = ctypes.c_void_p(ptr.value + 8)
    rc = lib.wanq_gemm_bf16(off, ptr, BF16, ptr, BF16, None, F32, None, None, 0, 8, 16, 64, None)
    assert rc == 1 and b"16-byte aligned" in lib.wanq_last_error()


def test_fp_linear_refuses_cpu_tensors():
    from viditq_extension import qgemm

    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.fp_linear(x, w)


def test_fp_linear_refusal_names_the_rule():
    from viditq_extension import qgemm

    assert qgemm.fp_linear_refusal(1, 1536, 1536) is None and qgemm.fp_linear_refusal(1, 13824, 5120) is None
    assert "N=12" in qgemm.fp_linear_refusal(1, 12, 64) and "K=48" in qgemm.fp_linear_refusal(1, 16, 48)


def test_hip_fp_gemm_refuses_a_layer_it_cannot_take_when_the_model_is_built():
    from wan.quant_wanx_hip import HipLinearFp

    w = torch.zeros(12, 64)
    with pytest.raises(ValueError, match=r"blocks\.3\.ffn\.0.*N=12"):
        HipLinearFp(w, None, torch.bfloat16, "hip", "blocks.3.ffn.0")
    assert HipLinearFp(w, None, torch.bfloat16).fp_gemm == "torch"  # the default path takes any shape, as before
    with pytest.raises(ValueError, match="fp_gemm"):
        HipLinearFp(w, None, torch.bfloat16, "rocblas")


def test_cli_default_is_torch():
    from wan import cli

    p = cli.build_parser("x", quant=True)
    assert p.parse_args([]).fp_gemm == "torch"
    assert p.parse_args(["--fp_gemm", "hip"]).fp_gemm == "hip"
