"""CPU-only checks of the sliding-window attention entry (wanq_attention_window_fwd): it is declared in the header, exported by
the library and prototyped in the binding; the ABI version stays 6; bad arguments are refused on the host with a return code and a
message naming the entry and the rule, before anything is launched; Lq = 0 is a no-op."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
HEADER = os.path.join(ROOT, "include", "wanq_hip.h")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")
NAME = "wanq_attention_window_fwd"
F16, BF16, F32 = 0, 1, 2
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
ARGTYPES = [vp, vp, vp, vp, i, i64, i64, i, i, i64, i64, i64, i64, f, i64, i64, vp]


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
    """wanq_attention_window_fwd on a well-formed 8 x 8 problem of two heads, window (3, 3), with the named arguments replaced"""
    a = dict(q=ptr, k=ptr, v=ptr, o=ptr, dtype=BF16, Lq=8, Lk=8, heads=2, head_dim=128, q_stride=256, k_stride=256, v_stride=256,
             o_stride=256, scale=0.088, left=3, right=3)
    a.update(kw)
    fn = getattr(lib, NAME)
    fn.argtypes = ARGTYPES
    rc = fn(a["q"], a["k"], a["v"], a["o"], a["dtype"], a["Lq"], a["Lk"], a["heads"], a["head_dim"], a["q_stride"], a["k_stride"],
            a["v_stride"], a["o_stride"], a["scale"], a["left"], a["right"], None)
    return rc, lib.wanq_last_error()


def test_symbol_is_declared_exported_and_prototyped(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", src)
    assert m, f"{NAME} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES) and params[-3:] == ["int64_t window_left", "int64_t window_right", "void* stream"], params
    assert hasattr(lib, NAME), f"{NAME} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert NAME in _C.PROTOTYPES and list(_C.PROTOTYPES[NAME]) == ARGTYPES


def test_abi_version_stays_6(lib):
    assert lib.wanq_abi_version() == 6


def test_bad_dtype_is_refused(lib, p):
    for code in (F32, 3, -1):
        rc, msg = call(lib, p[0], dtype=code)
        assert rc == WANQ_E_ARG and NAME.encode() in msg and b"dtype" in msg, (code, rc, msg)


def test_head_dim_other_than_128_is_refused(lib, p):
    for hd in (64, 96, 256):
        rc, msg = call(lib, p[0], head_dim=hd)
        assert rc == WANQ_E_SHAPE and NAME.encode() in msg and b"head_dim=%d" % hd in msg, (hd, rc, msg)


@pytest.mark.parametrize("which", ["q_stride", "k_stride", "v_stride", "o_stride"])
def test_stride_below_heads_times_128_is_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: 248})
    assert rc == WANQ_E_SHAPE and NAME.encode() in msg and b"stride" in msg, (rc, msg)
    rc, msg = call(lib, p[0], **{which: 260})  # large enough, not a multiple of 8 elements
    assert rc == WANQ_E_SHAPE and b"multiples of 8" in msg, (rc, msg)


@pytest.mark.parametrize("which", ["q", "k", "v", "o"])
def test_null_operands_are_refused(lib, p, which):
    rc, msg = call(lib, p[0], **{which: None})
    assert rc == WANQ_E_ARG and NAME.encode() in msg and b"NULL" in msg, (rc, msg)


@pytest.mark.parametrize("window", [(3, 3), (-1, -1), (0, -1), (5000, 5000)])
def test_lq_zero_is_ok_and_launches_nothing(lib, p, window):
    rc, _ = call(lib, p[0], Lq=0, left=window[0], right=window[1])  # (no GPU here: a launch would fail)
    assert rc == WANQ_OK
