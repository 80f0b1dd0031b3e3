"""CPU-only: the wanq_layernorm_quant_rows_* entries refuse bad arguments on the host with a code and a message naming the value."""
import ctypes
import re
import pytest

from test_abi import HEADER, lib  # noqa: F401  (the fixture builds the library when it is missing)

ARG, SHAPE, E4M3, E2M1, E2M3 = 1, 2, 0, 1, 2
ENTRIES = ("wanq_layernorm_quant_rows_fp8", "wanq_layernorm_quant_rows_mx", "wanq_layernorm_quant_rows_mx4_search")


# -> (return code, message); one aligned host buffer stands for every tensor: a refused call touches none of them
def call(lib, name, x=True, q=True, scale=True, rows_per_batch=4, cols=64, fmt=E2M1, had32=0):
    from viditq_extension import _C
    buf = ctypes.create_string_buffer(256 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = _C.PROTOTYPES[name], ctypes.c_int
    tail = () if name.endswith("fp8") else (fmt, had32)
    rc = fn(p if x else None, 2, None, None, None, 0, rows_per_batch, 1e-6, p if q else None, p if scale else None, 4, cols, *tail, None)
    lib.wanq_last_error.restype = ctypes.c_char_p
    return rc, lib.wanq_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_null_pointers_shapes_and_arity(lib, name):
    from viditq_extension import _C
    for missing in ("x", "q", "scale"):
        rc, msg = call(lib, name, **{missing: False})
        assert rc == ARG and name in msg and "non-NULL" in msg
    rule = 8 if name.endswith("fp8") else 32
    for cols in (rule * 3 + 4, 16384 + rule):
        rc, msg = call(lib, name, cols=cols)
        assert rc == SHAPE and f"cols={cols}" in msg
    rc, msg = call(lib, name, rows_per_batch=0)
    assert rc == ARG and "rows_per_batch=0" in msg
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    assert len(_C.PROTOTYPES[name]) == len(params.split(","))


@pytest.mark.parametrize("name,fmt,had32,words", [(ENTRIES[1], 3, 0, ("fmt=3",)), (ENTRIES[1], E2M3, 1, ("had32=1", "WANQ_MX_E2M3")),
                                                  (ENTRIES[1], E2M1, 2, ("had32=2",)), (ENTRIES[2], E4M3, 0, ("fmt=0", "WANQ_MX_E2M1")),
                                                  (ENTRIES[2], E2M3, 0, ("fmt=2", "WANQ_MX_E2M1")), (ENTRIES[2], E2M1, -1, ("had32=-1",))])
def test_formats_and_the_rotation_flag_are_checked(lib, name, fmt, had32, words):
    rc, msg = call(lib, name, fmt=fmt, had32=had32)
    assert rc == ARG and all(w in msg for w in words)
