"""CPU-only checks of K smoothing for the int8 Q.K^T attention (attn.qk.smooth_k / cross_attn.qk.smooth_k): the two C entries
(wanq_rmsnorm_rope_colsum, wanq_rmsnorm_rope_q8_centered) and the sizing function are declared, exported and prototyped, the ABI
version stays 6, and every refusal returns its code and a message before anything is launched.  Python side: the key is read from
the quant config (absent, false, true), `smooth_k` without `qk` is refused by name, and the block's keyword arguments default to
False.  Last, the reason no attention kernel changes, stated in torch.  The kernels themselves: tests/test_gpu_smooth_k.py."""
import copy
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wan2.1-quantization_amd")
HEADER = os.path.join(ROOT, "include", "wanq_hip.h")
LIB = os.path.join(PKG, "lib", "libwanq_hip.so")
YAML = os.path.join(PKG, "quant_configs", "w8a8_all_linears_qk8.yaml")
COLSUM, WS, CENTERED = "wanq_rmsnorm_rope_colsum", "wanq_rmsnorm_rope_colsum_workspace", "wanq_rmsnorm_rope_q8_centered"
F16, BF16, F32 = 0, 1, 2
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
ARGTYPES = {COLSUM: [vp, i, vp, vp, i64, i, i, i64, i64, f, vp, vp, i64, vp], WS: [i64, i],
            CENTERED: [vp, i, vp, vp, vp, i, vp, vp, i64, vp, i64, i, i, i64, i64, f, vp]}


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
    for name, args in ARGTYPES.items():
        getattr(lib, name).argtypes = args
    getattr(lib, WS).restype = ctypes.c_int64
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    yield ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16), buf  # host memory: never dereferenced by a refused call


def colsum(lib, ptr, **kw):
    """wanq_rmsnorm_rope_colsum on a well-formed [4, 256] problem, with the named arguments replaced"""
    a = dict(x=ptr, x_dtype=F32, weight=ptr, rope=None, rows=4, cols=256, head_dim=128, rows_per_batch=4, positions=0, eps=1e-6, colsum=ptr,
             workspace=ptr, workspace_bytes=4096)
    a.update(kw)
    rc = getattr(lib, COLSUM)(a["x"], a["x_dtype"], a["weight"], a["rope"], a["rows"], a["cols"], a["head_dim"], a["rows_per_batch"],
                              a["positions"], a["eps"], a["colsum"], a["workspace"], a["workspace_bytes"], None)
    return rc, lib.wanq_last_error()


def centered(lib, ptr, **kw):
    """wanq_rmsnorm_rope_q8_centered on a well-formed [4, 256] problem, with the named arguments replaced"""
    a = dict(x=ptr, x_dtype=F32, weight=ptr, rope=None, out=None, out_dtype=BF16, q8=ptr, qscale=ptr, scale_stride=64, center=ptr, rows=4,
             cols=256, head_dim=128, rows_per_batch=4, positions=0, eps=1e-6)
    a.update(kw)
    rc = getattr(lib, CENTERED)(a["x"], a["x_dtype"], a["weight"], a["rope"], a["out"], a["out_dtype"], a["q8"], a["qscale"], a["scale_stride"],
                                a["center"], a["rows"], a["cols"], a["head_dim"], a["rows_per_batch"], a["positions"], a["eps"], None)
    return rc, lib.wanq_last_error()


# ---- entries ----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_prototyped(lib):
    from viditq_extension import _C

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in (COLSUM, WS, CENTERED):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/wanq_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert _C.PROTOTYPES[name] == ARGTYPES[name]
    assert _C.lib.wanq_rmsnorm_rope_colsum_workspace.restype is ctypes.c_int64
    assert re.search(r"int64_t\s+" + WS + r"\s*\(\s*int64_t rows,\s*int cols\s*\)", src)
    assert "const float* center" in src and "float* colsum" in src
    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6


def test_workspace_is_a_function_of_the_shape_alone(lib):
    """64-row slabs, doubled until at most 1024 remain: one fp32 [cols] partial per slab."""
    ws = getattr(lib, WS)
    assert ws(0, 256) == 0
    for rows, slabs in ((1, 1), (63, 1), (64, 1), (65, 2), (256, 4), (1000, 16), (65536, 1024), (65537, 513), (32760, 512), (75600, 591)):
        assert ws(rows, 1536) == slabs * 1536 * 4, rows


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_colsum_refusals_carry_messages(lib, p):
    ptr, _ = p
    rc, msg = colsum(lib, ptr, colsum=None)
    assert rc == WANQ_E_ARG and b"colsum is NULL" in msg
    rc, msg = colsum(lib, ptr, x=None)
    assert rc == WANQ_E_ARG and b"NULL" in msg
    rc, msg = colsum(lib, ptr, x_dtype=3)
    assert rc == WANQ_E_ARG and b"dtype" in msg
    # a short (or missing) workspace: 4 rows are one slab of 256 fp32 partials
    rc, msg = colsum(lib, ptr, workspace_bytes=1023)
    assert rc == WANQ_E_ARG and b"workspace of 1023 bytes, 1024 needed" in msg
    rc, msg = colsum(lib, ptr, workspace=None, workspace_bytes=4096)
    assert rc == WANQ_E_ARG and b"workspace of 0 bytes, 1024 needed" in msg
    # cols is a whole number of the row frame's 8-element chunks
    rc, msg = colsum(lib, ptr, cols=252)
    assert rc == WANQ_E_SHAPE and b"cols=252 must be a multiple of 8" in msg
    rc, msg = colsum(lib, ptr, cols=16392)
    assert rc == WANQ_E_SHAPE and b"cols=16392" in msg
    rc, msg = colsum(lib, ptr, rope=ptr, head_dim=96)
    assert rc == WANQ_E_SHAPE and b"head_dim=96" in msg
    rc, msg = colsum(lib, ptr, rows=-1)
    assert rc == WANQ_E_SHAPE and b"rows=-1" in msg


def test_centered_refusals_carry_messages(lib, p):
    ptr, _ = p
    rc, msg = centered(lib, ptr, center=None)
    assert rc == WANQ_E_ARG and b"center is NULL" in msg
    rc, msg = centered(lib, ptr, q8=None)
    assert rc == WANQ_E_ARG and b"q8 is required" in msg
    rc, msg = centered(lib, ptr, head_dim=64)
    assert rc == WANQ_E_ARG and b"head_dim == 128" in msg
    rc, msg = centered(lib, ptr, qscale=None)
    assert rc == WANQ_E_ARG and b"needs qscale" in msg
    rc, msg = centered(lib, ptr, cols=264)  # a multiple of the 8-element chunk, but not of the 128-column head
    assert rc == WANQ_E_ARG and b"cols % 128 == 0" in msg
    rc, msg = centered(lib, ptr, cols=252)
    assert rc != WANQ_OK and msg


def test_python_wrappers_have_no_cpu_fallback():
    from wan import ops

    x, w = torch.zeros(4, 256), torch.ones(256)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.rmsnorm_rope_colsum(x, w, None, 128)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.rmsnorm_rope_q8(x, w, None, 128, True, center=torch.zeros(256))
    c = ops.center_of(torch.tensor([3.0, 1.0]), 3)
    assert c.dtype == torch.float32 and torch.equal(c, torch.tensor([1.0, 1.0 / 3.0]))  # a true division, one rounding


# ---- config and kernel mode ---------------------------------------------------------------------------------------------------
def _cfg():
    """quant_configs/w8a8_all_linears_qk8.yaml, edited in memory: without its `viditq` section, whose rotations want a calibration pass,
    and with the Linears in the fp8 format, the one whose codes are made in host memory (int8 weights are quantised on the GPU); the
    `attn` section, which these tests are about, is the file's"""
    from qdiff import config as qcfg

    cfg = qcfg.load(YAML)
    del cfg["viditq"]
    cfg["weight"]["format"] = cfg["act"]["format"] = "fp8_e4m3"
    cfg["weight"]["sym"] = True
    return cfg


def _kernel_mode(cfg):
    """hardware_forward_refactor of a tiny model in host memory -> its first kernel-mode block"""
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    fp = WanModel(dim=128, ffn_dim=256, num_heads=1, num_layers=1, text_dim=64, freq_dim=64).eval()
    model = QuantWanModel.from_float(fp, cfg)
    model.quant_layer_refactor()
    model.set_init_done()
    model.hardware_forward_refactor()
    return model.hip_blocks[0]


def test_the_key_is_read_absent_false_and_true():
    from qdiff import config as qcfg

    b = _kernel_mode(_cfg())
    assert b.attn_qk8 and not b.cross_attn_qk8 and b.attn_smooth_k is False and b.cross_attn_smooth_k is False
    for value in (False, True):
        cfg = _cfg()
        cfg["attn"]["qk"]["smooth_k"] = value
        b = _kernel_mode(cfg)
        assert b.attn_qk8 and b.attn_smooth_k is value and b.cross_attn_smooth_k is False
    cfg = _cfg()
    cfg["cross_attn"] = qcfg.create({"qk": {"n_bits": 8, "sym": True, "smooth_k": True}})
    b = _kernel_mode(cfg)
    assert b.attn_smooth_k is False and b.cross_attn_qk8 and b.cross_attn_smooth_k is True


@pytest.mark.parametrize("key", ["attn", "cross_attn"])
def test_smooth_k_without_qk_is_refused_by_name(key):
    from qdiff import config as qcfg

    cfg = _cfg()
    cfg[key] = qcfg.create({"smooth_k": True, "v": {"n_bits": 8, "sym": True}})
    with pytest.raises(ValueError, match=rf"^{key}\.smooth_k: .*{key}\.qk\.smooth_k.*no {key}\.qk"):
        _kernel_mode(cfg)


def test_block_keywords_default_to_false_and_need_their_qk():
    import inspect

    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel as Blk

    for fn in (Blk.__init__, Blk.from_float):
        sig = inspect.signature(fn).parameters
        assert sig["attn_smooth_k"].default is False and sig["cross_attn_smooth_k"].default is False
    b = Blk(128, 256, 1)
    assert b.attn_smooth_k is False and b.cross_attn_smooth_k is False
    b = Blk(128, 256, 1, attn_qk8=True, cross_attn_qk8=True, attn_smooth_k=True, cross_attn_smooth_k=True)
    assert b.attn_smooth_k is True and b.cross_attn_smooth_k is True
    with pytest.raises(ValueError, match=r"attn\.qk\.smooth_k without attn\.qk"):
        Blk(128, 256, 1, attn_smooth_k=True)
    with pytest.raises(ValueError, match=r"cross_attn\.qk\.smooth_k without cross_attn\.qk"):
        Blk(128, 256, 1, attn_qk8=True, cross_attn_smooth_k=True)


def test_the_sequence_parallel_centre_of_one_rank_is_the_division():
    from wan.distributed.parallel import SeqParallel

    s = torch.tensor([3.0, -7.0, 0.5])
    assert torch.equal(SeqParallel(False).mean_rows(s, 7), s / 7.0)


# ---- why no attention kernel changes ----------------------------------------------------------------------------------------------
def test_softmax_does_not_see_a_vector_shared_by_all_keys():
    """softmax(q (k - c)^T) v == softmax(q k^T) v: subtracting c from every key moves all scores of a query row by the same q.c."""
    g = torch.Generator().manual_seed(0)
    Lq, Lk, d = 37, 53, 128
    q, k, v = (torch.randn(n, d, generator=g, dtype=torch.float64) for n in (Lq, Lk, Lk))
    k = k + 6.0 * torch.randn(d, generator=g, dtype=torch.float64)  # the per-channel offset of a trained K
    c = copy.deepcopy(k.mean(0))
    plain = torch.softmax(q @ k.t() / d ** 0.5, -1) @ v
    smooth = torch.softmax(q @ (k - c).t() / d ** 0.5, -1) @ v
    assert (plain - smooth).abs().max().item() < 1e-12
