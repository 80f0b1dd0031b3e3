"""CPU-only checks of gptq.act_order and of the two entries it and the calibration hook brought (wanq_gptq_block_gidx in
csrc/gptq.hip, wanq_gram_accumulate in csrc/gram.hip): both are in the header, in the binding and in the library at ABI version 6 and
the header stays pedantic C99; bad arguments are refused on the host with the rule in the message; the config key parses, is
refused by layer name when it is no bool, and lifts the evenness rule only when it is on; the host model (qdiff/base/gptq.py, the
specification of act_order): an already descending diagonal changes nothing, the order is the stable descending sort of diag H
(ties to the lower channel, a dead channel last), the dequantised weight is (codes + zp) * delta on the unpermuted layout and the
grid is round-to-nearest's to the bit."""
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
GIDX, GRAM = "wanq_gptq_block_gidx", "wanq_gram_accumulate"
BF16, F16, F32 = 1, 0, 2


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
    getattr(lib, GIDX).argtypes = [vp, i64, vp, i64, vp, vp, vp, i, i, i, vp, vp, i64, i, i, i, vp]
    getattr(lib, GRAM).argtypes = [vp, i, vp, i64, i, vp]
    lib.wanq_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture()
def p():
    buf = ctypes.create_string_buffer(4096 + 16)
    a = ctypes.addressof(buf)
    yield ctypes.c_void_p(a + (-a) % 16)  # 16-byte aligned host memory: never dereferenced by a refused call (or by N = 0, rows = 0)


def gidx(lib, ptr, **kw):
    a = dict(w=ptr, w_stride=256, u=ptr, u_stride=256, delta=ptr, zp=ptr, g_idx=ptr, G=2, qmin=-8, qmax=7, codes=ptr, err=ptr, N=4, K=256,
             c0=0, cols=128)
    a.update(kw)
    rc = getattr(lib, GIDX)(a["w"], a["w_stride"], a["u"], a["u_stride"], a["delta"], a["zp"], a["g_idx"], a["G"], a["qmin"], a["qmax"],
                            a["codes"], a["err"], a["N"], a["K"], a["c0"], a["cols"], None)
    return rc, lib.wanq_last_error()


def gram(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=BF16, H=ptr, rows=0, C=64)
    a.update(kw)
    rc = getattr(lib, GRAM)(a["x"], a["x_dtype"], a["H"], a["rows"], a["C"], None)
    return rc, lib.wanq_last_error()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_in_header_binding_and_library_at_abi_6(lib):
    from viditq_extension import _C

    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6
    text = open(HEADER).read()
    for entry, n in ((GIDX, 17), (GRAM, 6)):
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"the header declares {entry}"
        assert len(m.group(1).split(",")) == n and len(_C.PROTOTYPES[entry]) == n
        assert hasattr(lib, entry)
    args = re.search(GIDX + r"\s*\(([^;]*)\)", text).group(1)
    assert "const int32_t* g_idx" in args and "int G" in args and "group_size" not in args
    # the entries that were there stay as they were
    assert len(_C.PROTOTYPES["wanq_gptq_block"]) == 16 and len(_C.PROTOTYPES["wanq_gptq_propagate"]) == 10


def test_header_is_still_pedantic_c99(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return wanq_gptq_block_gidx(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   "wanq_gram_accumulate(0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("which", ["w", "u", "delta", "zp", "g_idx", "codes", "err"])
def test_gidx_refuses_null_pointers(lib, p, which):
    rc, msg = gidx(lib, p, **{which: None})
    assert rc == 1 and GIDX.encode() in msg and b"non-NULL" in msg and which.encode() in msg


def test_gidx_shape_rules_are_refused_with_the_rule(lib, p):
    for G in (0, -3):
        rc, msg = gidx(lib, p, G=G)
        assert rc == 2 and msg == b"wanq_gptq_block_gidx: G=%d must be at least 1 (the groups of a row of delta / zp)" % G
    for cols in (0, -1, 129, 256):
        rc, msg = gidx(lib, p, cols=cols)
        assert rc == 2 and msg == b"wanq_gptq_block_gidx: cols=%d must be 1..128" % cols
    rc, msg = gidx(lib, p, c0=192, cols=128)
    assert rc == 2 and msg == b"wanq_gptq_block_gidx: c0=192 + cols=128 must not exceed K=256"
    rc, msg = gidx(lib, p, c0=-2)
    assert rc == 2 and b"c0=-2" in msg
    rc, msg = gidx(lib, p, w_stride=255)
    assert rc == 2 and b"w_stride=255" in msg and b"at least K=256" in msg
    rc, msg = gidx(lib, p, u_stride=100)
    assert rc == 2 and b"u_stride=100" in msg and b"at least K=256" in msg
    rc, msg = gidx(lib, p, N=-1)
    assert rc == 2 and b"N=-1" in msg
    rc, msg = gidx(lib, p, qmin=-129)
    assert rc == 1 and b"qmin=-129" in msg
    rc, msg = gidx(lib, p, qmin=3, qmax=2)
    assert rc == 1 and b"int8 range" in msg


def test_gidx_has_no_evenness_rule_and_n_zero_launches_nothing(lib, p):
    # what wanq_gptq_block refuses with a group size (an odd c0, odd groups) is no rule here; N = 0 returns before any launch
    assert gidx(lib, p, N=0)[0] == 0 and gidx(lib, p, N=0, c0=33, cols=5)[0] == 0 and gidx(lib, p, N=0, G=85, K=255, w_stride=255, u_stride=255, cols=64)[0] == 0


def test_gram_refusals_name_their_rule(lib, p):
    for which in ("x", "H"):
        rc, msg = gram(lib, p, rows=4, **{which: None})
        assert rc == 1 and msg == b"wanq_gram_accumulate: x and H must be non-NULL"
    for C in (12, 60, 0, -8):
        rc, msg = gram(lib, p, rows=4, C=C)
        assert rc == 2 and b"C=%d must be a multiple of 8" % C in msg
    rc, msg = gram(lib, p, rows=-1)
    assert rc == 2 and b"rows=-1" in msg
    rc, msg = gram(lib, p, rows=4, x_dtype=F32)
    assert rc == 1 and b"x_dtype=2 must be bf16 or fp16" in msg
    off = ctypes.c_void_p(p.value + 8)
    for which in ("x", "H"):
        rc, msg = gram(lib, p, rows=4, **{which: off})
        assert rc == 1 and b"16-byte aligned" in msg
    assert gram(lib, p, rows=0)[0] == 0 and gram(lib, p, rows=0, x_dtype=F16, C=8)[0] == 0  # rows == 0: nothing to add, no launch


def test_python_wrappers_refuse_cpu_tensors():
    from viditq_extension import fused

    w, u = torch.zeros(4, 64), torch.eye(64)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fused.gptq_block_gidx_(w, u, torch.ones(4, 2), torch.zeros(4, 2), torch.zeros(64, dtype=torch.int32), -8, 7,
                               torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, 64), 0, 64)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fused.gram_accumulate_onepass_(torch.zeros(64, 64), torch.zeros(3, 64, dtype=torch.bfloat16))
    assert callable(fused.gram_accumulate_)  # the two-sided form stays exported


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
    return (torch.rand(N, K, generator=g) * 2 - 1) * (6.0 / (N + K)) ** 0.5


def _hessian(K, rows, g, spread=True):
    """H = X^T X (float64) of mildly correlated Gaussian inputs with a lognormal per-channel scale (`spread`): distinct diagonal"""
    z = torch.randn(rows, K, generator=g, dtype=torch.float64)
    x = z @ (torch.eye(K, dtype=torch.float64) + torch.randn(K, K, generator=g, dtype=torch.float64) / K ** 0.5)
    if spread:
        x = x * torch.exp(torch.randn(K, generator=g, dtype=torch.float64))
    return x.T @ x


def _layer(cfg, N, K, seed=0, name="blocks.1.ffn.0"):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    fp = torch.nn.Linear(K, N, bias=True)
    fp.weight.data.copy_(_xavier(N, K, torch.Generator().manual_seed(seed)))
    return QuantizedLinear(K, N, True, fp.weight.device, qcfg.create(cfg), fp, name), fp


GPTQ = {"layer_name_regex": "", "damp": 0.01, "block": 128}
W4G = {"n_bits": 4, "sym": False, "group_size": 16}


# ---- the config key ---------------------------------------------------------------------------------------------------------------
def test_shipped_actorder_config_parses():
    from qdiff import config as qcfg

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "gptq", "w4a16_g128_gptq_actorder_all_linears.yaml"))
    plain = qcfg.load(os.path.join(PKG, "quant_configs", "gptq", "w4a16_g128_gptq_all_linears.yaml"))
    assert dict(cfg.gptq) == {"layer_name_regex": "", "damp": 0.01, "block": 128, "act_order": True}
    assert cfg.gptq.act_order is True and plain.gptq.get("act_order", False) is False
    assert dict(cfg.weight) == dict(plain.weight) and cfg.get("act", None) is None
    assert cfg.remain_fp_regex == plain.remain_fp_regex and cfg.calib_data.hessian_path == plain.calib_data.hessian_path


@pytest.mark.parametrize("bad", [1, 0, "yes", "True", 0.5, None])
def test_a_non_bool_act_order_is_refused_by_layer_name(monkeypatch, bad):
    _torch_weight_kernels(monkeypatch)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0: gptq\.act_order=.* must be True or False"):
        _layer({"weight": W4G, "gptq": dict(GPTQ, act_order=bad)}, 24, 64)


def test_act_order_lifts_the_evenness_rule_and_only_then(monkeypatch):
    _torch_weight_kernels(monkeypatch)
    ql, _ = _layer({"weight": W4G, "gptq": dict(GPTQ, block=33, act_order=True)}, 24, 64)
    assert ql.gptq is not None and ql.gptq.act_order is True
    today = r"blocks\.1\.ffn\.0: gptq with weight\.group_size=16 needs an even group size and an even gptq\.block"
    with pytest.raises(ValueError, match=today):
        _layer({"weight": W4G, "gptq": dict(GPTQ, block=33, act_order=False)}, 24, 64)
    with pytest.raises(ValueError, match=today):
        _layer({"weight": W4G, "gptq": dict(GPTQ, block=33)}, 24, 64)
    ql, _ = _layer({"weight": W4G, "gptq": dict(GPTQ, act_order=False)}, 24, 64)  # absent and False are today's layer
    assert ql.gptq is not None and ql.gptq.get("act_order", False) is False


# ---- the host model ---------------------------------------------------------------------------------------------------------------
def _quantizer(group_size):
    from qdiff import config as qcfg
    from qdiff.base.base_quantizer import StaticQuantizer

    return StaticQuantizer(qcfg.create({"n_bits": 4, "sym": False, **({"group_size": group_size} if group_size else {})}))


def _unpermuted_deq(codes, q, N, K):
    G = q.delta.numel() // N
    return ((codes.float().view(N, G, -1) + q.zero_point.view(N, G, 1)) * q.delta.view(N, G, 1)).view(N, K)


@pytest.mark.parametrize("group_size", [None, 16], ids=["per channel", "g16"])
@pytest.mark.parametrize("block", [128, 16, 7], ids=["one block", "blocks of 16", "blocks of 7"])
def test_a_descending_diagonal_gives_the_plain_solvers_codes(monkeypatch, group_size, block):
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    g = torch.Generator().manual_seed(2)
    N, K = 24, 64
    w, H = _xavier(N, K, g), _hessian(K, 256, g)
    order = torch.sort(torch.diagonal(H), descending=True).indices
    H = H[order][:, order]
    assert (torch.diagonal(H)[:-1] > torch.diagonal(H)[1:]).all()
    U, w0 = gptq.gptq_prepare(H, w, 0.01)
    Up, wp, perm = gptq.gptq_prepare(H, w, 0.01, act_order=True)
    assert torch.equal(perm, torch.arange(K)) and perm.dtype == torch.int64 and torch.equal(Up, U) and torch.equal(wp, w0)
    plain = gptq.gptq_solve_host(w0, U, _quantizer(group_size), block)  # (the host model runs any block: evenness is the kernel's rule)
    ao = gptq.gptq_solve_host(wp, Up, _quantizer(group_size), block, act_order=True, perm=perm)
    assert torch.equal(ao[0], plain[0]) and torch.equal(ao[1].view(torch.int32), plain[1].view(torch.int32))


@pytest.mark.parametrize("group_size", [None, 16], ids=["per channel", "g16"])
@pytest.mark.parametrize("block", [128, 33], ids=["one block", "blocks of 33"])
def test_a_shuffled_diagonal_is_solved_in_stable_descending_order_on_the_round_to_nearest_grid(monkeypatch, group_size, block):
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    g = torch.Generator().manual_seed(3)
    N, K = 24, 64
    w, H = _xavier(N, K, g), _hessian(K, 256, g)
    want_perm = torch.sort(torch.diagonal(H), descending=True, stable=True).indices
    assert not torch.equal(want_perm, torch.arange(K))
    U, wp, perm = gptq.gptq_prepare(H, w, 0.01, act_order=True)
    assert torch.equal(perm, want_perm) and torch.equal(wp, w[:, perm]) and torch.equal(U, torch.triu(U))
    # U factors the permuted, damped Hessian
    Hd = H[perm][:, perm] + 0.01 * torch.diagonal(H).mean() * torch.eye(K, dtype=torch.float64)
    assert torch.allclose(U.double().T @ U.double(), torch.linalg.inv(Hd), rtol=1e-4, atol=1e-9)
    q, rtn = _quantizer(group_size), _quantizer(group_size)
    rtn.init_quant_params(w)
    codes, deq = gptq.gptq_solve_host(wp, U, q, block, act_order=True, perm=perm)
    for a, b in ((q.delta, rtn.delta), (q.zero_point, rtn.zero_point)):  # the grid is that of the UNPERMUTED original weight
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert codes.dtype == torch.int8 and torch.equal(deq, _unpermuted_deq(codes, q, N, K))  # exactly, on the unpermuted layout
    # the same codes from the loop spelt out: the host block model on the permuted problem with the column map perm // group_size
    qmin, qmax = gptq.stored_range(q)
    G = K // group_size if group_size else 1
    g_idx = perm // group_size if group_size else torch.zeros_like(perm)
    ww, cc = wp.clone(), torch.empty(N, K, dtype=torch.int8)
    for c0 in range(0, K, block):
        cols = min(block, K - c0)
        err = gptq.gptq_block_host(ww, U, q.delta.reshape(N, G), q.zero_point.reshape(N, G), group_size, qmin, qmax, cc, c0, cols, g_idx)
        gptq.gptq_propagate_host(ww, U, err, c0, cols)
    back = torch.empty_like(cc)
    back[:, perm] = cc
    assert torch.equal(back, codes)
    # it is GPTQ: below round-to-nearest on the layer objective, and not the plain order's codes
    U0, w0 = gptq.gptq_prepare(H, w, 0.01)
    plain = gptq.gptq_solve_host(w0, U0, _quantizer(group_size), block)
    rtn_codes = torch.clamp(torch.round(w.view(N, G, -1) / q.delta.view(N, G, 1)) - q.zero_point.view(N, G, 1), qmin, qmax).view(N, K)
    o_a, o_p, o_r = (gptq.objective(w, t, H).sum().item() for t in (deq, plain[1], _unpermuted_deq(rtn_codes, q, N, K)))
    print(f"g={group_size} block={block}: objective act_order / RTN {o_a / o_r:.4f}, plain / RTN {o_p / o_r:.4f}, act_order / plain {o_a / o_p:.4f}")
    assert o_a < o_r and not torch.equal(codes, plain[0])
    with pytest.raises(ValueError, match="act_order=True needs perm"):
        gptq.gptq_solve_host(wp, U, q, block, act_order=True)
    with pytest.raises(ValueError, match="act_order=True needs perm"):
        gptq.gptq_solve_host(wp, U, q, block, perm=perm)


def test_a_tie_in_the_diagonal_goes_to_the_lower_channel():
    from qdiff.base import gptq

    H = torch.diag(torch.tensor([2.0, 5.0, 2.0, 7.0, 5.0, 2.0]))
    _, wp, perm = gptq.gptq_prepare(H, torch.arange(12.0).view(2, 6), 0.01, act_order=True)
    assert perm.tolist() == [3, 1, 4, 0, 2, 5]
    assert torch.equal(wp, torch.arange(12.0).view(2, 6)[:, perm])


def test_a_dead_channel_is_handled_as_before_and_solved_last(monkeypatch):
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    g = torch.Generator().manual_seed(4)
    N, K, dead = 24, 64, 9
    w, H = _xavier(N, K, g), _hessian(K, 256, g)
    H[dead, :] = 0.0
    H[:, dead] = 0.0
    assert torch.diagonal(H)[torch.arange(K) != dead].min() > 1.0  # the rule sets a dead channel's diagonal to 1: the smallest here
    U, wp, perm = gptq.gptq_prepare(H, w, 0.01, act_order=True)
    assert perm[-1] == dead and torch.equal(wp[:, -1], torch.zeros(N))     # zeroed as before, and last in the order
    alive = perm[:-1]
    assert torch.equal(alive, torch.sort(torch.diagonal(H), descending=True, stable=True).indices[:-1])
    assert torch.equal(wp[:, :-1], w[:, alive]) and (U[:-1, -1] == 0).all()  # coupled to nothing
    assert H[dead, dead] == 0 and w[:, dead].abs().sum() > 0               # the inputs are not modified
    q = _quantizer(16)
    q.init_quant_params(w)
    q.init_done = True
    codes, deq = gptq.gptq_solve_host(wp, U, q, 128, act_order=True, perm=perm)
    z = q.zero_point.view(N, K // 16)[:, dead // 16]
    assert torch.equal(codes[:, dead].float(), torch.clamp(-z, -8, 7))     # the code of weight 0 on the channel's own group
    assert torch.equal(deq, _unpermuted_deq(codes, q, N, K))


# ---- the layer --------------------------------------------------------------------------------------------------------------------
def test_an_act_order_layer_keeps_the_round_to_nearest_grid_and_layout(monkeypatch):
    from qdiff.base import gptq

    _torch_weight_kernels(monkeypatch)
    N, K = 24, 64
    H = _hessian(K, 256, torch.Generator().manual_seed(5)).float()
    ao, fp = _layer({"weight": W4G, "gptq": dict(GPTQ, block=33, act_order=True)}, N, K)
    plain, _ = _layer({"weight": W4G, "gptq": GPTQ}, N, K)
    rtn, _ = _layer({"weight": W4G}, N, K)
    assert ao.requantize_gptq_(H) is ao and plain.requantize_gptq_(H) is plain
    for a, b in ((ao.w_quantizer.delta, rtn.w_quantizer.delta), (ao.w_quantizer.zero_point, rtn.w_quantizer.zero_point)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert ao.int_weight.shape == rtn.int_weight.shape and ao.int_weight.dtype == rtn.int_weight.dtype
    assert not torch.equal(ao.int_weight, rtn.int_weight) and not torch.equal(ao.int_weight, plain.int_weight)
    assert torch.equal(ao.weight.data, _unpermuted_deq(ao.int_weight, ao.w_quantizer, N, K))
    o_a, o_r = gptq.objective(fp.weight.data, ao.weight.data, H).sum(), gptq.objective(fp.weight.data, rtn.weight.data, H).sum()
    assert o_a < o_r
    again, _ = _layer({"weight": W4G, "gptq": dict(GPTQ, act_order=True)}, N, K)
    again.set_codes_(ao._codes.clone())  # simulation mode reads an act_order checkpoint's codes as any GPTQ checkpoint's
    assert torch.equal(again.int_weight, ao.int_weight) and torch.equal(again.weight.data, ao.weight.data)
