"""CPU-only checks of the W4A4 MXFP4 Linears (e2m1 activations against e2m1 weights, optionally behind a 32-point block Hadamard
rotation): the two C entries (wanq_gemm_mx4, wanq_quant_rows_mx_had32) are declared, exported and prototyped and refuse what the header
says, in its order, and qgemm.mx4_linear_refusal agrees; the host definition of the rotation (mx_hadamard32_host) is the Sylvester
matrix product and, bit for bit, a literal five-stage loop; `had32=False` leaves mx_quant_rows_host as it was; the identity
(x H)(w H / 32)^T = x w^T holds exactly through both quantisers where nothing rounds; the outlier block the rotation exists for; the
config pair and the `mx:` section, their refusals, the three refusals tests/test_mx_abi.py pins; kernel mode's dispatch and late-GELU
rule for the new activation forms; the rotation record of the integer checkpoint.
The kernels themselves: tests/test_gpu_mx4.py."""
import ctypes
import os
import re

import pytest
import torch

from test_fp8_abi import BF16, F32, HEADER, I32, PKG, WANQ_E_ARG, WANQ_E_SHAPE, WANQ_OK, i, i64, lib, p, vp  # noqa: F401 (fixtures)
from test_mx_abi import YAML4, YAML8, _cfg, _layer

YAML44 = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_all_linears.yaml")
YAML44H = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_had32_all_linears.yaml")
FP8, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"
GEMM4, QUANTH = "wanq_gemm_mx4", "wanq_quant_rows_mx_had32"
ARGTYPES = {GEMM4: [vp, vp, vp, vp, vp, i, vp, i, vp, vp, i, i64, i, i, vp], QUANTH: [vp, i, vp, vp, i64, i, i, i, vp]}


def gemm4(lib, ptr, **kw):
    """wanq_gemm_mx4 on a well-formed [8, 128] x [16, 128] problem, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, sa=ptr, sw=ptr, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0, M=8, N=16,
             K=128)
    a.update(kw)
    fn = getattr(lib, GEMM4)
    fn.argtypes = ARGTYPES[GEMM4]
    rc = fn(a["a"], a["w"], a["sa"], a["sw"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"], a["epi"],
            a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def quanth(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=F32, q=ptr, scale=ptr, rows=4, cols=64, fmt=1, act=0)
    a.update(kw)
    fn = getattr(lib, QUANTH)
    fn.argtypes = ARGTYPES[QUANTH]
    return fn(a["x"], a["x_dtype"], a["q"], a["scale"], a["rows"], a["cols"], a["fmt"], a["act"], None), lib.wanq_last_error()


# ---- entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first", [(GEMM4, ["const uint8_t* a", "const uint8_t* w", "const uint8_t* sa_u8", "const uint8_t* sw_u8"]),
                                        (QUANTH, ["const void* x", "int x_dtype", "uint8_t* q", "uint8_t* scale_u8"])])
def test_entries_are_declared_exported_and_prototyped(lib, name, first):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES[name]) and params[:4] == first, params
    assert hasattr(lib, name), f"{name} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert name in _C.PROTOTYPES and list(_C.PROTOTYPES[name]) == ARGTYPES[name]
    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6


def test_gemm_refusals_in_the_headers_order(lib, p):
    for name in ("a", "w", "sa", "sw", "out"):
        rc, msg = gemm4(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and GEMM4.encode() in msg and b"must be non-NULL" in msg, (name, rc, msg)
    rc, msg = gemm4(lib, p[0], out_dtype=I32)
    assert rc == WANQ_E_ARG and b"out dtype 3" in msg, (rc, msg)
    rc, msg = gemm4(lib, p[0], bias=p[0], bias_dtype=I32)
    assert rc == WANQ_E_ARG and b"bias dtype 3" in msg, (rc, msg)
    rc, msg = gemm4(lib, p[0], epi=4)
    assert rc == WANQ_E_ARG and b"unknown epilogue flag" in msg, (rc, msg)
    rc, msg = gemm4(lib, p[0], epi=2)
    assert rc == WANQ_E_ARG and b"needs gate and residual" in msg, (rc, msg)
    for M in (-1, 1 << 31):
        rc, msg = gemm4(lib, p[0], M=M)
        assert rc == WANQ_E_SHAPE and b"M=%d" % M in msg and b"out of range" in msg, (rc, msg)
    for N in (12, 4, 0):
        rc, msg = gemm4(lib, p[0], N=N)
        assert rc == WANQ_E_SHAPE and b"N=%d" % N in msg and b"multiple of 8" in msg, (rc, msg)
    for K in (0, 32, 64, 96, 192, 100, -128):
        rc, msg = gemm4(lib, p[0], K=K)
        assert rc == WANQ_E_SHAPE and GEMM4.encode() in msg and b"K=%d" % K in msg and b"multiple of 128" in msg, (rc, msg)
    off = lambda n: ctypes.c_void_p(p[0].value + n)  # noqa: E731
    for name in ("a", "w", "out"):
        rc, msg = gemm4(lib, p[0], **{name: off(8)})
        assert rc == WANQ_E_ARG and b"16-byte aligned" in msg, (name, rc, msg)
    for name in ("sa", "sw"):
        rc, msg = gemm4(lib, p[0], **{name: off(2)})
        assert rc == WANQ_E_ARG and b"sa_u8 and sw_u8 must be 4-byte aligned" in msg, (name, rc, msg)
    rc, msg = gemm4(lib, p[0], bias=off(4), bias_dtype=F32)
    assert rc == WANQ_E_ARG and b"aligned to 4 elements" in msg, (rc, msg)
    rc, msg = gemm4(lib, p[0], M=(1 << 31) - 256, N=128 * 256)
    assert rc == WANQ_E_SHAPE and b"too many tiles" in msg, (rc, msg)
    # the order: N before K, K before the alignment, the tile count last
    assert b"N=12" in gemm4(lib, p[0], N=12, K=64)[1] and b"K=64" in gemm4(lib, p[0], K=64, a=off(8))[1]
    assert gemm4(lib, p[0], M=0)[0] == WANQ_OK  # nothing to do, nothing launched


def test_python_refusal_text_agrees_with_the_c_entry(lib, p):
    from viditq_extension import qgemm

    cases = [(8, 16, 128), (1, 8, 128), (8, 16, 64), (8, 16, 96), (8, 16, 192), (8, 12, 128), (8, 12, 64), (8, 0, 128), (8, 16, 0),
             (-1, 12, 64), ((1 << 31) - 256, 128 * 256, 128), (1 << 31, 16, 128), (32760, 8960, 1536), (32760, 1536, 8960), (75600, 5120, 13824)]
    for M, N, K in cases:
        why = qgemm.mx4_linear_refusal(M, N, K)
        rc, msg = gemm4(lib, p[0], M=M if why else 0, N=N, K=K)  # (accepted: sent with M = 0)
        assert (why is None) == (rc == WANQ_OK), (M, N, K, why, msg)
        if why is not None:
            assert why.encode() in msg, (why, msg)
    assert "K=64 must be a positive multiple of 128" == qgemm.mx4_linear_refusal(8, 16, 64)
    assert "N=12 must be a positive multiple of 8" == qgemm.mx4_linear_refusal(8, 12, 64)
    assert "M=-1 out of range" == qgemm.mx4_linear_refusal(-1, 12, 64)


def test_rotating_quantiser_refusals_are_the_plain_quantisers(lib, p):
    for name in ("x", "q", "scale"):
        rc, msg = quanth(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and QUANTH.encode() in msg and b"non-NULL" in msg, (name, rc, msg)
    rc, msg = quanth(lib, p[0], x_dtype=I32)
    assert rc == WANQ_E_ARG and b"bad x dtype 3" in msg, (rc, msg)
    for f in (2, -1):
        rc, msg = quanth(lib, p[0], fmt=f)
        assert rc == WANQ_E_ARG and b"fmt=%d" % f in msg, (rc, msg)
    rc, msg = quanth(lib, p[0], act=2)
    assert rc == WANQ_E_ARG and b"act must be 0 or 1" in msg, (rc, msg)
    for cols in (8, 48, 2056):
        rc, msg = quanth(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and QUANTH.encode() in msg and b"cols=%d must be a multiple of 32" % cols in msg, (rc, msg)
    rc, msg = quanth(lib, p[0], q=ctypes.c_void_p(p[0].value + 4))
    assert rc == WANQ_E_ARG and b"q must be 16-byte aligned" in msg, (rc, msg)
    assert quanth(lib, p[0], rows=0)[0] == WANQ_OK and quanth(lib, p[0], rows=0, fmt=0)[0] == WANQ_OK


# ---- the host definition of the rotation --------------------------------------------------------------------------------------------
def sylvester32():
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < 32:
        h = torch.cat((torch.cat((h, h), 1), torch.cat((h, -h), 1)), 0)
    return h


def five_stage_loop(x):
    """the issue's definition, literally: fp32, h = 1, 2, 4, 8, 16, pairs (i, i + h) with bit h of i clear"""
    v = x.float().clone().reshape(-1, 32)
    for h in (1, 2, 4, 8, 16):
        for i in range(32):
            if not i & h:
                a, b = v[:, i].clone(), v[:, i + h].clone()
                v[:, i], v[:, i + h] = a + b, a - b
    return v.reshape(x.shape)


def test_hadamard_host_is_the_sylvester_product_and_the_five_stage_loop():
    from qdiff.base.base_quantizer import mx_hadamard32_host

    H = sylvester32()
    assert torch.equal(H, H.T) and torch.equal(H @ H, 32 * torch.eye(32, dtype=torch.float64))
    assert all(H[i, j].item() == (-1) ** bin(i & j).count("1") for i in range(32) for j in range(32))
    g = torch.Generator().manual_seed(1)
    xi = torch.randint(-50, 51, (5, 96), generator=g).float()
    got = mx_hadamard32_host(xi)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 96)
    assert torch.equal(got.double(), (xi.double().view(5, 3, 32) @ H).view(5, 96))
    xr = torch.randn(7, 160, generator=g) * (10.0 ** torch.arange(-3, 4).float())[:, None]
    assert torch.equal(mx_hadamard32_host(xr), five_stage_loop(xr))
    assert torch.equal(mx_hadamard32_host(xr.to(torch.bfloat16)), five_stage_loop(xr.to(torch.bfloat16).float()))
    with pytest.raises(ValueError, match="cols=48"):
        mx_hadamard32_host(torch.zeros(2, 48))


def _todays_mx_quant_rows_host(x, fmt, gelu=False):
    """mx_quant_rows_host as it stood before `had32` existed, restated"""
    from qdiff.base.base_quantizer import _pow2_f64, mx_pack_e2m1

    emax, vmax = (8, 448.0) if fmt == FP8 else (2, 6.0)
    x = x.float()
    if gelu:
        x = torch.nn.functional.gelu(x, approximate="tanh")
    rows, cols = x.shape
    xb = x.reshape(rows, cols // 32, 32)
    amax = xb.abs().amax(dim=-1).contiguous()
    s = (((amax.view(torch.int32) >> 23) & 0xff) - emax).clamp(0, 254)
    t = (xb.double() * _pow2_f64(127 - s).unsqueeze(-1)).clamp(-vmax, vmax).reshape(rows, cols)
    if fmt == FP8:
        return t.float().to(torch.float8_e4m3fn).view(torch.uint8), s.to(torch.uint8)
    a = t.abs()
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)).to(torch.uint8)
    return mx_pack_e2m1(mag | (torch.signbit(t).to(torch.uint8) << 3)), s.to(torch.uint8)


@pytest.mark.parametrize("fmt", [FP8, FP4])
def test_without_the_rotation_the_host_quantiser_is_todays(fmt):
    from qdiff.base.base_quantizer import mx_hadamard32_host, mx_quant_rows_host

    g = torch.Generator().manual_seed(2)
    x = torch.randn(9, 192, generator=g) * (10.0 ** torch.arange(-4, 5).float())[:, None]
    x[3] = 0
    x[:, 40] *= 100
    for gelu in (False, True):
        want = _todays_mx_quant_rows_host(x, fmt, gelu)
        for got in (mx_quant_rows_host(x, fmt, gelu), mx_quant_rows_host(x, fmt, gelu, False), mx_quant_rows_host(x, fmt, gelu, had32=False)):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        # had32=True: the same quantiser on the rotated (post-GELU) row
        pre = torch.nn.functional.gelu(x, approximate="tanh") if gelu else x
        want = _todays_mx_quant_rows_host(mx_hadamard32_host(pre), fmt)
        got = mx_quant_rows_host(x, fmt, gelu, had32=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_identity_is_exact_where_nothing_rounds():
    """x and w constant inside every block, values c in +-{0, 1, 2, 3, 4, 6}: a block rotates to (32 c, 0, ..., 0), the weight's (as
    w / 32) to (c, 0, ..., 0), and both are an e2m1 value times a power of two, so both quantisers are exact and the decoded
    product of the ROTATED operands equals x w^T of the original ones"""
    from qdiff.base.base_quantizer import mx_decode, mx_quant_rows_host

    g = torch.Generator().manual_seed(3)
    vals = torch.tensor([0.0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6])
    M, N, nb = 6, 8, 5
    x = vals[torch.randint(0, 11, (M, nb), generator=g)].repeat_interleave(32, dim=1)
    w = vals[torch.randint(0, 11, (N, nb), generator=g)].repeat_interleave(32, dim=1)
    xq, xs = mx_quant_rows_host(x, FP4, had32=True)
    wq, ws = mx_quant_rows_host(w * 0.03125, FP4, had32=True)
    xd, wd = mx_decode(xq, xs, FP4, torch.float64), mx_decode(wq, ws, FP4, torch.float64)
    assert torch.equal(xd.view(M, nb, 32)[:, :, 0], 32 * x.double().view(M, nb, 32)[:, :, 0]) and not bool(xd.view(M, nb, 32)[:, :, 1:].any())
    assert torch.equal(wd.view(N, nb, 32)[:, :, 0], w.double().view(N, nb, 32)[:, :, 0])
    want = x.double() @ w.double().T
    assert bool(want.any()) and torch.equal(xd @ wd.T, want)


def test_the_outlier_block_is_what_the_rotation_is_for():
    """[8, 0.3 x 31].  Unrotated: scale 2, 8 -> code 4 (exact), 0.15 -> 0: all 31 small values lost, squared error 31 x 0.09 = 2.79.
    Rotated: [17.3, 7.7 x 31], scale 4, codes decode to 16 and 8: squared error 1.3^2 + 31 x 0.3^2 = 4.48 there, / 32 = 0.14 in the
    original domain (x_hat = x_hat_rot H / 32)"""
    from qdiff.base.base_quantizer import mx_decode, mx_hadamard32_host, mx_quant_rows_host

    x = torch.full((1, 32), 0.3)
    x[0, 0] = 8.0
    q, s = mx_quant_rows_host(x, FP4)
    plain = mx_decode(q, s, FP4, torch.float64)
    assert s.item() == 128 and plain[0, 0].item() == 8.0 and not bool(plain[0, 1:].any())
    e_plain = ((plain - x.double()) ** 2).sum().item()
    rot = mx_hadamard32_host(x)
    assert abs(rot[0, 0].item() - 17.3) < 1e-5 and float((rot[0, 1:] - 7.7).abs().max()) < 1e-5
    q, s = mx_quant_rows_host(x, FP4, had32=True)
    dec = mx_decode(q, s, FP4, torch.float64)
    assert s.item() == 129 and dec[0, 0].item() == 16.0 and bool((dec[0, 1:] == 8.0).all())
    back = dec @ sylvester32() / 32
    e_rot = ((back - x.double()) ** 2).sum().item()
    assert abs(e_plain - 2.79) < 0.01 and abs(e_rot - 0.14) < 0.01, (e_plain, e_rot)
    assert 4 * e_rot <= e_plain


# ---- config -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,had", [(YAML44, False), (YAML44H, True)])
def test_both_shipped_configs_load_and_build_an_mx_layer_in_host_memory(path, had):
    from qdiff.base.base_quantizer import MxQuantizer, mx_decode, mx_quant_rows_host

    cfg = _cfg(path)
    assert cfg.weight.format == FP4 and cfg.act.format == FP4 and cfg.weight.n_bits == 4 and cfg.act.n_bits == 4
    assert cfg.weight.sym is True and cfg.act.sym is True
    assert (cfg.get("mx") is not None and cfg.mx.block_hadamard is True) if had else cfg.get("mx") is None
    ql = _layer(cfg, K=192, N=24)
    assert ql.kind == "mx" and ql.mx == FP4 and ql.mx_act == FP4 and ql.mx_had32 is had and not ql.fp8 and ql.group_size is None
    assert isinstance(ql.w_quantizer, MxQuantizer) and isinstance(ql.a_quantizer, MxQuantizer)
    assert ql.w_quantizer.had32 is had and ql.a_quantizer.had32 is had and ql.w_quantizer.weight_side and not ql.a_quantizer.weight_side
    w = ql.fp_module.weight.data
    wc, ws = mx_quant_rows_host(w * 0.03125, FP4, had32=True) if had else mx_quant_rows_host(w, FP4)
    assert torch.equal(ql._codes, wc) and torch.equal(ql.w_quantizer.scale_u8, ws) and tuple(wc.shape) == (24, 96)
    wdq = mx_decode(wc, ws, FP4)
    assert torch.equal(ql.weight.data, wdq)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 37, 192, generator=g)
    x[:, :, 7] *= 30
    aq, as_ = mx_quant_rows_host(x.view(-1, 192), FP4, had32=had)
    want = torch.nn.functional.linear(mx_decode(aq, as_, FP4), wdq, ql.bias.detach().float()).view(2, 37, 24)
    got = ql(x)
    assert torch.equal(got, want)
    fpy = ql.fp_module(x)
    rel = ((got - fpy).norm() / fpy.norm()).item()
    assert rel < 0.35, rel       # one mantissa bit on both sides (W4A8-MXFP4 alone: below 0.25, tests/test_mx_abi.py)
    ql = _layer(_cfg(path, weight__group_size=32), K=192, N=24)
    assert ql.mx_act == FP4 and ql.group_size is None


def test_the_rotation_helps_a_layer_with_an_outlier_channel():
    """the same layer and input under both configs: with one input channel 30 x the rest, the rotated layer is the closer one"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(64, 192, generator=g)
    x[:, 7] *= 30
    rel = {}
    for path in (YAML44, YAML44H):
        ql = _layer(_cfg(path), K=192, N=24)
        fpy = ql.fp_module(x)
        rel[path] = ((ql(x) - fpy).norm() / fpy.norm()).item()
    assert rel[YAML44H] < rel[YAML44], rel


def test_new_and_pinned_refusals_name_the_layer_and_the_key():
    from qdiff import config as qcfg

    L = r"blocks\.0\.ffn\.0: "
    # the three refusals tests/test_mx_abi.py pins, with its regexes
    for path in (YAML8, YAML4):
        with pytest.raises(NotImplementedError, match=L + r"act\.format: mxfp4_e2m1.*no fp4 activation quantiser path is built yet"):
            _layer(_cfg(path, act__format=FP4))                                   # 8-bit codes
    with pytest.raises(NotImplementedError, match=L + r"act\.format: mxfp4_e2m1.*no fp4 activation quantiser path is built yet"):
        _layer(_cfg(YAML8, act__format=FP4, act__n_bits=4))                       # against an mxfp8_e4m3 weight
    with pytest.raises(NotImplementedError, match=L + r"act\.format: mxfp4_e2m1.*no fp4 activation"):
        _layer(_cfg(YAML8, weight__format="fp8_e4m3", act__format=FP4))           # against an fp8_e4m3 weight
    with pytest.raises(NotImplementedError, match=L + r"act\.format: mxfp4_e2m1.*no fp4 activation.*e4m3 weight"):
        _layer(_cfg(YAML8, weight__format="fp8_e4m3", act__format=FP4, act__n_bits=4))
    # the W4A4 pair's own section rules
    for edits, rx in (({"act__n_bits": 8}, r"act\.format: mxfp4_e2m1 with act\.n_bits: 8.*8-bit codes"),
                      ({"weight__n_bits": 8}, r"weight\.format: mxfp4_e2m1 needs weight\.n_bits: 4 \(it is 8\)"),
                      ({"act__sym": False}, r"act\.format.*act\.sym: True"),
                      ({"act__n_bits": qcfg.ListConfig([4, 8])}, r"act\.format with a bit-width list"),
                      ({"weight__format": None}, r"an MX format on one side.*weight\.format is None"),
                      ({"weight__group_size": 64}, r"weight\.format: mxfp4_e2m1 with weight\.group_size=64.*32 input channels")):
        with pytest.raises(NotImplementedError, match=L + rx):
            _layer(_cfg(YAML44, **edits))
    # mx.block_hadamard: only with the W4A4 pair
    on = qcfg.create({"block_hadamard": True})
    for path in (YAML8, YAML4):
        cfg = _cfg(path)
        cfg["mx"] = on
        with pytest.raises(NotImplementedError, match=L + r"mx\.block_hadamard: True is not supported with weight\.format.*W4A4 pair only"):
            _layer(cfg)
    for path in ("w8a8_all_linears.yaml", "w8a8_fp8_all_linears.yaml", "w4a16_all_linears.yaml"):
        cfg = _cfg(os.path.join(PKG, "quant_configs", path))
        cfg["mx"] = on
        with pytest.raises(NotImplementedError, match=L + r"mx\.block_hadamard: True is not supported with no MX format"):
            _layer(cfg, K=128)
    cfg = _cfg(YAML44)
    cfg["mx"] = qcfg.create({"block_hadamard": 1})
    with pytest.raises(ValueError, match=L + r"mx\.block_hadamard=1 must be True or False"):
        _layer(cfg)
    cfg["mx"] = qcfg.create({"hadamard": True})
    with pytest.raises(ValueError, match=L + r"mx\.hadamard is not a known key"):
        _layer(cfg)
    cfg["mx"] = qcfg.create({"block_hadamard": False})
    assert _layer(cfg).mx_had32 is False
    # GPTQ still refuses an MX layer
    cfg = _cfg(YAML44)
    cfg["gptq"] = qcfg.create({"layer_name_regex": "ffn"})
    with pytest.raises(NotImplementedError, match=L + r"gptq with weight\.format='mxfp4_e2m1'"):
        _layer(cfg)


# ---- kernel mode: dispatch ------------------------------------------------------------------------------------------------------------
def test_kernel_mode_layer_forms_and_the_late_gelu_rule():
    from wan.quant_wanx_hip import _ROW_QUANTISERS, HipLinearMx, _late_gelu, _to_hip_linear

    def mx(w_fmt=FP4, a_fmt=FP4, had32=False):
        return HipLinearMx(128, 256, True, w_fmt, "blocks.0.ffn.0", a_fmt, had32)

    a8w8, a8w4, a4, a4h = mx(FP8, FP8), mx(FP4, FP8), mx(), mx(had32=True)
    assert [m.act_form for m in (a8w8, a8w4, a4, a4h)] == ["mxfp8", "mxfp8", "mxfp4", "mxfp4_h32"]
    assert all(m.act_key == m.act_form and m.plain_rows and m.sharded == ("weight", "scale_weight") for m in (a8w8, a8w4, a4, a4h))
    assert {"mxfp4", "mxfp4_h32"} <= set(_ROW_QUANTISERS)
    assert _late_gelu(a4, mx()) and _late_gelu(a4h, mx(had32=True)) and _late_gelu(a8w4, a8w8)
    assert not _late_gelu(a4, a4h) and not _late_gelu(a4h, a4)
    assert not _late_gelu(a8w4, a4) and not _late_gelu(a4, a8w4) and not _late_gelu(a8w8, a4h)
    assert sorted(k for k, _ in a4.named_buffers()) == ["bias", "scale_weight", "weight"]
    assert sorted(k for k, _ in a4h.named_buffers()) == ["bias", "mx_had32", "scale_weight", "weight"]
    assert a4h.mx_had32.dtype == torch.uint8 and a4h.mx_had32.tolist() == [1] and tuple(a4.weight.shape) == (256, 64)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: no MX GEMM takes weight mxfp8_e4m3 against act mxfp4_e2m1"):
        mx(FP8, FP4)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: no MX GEMM takes.*behind the block rotation"):
        mx(FP4, FP8, True)
    for path, had in ((YAML44, False), (YAML44H, True)):
        ql = _layer(_cfg(path), K=256, N=24)
        hl = _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
        assert isinstance(hl, HipLinearMx) and hl.mx == FP4 and hl.a_fmt == FP4 and hl.had32 is had
        assert hl.act_key == ("mxfp4_h32" if had else "mxfp4") and not hl.quantized and not hl.fp8
        assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.scale_u8)
        with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: format: mxfp4_e2m1 has no kernel-mode form.*K=192 must be"):
            _to_hip_linear(_layer(_cfg(path), K=192, N=24), None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")


def test_forward_picks_the_gemm_by_the_activation_format(monkeypatch):
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import HipLinearMx

    calls = []
    monkeypatch.setattr(qgemm, "mx_linear", lambda *a, **k: calls.append("mx_linear"))
    monkeypatch.setattr(qgemm, "mx4_linear", lambda *a, **k: calls.append("mx4_linear"))
    for a_fmt, had in ((FP8, False), (FP4, False), (FP4, True)):
        HipLinearMx(128, 256, True, FP4, "l", a_fmt, had)(None, None)
    assert calls == ["mx_linear", "mx4_linear", "mx4_linear"]


# ---- integer checkpoint -------------------------------------------------------------------------------------------------------------
def test_the_checkpoint_records_the_rotation_and_refuses_the_other_setting(tmp_path):
    from test_mx_abi import _tiny_model
    from wan.quant_wanx_hip import HipLinearMx

    files = {}
    for path in (YAML4, YAML44, YAML44H):
        model = _tiny_model(path)
        files[path] = str(tmp_path / (os.path.basename(path) + ".pt"))
        sd = model.quantize_and_save_weight(files[path])
        assert tuple(sd["blocks.1.ffn.0.weight"].shape) == (256, 64) and tuple(sd["blocks.1.ffn.0.scale_weight"].shape) == (256, 4)
        rec = [k for k in sd if k.endswith(".mx_had32")]
        assert len(rec) == (20 if path == YAML44H else 0) and all(sd[k].dtype == torch.uint8 and sd[k].tolist() == [1] for k in rec)
        fresh = _tiny_model(path).hardware_forward_refactor(load_path=files[path])
        lins = [m for m in fresh.hip_blocks.modules() if isinstance(m, HipLinearMx)]
        assert len(lins) == 20 and all(m.had32 is (path == YAML44H) and m.a_fmt == (FP8 if path == YAML4 else FP4) for m in lins)
        assert torch.equal(fresh.hip_blocks[1].ffn0.weight, sd["blocks.1.ffn.0.weight"])
        assert all(m.sharded == ("weight", "scale_weight") for m in lins)
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q holds codes quantised behind the block Hadamard rotation.*built without it"):
        _tiny_model(YAML44).hardware_forward_refactor(load_path=files[YAML44H])
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q holds codes quantised without the block Hadamard rotation.*built with it"):
        _tiny_model(YAML44H).hardware_forward_refactor(load_path=files[YAML44])
    # the W4A8-MXFP4 layer's buffers and shapes are the W4A4 layer's: an existing checkpoint (no record) loads as unrotated
    _tiny_model(YAML44).hardware_forward_refactor(load_path=files[YAML4])
