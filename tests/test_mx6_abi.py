"""CPU-only checks of the MXFP6 (e2m3) Linears, W6A6 and W4A6: the two C entries (wanq_quant_rows_mx6, wanq_gemm_mx6) are declared,
exported and prototyped, the header still compiles as C99 and the ABI version stays 6; every argument rule returns its code and a
message before anything is launched; qgemm.mx6_linear_refusal agrees with the C entry.  The format is pinned independently of the
host expression: a 64-entry decode table written out from the rule, the quantiser against a brute-force nearest-value search over it
(ties to the even code), the packing against bytes written out by hand.  Two derived properties: an e2m3 row's scale bytes are the
e2m1 quantiser's, and e2m3 is elementwise at least as close as e2m1.  Config side: both shipped configs parse and build a layer of
kind "mx"; every other pairing with the new format is refused by layer name; `mxfp6_e2m3` is still not a known format.
The kernels themselves: tests/test_gpu_mx6.py."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from test_fp8_abi import BF16, F32, HEADER, I32, PKG, WANQ_E_ARG, WANQ_E_SHAPE, WANQ_OK, i, i64, lib, p, vp  # noqa: F401 (fixtures)
from test_mx_abi import YAML4, YAML8, _cfg, _layer, blocks_of

YAML66 = os.path.join(PKG, "quant_configs", "mx", "w6a6_mxfp6_all_linears.yaml")
YAML46 = os.path.join(PKG, "quant_configs", "mx", "w4a6_mxfp4_mxfp6_all_linears.yaml")
YAML44 = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_all_linears.yaml")
FP8, FP6, FP4 = "mxfp8_e4m3", "mxfp6_e2m3fn", "mxfp4_e2m1"
GEMM6, QUANT6 = "wanq_gemm_mx6", "wanq_quant_rows_mx6"
ARGTYPES = {GEMM6: [vp, vp, vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp], QUANT6: [vp, i, vp, vp, i64, i, i, vp]}
# value of every 6-bit code, from the rule: sign in bit 5, E in bits 3-4 (bias 1), M in bits 0-2; E = 0: M / 8; E > 0: 2^(E - 1) (1 + M / 8)
MAGS = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875,
        1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
        2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75,
        4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5]
TABLE = MAGS + [-v for v in MAGS]


def gemm6(lib, ptr, **kw):
    """wanq_gemm_mx6 on a well-formed [8, 128] x [16, 128] problem, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, sa=ptr, sw=ptr, w_fmt=2, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0,
             M=8, N=16, K=128)
    a.update(kw)
    fn = getattr(lib, GEMM6)
    fn.argtypes = ARGTYPES[GEMM6]
    rc = fn(a["a"], a["w"], a["sa"], a["sw"], a["w_fmt"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"],
            a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def quant6(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=F32, q=ptr, scale=ptr, rows=4, cols=64, act=0)
    a.update(kw)
    fn = getattr(lib, QUANT6)
    fn.argtypes = ARGTYPES[QUANT6]
    return fn(a["x"], a["x_dtype"], a["q"], a["scale"], a["rows"], a["cols"], a["act"], None), lib.wanq_last_error()


# ---- entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first", [(GEMM6, ["const uint8_t* a", "const uint8_t* w", "const uint8_t* sa_u8", "const uint8_t* sw_u8"]),
                                        (QUANT6, ["const void* x", "int x_dtype", "uint8_t* q", "uint8_t* scale_u8"])])
def test_entries_are_declared_exported_and_prototyped(lib, name, first):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES[name]) and params[:4] == first, params
    assert hasattr(lib, name), f"{name} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert name in _C.PROTOTYPES and list(_C.PROTOTYPES[name]) == ARGTYPES[name]
    assert _C.MX6_FMT == {FP6: 2, FP4: 1} and re.search(r"WANQ_MX_E4M3 = 0, WANQ_MX_E2M1 = 1, WANQ_MX_E2M3 = 2", src)
    assert lib.wanq_abi_version() == 6 and _C.ABI_VERSION == 6


def test_header_still_compiles_as_c99_and_the_abi_version_stays_6(lib, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return (int)(sizeof(&%s) + sizeof(&%s) == 0) + WANQ_MX_E2M3; }\n' % (GEMM6, QUANT6))
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert lib.wanq_abi_version() == 6


# ---- refusals of the C entries ----------------------------------------------------------------------------------------------------
def test_gemm_refusals_in_the_headers_order(lib, p):
    for name in ("a", "w", "sa", "sw", "out"):
        rc, msg = gemm6(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and GEMM6.encode() in msg and b"must be non-NULL" in msg, (name, rc, msg)
    for f in (0, 3, -1):
        rc, msg = gemm6(lib, p[0], w_fmt=f)
        assert rc == WANQ_E_ARG and b"w_fmt=%d" % f in msg and b"WANQ_MX_E2M3 or WANQ_MX_E2M1" in msg, (rc, msg)
    rc, msg = gemm6(lib, p[0], out_dtype=I32)
    assert rc == WANQ_E_ARG and b"out dtype 3" in msg, (rc, msg)
    rc, msg = gemm6(lib, p[0], bias=p[0], bias_dtype=I32)
    assert rc == WANQ_E_ARG and b"bias dtype 3" in msg, (rc, msg)
    rc, msg = gemm6(lib, p[0], epi=4)
    assert rc == WANQ_E_ARG and b"unknown epilogue flag" in msg, (rc, msg)
    rc, msg = gemm6(lib, p[0], epi=2)
    assert rc == WANQ_E_ARG and b"needs gate and residual" in msg, (rc, msg)
    for M in (-1, 1 << 31):
        rc, msg = gemm6(lib, p[0], M=M)
        assert rc == WANQ_E_SHAPE and b"M=%d" % M in msg and b"out of range" in msg, (rc, msg)
    for N in (12, 4, 0):
        rc, msg = gemm6(lib, p[0], N=N)
        assert rc == WANQ_E_SHAPE and b"N=%d" % N in msg and b"multiple of 8" in msg, (rc, msg)
    for w_fmt in (2, 1):
        for K in (0, 32, 64, 96, 192, 100, -128):
            rc, msg = gemm6(lib, p[0], K=K, w_fmt=w_fmt)
            assert rc == WANQ_E_SHAPE and GEMM6.encode() in msg and b"K=%d" % K in msg and b"multiple of 128" in msg, (rc, msg)
    off = lambda n: ctypes.c_void_p(p[0].value + n)  # noqa: E731
    for name in ("a", "w", "out"):
        rc, msg = gemm6(lib, p[0], **{name: off(8)})
        assert rc == WANQ_E_ARG and b"16-byte aligned" in msg, (name, rc, msg)
    rc, msg = gemm6(lib, p[0], epi=2, gate=p[0], residual=off(8))
    assert rc == WANQ_E_ARG and b"16-byte aligned" in msg, (rc, msg)
    for name in ("sa", "sw"):
        rc, msg = gemm6(lib, p[0], **{name: off(2)})
        assert rc == WANQ_E_ARG and b"sa_u8 and sw_u8 must be 4-byte aligned" in msg, (name, rc, msg)
    rc, msg = gemm6(lib, p[0], bias=off(4), bias_dtype=F32)
    assert rc == WANQ_E_ARG and b"aligned to 4 elements" in msg, (rc, msg)
    rc, msg = gemm6(lib, p[0], M=(1 << 31) - 256, N=128 * 256)
    assert rc == WANQ_E_SHAPE and b"too many tiles" in msg, (rc, msg)
    assert b"N=12" in gemm6(lib, p[0], N=12, K=64)[1] and b"K=64" in gemm6(lib, p[0], K=64, a=off(8))[1]
    assert gemm6(lib, p[0], M=0)[0] == WANQ_OK and gemm6(lib, p[0], M=0, w_fmt=1)[0] == WANQ_OK  # nothing to do, nothing launched


def test_quantiser_refusals(lib, p):
    for name in ("x", "q", "scale"):
        rc, msg = quant6(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and QUANT6.encode() in msg and b"non-NULL" in msg, (name, rc, msg)
    rc, msg = quant6(lib, p[0], x_dtype=I32)
    assert rc == WANQ_E_ARG and b"bad x dtype 3" in msg, (rc, msg)
    for act in (2, -1):
        rc, msg = quant6(lib, p[0], act=act)
        assert rc == WANQ_E_ARG and b"act must be 0 or 1" in msg, (rc, msg)
    for cols in (0, 12, 16392, 16416):
        rc, msg = quant6(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and QUANT6.encode() in msg and b"cols=%d" % cols in msg, (rc, msg)
    for cols in (8, 48, 2056):
        rc, msg = quant6(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and b"cols=%d must be a multiple of 32" % cols in msg, (rc, msg)
    rc, msg = quant6(lib, p[0], q=ctypes.c_void_p(p[0].value + 4))
    assert rc == WANQ_E_ARG and b"q must be 16-byte aligned" in msg, (rc, msg)
    assert quant6(lib, p[0], rows=0)[0] == WANQ_OK


def test_python_refusal_text_agrees_with_the_c_entry(lib, p):
    from viditq_extension import qgemm

    cases = [(8, 16, 128), (1, 8, 128), (8, 16, 64), (8, 16, 96), (8, 16, 192), (8, 12, 128), (8, 0, 128), (8, 16, 0),
             ((1 << 31) - 256, 128 * 256, 128), (1 << 31, 16, 128), (32760, 8960, 1536), (32760, 1536, 8960), (75600, 5120, 13824)]
    for w_fmt in (FP6, FP4):
        for M, N, K in cases:
            why = qgemm.mx6_linear_refusal(M, N, K, w_fmt)
            rc, msg = gemm6(lib, p[0], M=M if why else 0, N=N, K=K, w_fmt=2 if w_fmt == FP6 else 1)  # (accepted: sent with M = 0)
            assert (why is None) == (rc == WANQ_OK), (M, N, K, why, msg)
            if why is not None:
                assert why.encode() in msg, (why, msg)
    assert "K=64 must be a positive multiple of 128" == qgemm.mx6_linear_refusal(8, 16, 64, FP4)
    assert "w_fmt='mxfp8_e4m3'" in qgemm.mx6_linear_refusal(8, 16, 128, FP8)


# ---- the format, independently of the host expression ---------------------------------------------------------------------------------
def host(x, fmt=FP6, gelu=False):
    from qdiff.base.base_quantizer import mx_quant_rows_host

    return mx_quant_rows_host(x, fmt, gelu)


def nearest_code(t):
    """brute force over the decode table: the magnitude code nearest to min(|t|, 7.5), a tie to the even code; the sign bit of t"""
    a = min(abs(t), 7.5)
    d = min(abs(a - v) for v in MAGS)
    best = [c for c, v in enumerate(MAGS) if abs(a - v) == d]
    c = best[0] if len(best) == 1 else [c for c in best if c % 2 == 0][0]
    return c | (32 if math.copysign(1.0, t) < 0 else 0)


def test_decode_table_and_the_spec_constants():
    from qdiff.base.base_quantizer import _MX_SPEC, E2M3_VALUES, MX_FORMATS, mx_decode, mx_fmt_code, mx_pack_e2m3

    assert len(TABLE) == 64 and MAGS == sorted(MAGS) and len(set(MAGS)) == 32 and max(MAGS) == 7.5
    assert all(MAGS[c] == ((c & 7) / 8 if c < 8 else 2.0 ** ((c >> 3) - 1) * (1 + (c & 7) / 8)) for c in range(32))
    assert list(E2M3_VALUES) == MAGS and _MX_SPEC[FP6][:2] == (2, 7.5) and mx_fmt_code(FP6) == 2 and FP6 in MX_FORMATS
    codes = mx_pack_e2m3(torch.arange(64, dtype=torch.uint8)[None])
    dec = mx_decode(codes, torch.tensor([[127, 128]], dtype=torch.uint8), FP6, torch.float64)[0]
    assert dec[:32].tolist() == TABLE[:32] and dec[32:].tolist() == [2 * v for v in TABLE[32:]]
    assert math.copysign(1.0, dec[32].item()) == -1.0     # code 32 is -0


def test_quantiser_against_the_nearest_value_search_over_the_table():
    """blocks pinned at 7.5 (E = 129, s = 127, scale 2^0): every grid point, every midpoint between neighbouring codes and its fp32
    neighbours, on both signs, +-0, values in (7.5, 8); then blocks whose amax sits on a binade edge and one ulp either side"""
    from qdiff.base.base_quantizer import mx_unpack_e2m3

    vals = [0.0, -0.0]
    for sign in (1.0, -1.0):
        for c, v in enumerate(MAGS):
            vals.append(sign * v)
            if c + 1 < 32:
                mid = torch.tensor((v + MAGS[c + 1]) / 2)
                vals += [sign * mid.item(), sign * torch.nextafter(mid, torch.zeros(())).item(), sign * torch.nextafter(mid, mid * 2).item()]
        vals += [sign * 7.51, sign * 7.75, sign * torch.nextafter(torch.tensor(8.0), torch.zeros(())).item()]
    x = blocks_of(vals, 7.5)
    codes, s = host(x)
    assert tuple(codes.shape) == (1, x.shape[1] // 4 * 3) and codes.dtype == torch.uint8 and set(s.view(-1).tolist()) == {127}
    got = mx_unpack_e2m3(codes).view(-1, 32)
    assert got[:, 0].tolist() == [31] * got.shape[0]
    got = got[:, 1:].reshape(-1)[:len(vals)].tolist()
    want = [nearest_code(v) for v in vals]
    assert got == want, [(vals[j], got[j], want[j]) for j in range(len(vals)) if got[j] != want[j]][:8]
    assert set(want) == set(range(64))
    # amax on a binade edge: the scale byte steps AT the power of two, and the codes follow the scaled values
    one = torch.tensor(1.0)
    for pin in (torch.nextafter(one, one * 0).item(), 1.0, torch.nextafter(one, one * 2).item(), 4.0, torch.nextafter(one * 4, one).item(),
                2.0 ** -126, 2.0 ** -130, 2.0 ** 127 * 1.5):
        b = torch.zeros(1, 32)
        b[0, 0], b[0, 1], b[0, 2], b[0, 3] = pin, -pin / 2, pin * 0.3, pin * 0.47
        codes, s = host(b)
        E = 0 if pin < 2.0 ** -126 else math.frexp(pin)[1] - 1 + 127
        sb = min(254, max(0, E - 2))
        assert s.tolist() == [[sb]], (pin, s)
        assert mx_unpack_e2m3(codes)[0].tolist() == [nearest_code(math.ldexp(v, 127 - sb)) for v in b[0].double().tolist()], pin


def test_pack_round_trips_and_a_block_of_codes_0_to_31_is_these_24_bytes():
    from qdiff.base.base_quantizer import mx_pack_e2m3, mx_unpack_e2m3

    # codes 0 .. 31 at bits 6 j .. 6 j + 5 of a little-endian string: four codes a, b, c, d make the bytes a | b << 6, b >> 2 | c << 4,
    # c >> 4 | d << 2 -- worked out by hand for the eight groups
    by_hand = [0x40, 0x20, 0x0c, 0x44, 0x61, 0x1c, 0x48, 0xa2, 0x2c, 0x4c, 0xe3, 0x3c,
               0x50, 0x24, 0x4d, 0x54, 0x65, 0x5d, 0x58, 0xa6, 0x6d, 0x5c, 0xe7, 0x7d]
    assert mx_pack_e2m3(torch.arange(32, dtype=torch.uint8)[None]).tolist() == [by_hand]
    c = (torch.arange(3 * 96) * 37 % 64).to(torch.uint8).view(3, 96)
    pk = mx_pack_e2m3(c)
    assert tuple(pk.shape) == (3, 72) and pk.dtype == torch.uint8 and torch.equal(mx_unpack_e2m3(pk), c)
    for r in range(3):       # bit by bit
        word = sum(int(c[r, k]) << (6 * k) for k in range(96))
        assert pk[r].tolist() == list(word.to_bytes(72, "little"))
    g = torch.Generator().manual_seed(2)
    raw = torch.randint(0, 256, (5, 48), generator=g, dtype=torch.uint8)
    assert torch.equal(mx_pack_e2m3(mx_unpack_e2m3(raw)), raw)


def test_scale_bytes_are_the_e2m1_quantisers_and_e2m3_is_never_further_away():
    """on random fp32 rows: the same emax, so the same scale bytes; the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} is a subset of the e2m3 grid
    under the same scale and 7.5 is nearer than 6 to anything clamped, so |x - deq6(x)| <= |x - deq4(x)| elementwise"""
    from qdiff.base.base_quantizer import mx_decode

    g = torch.Generator().manual_seed(6)
    x = torch.randn(9, 256, generator=g) * (10.0 ** torch.randint(-6, 7, (9, 8), generator=g).float()).repeat_interleave(32, dim=1)
    x[2, 64:96] = 0
    x[:, 77] *= 300
    q6, s6 = host(x, FP6)
    q4, s4 = host(x, FP4)
    assert torch.equal(s6, s4)
    d6, d4 = mx_decode(q6, s6, FP6, torch.float64), mx_decode(q4, s4, FP4, torch.float64)
    e6, e4 = (x.double() - d6).abs(), (x.double() - d4).abs()
    assert bool((e6 <= e4).all()) and bool((e6 < e4).any())


# ---- config ---------------------------------------------------------------------------------------------------------------------
def test_both_new_configs_parse_and_build_a_layer_of_kind_mx():
    from qdiff.base.base_quantizer import MxQuantizer, mx_decode

    for path, wf, bits in ((YAML66, FP6, 6), (YAML46, FP4, 4)):
        cfg = _cfg(path)
        assert cfg.weight.format == wf and cfg.act.format == FP6
        assert cfg.weight.n_bits == bits and cfg.weight.sym is True and cfg.act.n_bits == 6 and cfg.act.sym is True
        ql = _layer(cfg, K=192, N=24)
        assert ql.kind == "mx" and ql.mx == wf and ql.mx_act == FP6 and not ql.fp8 and ql.group_size is None and ql.mx_had32 is False
        assert isinstance(ql.w_quantizer, MxQuantizer) and ql.a_quantizer.format == FP6
        wc, ws = host(ql.fp_module.weight.data, wf)
        assert tuple(ql._codes.shape) == (24, 144 if wf == FP6 else 96) and torch.equal(ql._codes, wc) and torch.equal(ql.w_quantizer.scale_u8, ws)
        assert _layer(_cfg(path, weight__group_size=32)).mx == wf   # the format's own block, spelled out
        # simulation mode in host memory is F.linear on the dequantised operands
        g = torch.Generator().manual_seed(4)
        x = torch.randn(2, 37, 192, generator=g)
        aq, as_ = host(x.view(-1, 192), FP6)
        want = torch.nn.functional.linear(mx_decode(aq, as_, FP6), mx_decode(wc, ws, wf), ql.bias.detach().float()).view(2, 37, 24)
        assert torch.equal(ql(x), want)


def test_every_other_pairing_with_the_new_format_is_refused_by_layer_name():
    from qdiff import config as qcfg

    L = r"blocks\.0\.ffn\.0: "
    for edits, rx in (({"act__format": FP8, "act__n_bits": 8}, L + r"weight\.format: mxfp6_e2m3fn against act\.format: mxfp8_e4m3 is not supported"),
                      ({"act__format": FP4, "act__n_bits": 4}, L + r"weight\.format: mxfp6_e2m3fn against act\.format: mxfp4_e2m1 is not supported"),
                      ({"weight__format": FP8, "weight__n_bits": 8}, L + r"act\.format: mxfp6_e2m3fn against weight\.format: mxfp8_e4m3 is not supported"),
                      ({"weight__format": "fp8_e4m3", "weight__n_bits": 8}, L + r"act\.format: mxfp6_e2m3fn against weight\.format: fp8_e4m3"),
                      ({"act__format": None}, L + r"an MX format on one side.*act\.format is None"),
                      ({"weight__format": None}, L + r"an MX format on one side.*weight\.format is None"),
                      ({"weight__group_size": 64}, L + r"weight\.format: mxfp6_e2m3fn with weight\.group_size=64.*32 input channels"),
                      ({"weight__sym": False}, L + r"weight\.format: mxfp6_e2m3fn needs weight\.sym: True"),
                      ({"act__sym": False}, L + r"act\.format: mxfp6_e2m3fn needs act\.sym: True"),
                      ({"weight__n_bits": 8}, L + r"weight\.format: mxfp6_e2m3fn needs weight\.n_bits: 6 \(it is 8\)"),
                      ({"act__n_bits": 8}, L + r"act\.format: mxfp6_e2m3fn needs act\.n_bits: 6 \(it is 8\)"),
                      ({"act__n_bits": qcfg.ListConfig([4, 6])}, L + r"act\.format with a bit-width list")):
        with pytest.raises(NotImplementedError, match=rx):
            _layer(_cfg(YAML66, **edits))
    with pytest.raises(NotImplementedError, match=L + r"weight\.format: mxfp4_e2m1 needs weight\.n_bits: 4 \(it is 6\)"):
        _layer(_cfg(YAML46, weight__n_bits=6))
    for path in (YAML66, YAML46):
        cfg = _cfg(path)
        cfg["mx"] = qcfg.create({"block_hadamard": True})
        with pytest.raises(NotImplementedError, match=L + r"mx\.block_hadamard: True is not supported with.*mxfp6_e2m3fn.*no rotating e2m3"):
            _layer(cfg)
    with pytest.raises(ValueError, match=L + r"weight\.format: mxfp6_e2m3fn needs in_features=48"):
        _layer(_cfg(YAML66), K=48)


def test_mxfp6_e2m3_without_fn_is_still_not_a_known_format():
    for path in (YAML8, YAML4, YAML66):
        for sec in ("weight", "act"):
            with pytest.raises(ValueError, match=r"blocks\.0\.ffn\.0: " + sec + r"\.format='mxfp6_e2m3' is not a known format.*mxfp6_e2m3fn"):
                _layer(_cfg(path, **{sec + "__format": "mxfp6_e2m3"}))


# ---- kernel mode's layer and the integer checkpoint -----------------------------------------------------------------------------------
def test_kernel_mode_layer_buffers_forms_and_construction_refusals():
    from wan.quant_wanx_hip import HipLinearMx, _to_hip_linear

    for path, wf in ((YAML66, FP6), (YAML46, FP4)):
        ql = _layer(_cfg(path), K=256, N=24)
        hl = _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
        assert isinstance(hl, HipLinearMx) and hl.mx == wf and hl.a_fmt == FP6 and hl.act_form == hl.act_key == "mxfp6" and not hl.had32
        assert sorted(k for k, _ in hl.named_buffers()) == ["bias", "mx_fmt", "scale_weight", "weight"]
        assert hl.mx_fmt.tolist() == [2 if wf == FP6 else 1, 2] and tuple(hl.weight.shape) == (24, 192 if wf == FP6 else 128)
        assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.scale_u8)
        assert hl.sharded == ("weight", "scale_weight")
        with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: format: " + wf + r" has no kernel-mode form.*K=192 must be"):
            _to_hip_linear(_layer(_cfg(path), K=192, N=24), None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: no MX GEMM takes weight mxfp6_e2m3fn against act mxfp8_e4m3"):
        HipLinearMx(256, 24, True, FP6, "blocks.0.ffn.0")
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: no MX GEMM takes weight mxfp8_e4m3 against act mxfp6_e2m3fn"):
        HipLinearMx(256, 24, True, FP8, "blocks.0.ffn.0", FP6)
    with pytest.raises(NotImplementedError, match=r"no MX GEMM takes.*behind the block rotation"):
        HipLinearMx(256, 24, True, FP6, "blocks.0.ffn.0", FP6, True)


@pytest.mark.parametrize("path,wf", [(YAML66, FP6), (YAML46, FP4)])
def test_integer_checkpoint_holds_the_packed_codes_and_records_the_format(tmp_path, path, wf):
    from test_mx_abi import _tiny_model
    from wan.quant_wanx_hip import HipLinearMx

    model = _tiny_model(path)
    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    for base, (N, K) in (("blocks.0.self_attn.q", (128, 128)), ("blocks.1.ffn.0", (256, 128)), ("blocks.1.ffn.2", (128, 256))):
        assert sd[base + ".weight"].dtype == torch.uint8 and tuple(sd[base + ".weight"].shape) == (N, K // 4 * 3 if wf == FP6 else K // 2)
        assert sd[base + ".scale_weight"].dtype == torch.uint8 and tuple(sd[base + ".scale_weight"].shape) == (N, K // 32)
        assert sd[base + ".mx_fmt"].dtype == torch.uint8 and sd[base + ".mx_fmt"].tolist() == [2 if wf == FP6 else 1, 2]
    fresh = _tiny_model(path).hardware_forward_refactor(load_path=file)
    lins = [m for m in fresh.hip_blocks.modules() if isinstance(m, HipLinearMx)]
    assert len(lins) == 20 and all(m.a_fmt == FP6 and m.mx == wf for m in lins)
    assert torch.equal(fresh.hip_blocks[1].ffn2.weight, sd["blocks.1.ffn.2.weight"])
    assert torch.equal(fresh.hip_blocks[1].ffn2.weight, model.get_submodule("blocks.1.ffn.2")._codes)
    # the record decides: a model built under another pair refuses the file by layer name, and an MXFP6 model a file without the record
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved with mx_fmt \[[12], 2\] and the model's layer was built with"):
        _tiny_model(YAML46 if wf == FP6 else YAML44).hardware_forward_refactor(load_path=file)
    _tiny_model(YAML44).quantize_and_save_weight(file)
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved with no mx_fmt"):
        _tiny_model(YAML46).hardware_forward_refactor(load_path=file)
