"""CPU-only checks of the OCP MX Linears (MXFP8 activations against MXFP8 / MXFP4 weights): the two C entries (wanq_quant_rows_mx,
wanq_gemm_mx) are declared, exported and prototyped, the header still compiles as C99 and the ABI version stays 6; every argument rule
returns its code and a message before anything is launched; qgemm.mx_linear_refusal agrees with the C entry.  Python side: both shipped
configs parse; every combination the `format` key does not take is refused by layer name; the host expression of the format
(qdiff/base/base_quantizer.py) is pinned value by value -- every e4m3 code, every e2m1 value and midpoint, the exponent boundary of the
block scale, saturation, the nibble packing; simulation mode in host memory is F.linear on the dequantised operands; the integer
checkpoint of a tiny model reloads bit for bit.
The kernels themselves: tests/test_gpu_mx.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from test_fp8_abi import BF16, F32, HEADER, I32, PKG, WANQ_E_ARG, WANQ_E_SHAPE, WANQ_OK, i, i64, lib, p, vp  # noqa: F401 (fixtures)

YAML8 = os.path.join(PKG, "quant_configs", "w8a8_mxfp8_all_linears.yaml")
YAML4 = os.path.join(PKG, "quant_configs", "w4a8_mxfp4_all_linears.yaml")
FP8, FP4 = "mxfp8_e4m3", "mxfp4_e2m1"
GEMM, QUANT = "wanq_gemm_mx", "wanq_quant_rows_mx"
ARGTYPES = {GEMM: [vp, vp, vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp], QUANT: [vp, i, vp, vp, i64, i, i, i, vp]}


def gemm(lib, ptr, **kw):
    """wanq_gemm_mx on a well-formed [8, 128] x [16, 128] problem, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, sa=ptr, sw=ptr, w_fmt=0, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0,
             M=8, N=16, K=128)
    a.update(kw)
    fn = getattr(lib, GEMM)
    fn.argtypes = ARGTYPES[GEMM]
    rc = fn(a["a"], a["w"], a["sa"], a["sw"], a["w_fmt"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"],
            a["epi"], a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def quant(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=F32, q=ptr, scale=ptr, rows=4, cols=64, fmt=0, act=0)
    a.update(kw)
    fn = getattr(lib, QUANT)
    fn.argtypes = ARGTYPES[QUANT]
    return fn(a["x"], a["x_dtype"], a["q"], a["scale"], a["rows"], a["cols"], a["fmt"], a["act"], None), lib.wanq_last_error()


# ---- entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first", [(GEMM, ["const uint8_t* a", "const uint8_t* w", "const uint8_t* sa_u8", "const uint8_t* sw_u8"]),
                                        (QUANT, ["const void* x", "int x_dtype", "uint8_t* q", "uint8_t* scale_u8"])])
def test_entries_are_declared_exported_and_prototyped(lib, name, first):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES[name]) and params[:4] == first, params
    assert hasattr(lib, name), f"{name} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert name in _C.PROTOTYPES and list(_C.PROTOTYPES[name]) == ARGTYPES[name]
    assert _C.MX_FMT == {FP8: 0, FP4: 1} and re.search(r"WANQ_MX_E4M3 = 0, WANQ_MX_E2M1 = 1", src)


def test_header_still_compiles_as_c99_and_the_abi_version_stays_6(lib, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return (int)(sizeof(&%s) + sizeof(&%s) == 0) + WANQ_MX_E2M1; }\n' % (GEMM, QUANT))
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert lib.wanq_abi_version() == 6


# ---- refusals of the C entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_fmt", [0, 1])
@pytest.mark.parametrize("K", [0, 32, 64, 96, 192, 100, -128])
def test_k_not_a_multiple_of_128_is_refused(lib, p, K, w_fmt):
    rc, msg = gemm(lib, p[0], K=K, w_fmt=w_fmt)
    assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"K=%d" % K in msg and b"multiple of 128" in msg, (rc, msg)


def test_n_m_and_the_tile_count_are_refused(lib, p):
    for N in (12, 4, 0):
        rc, msg = gemm(lib, p[0], N=N)
        assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"N=%d" % N in msg and b"multiple of 8" in msg, (rc, msg)
    for M in (-1, 1 << 31):
        rc, msg = gemm(lib, p[0], M=M)
        assert rc == WANQ_E_SHAPE and b"M=%d" % M in msg and b"out of range" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], M=(1 << 31) - 256, N=128 * 256)
    assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"too many tiles" in msg, (rc, msg)
    assert gemm(lib, p[0], M=0)[0] == WANQ_OK and gemm(lib, p[0], M=0, w_fmt=1)[0] == WANQ_OK  # nothing to do, nothing launched


def test_gemm_arguments_are_refused(lib, p):
    for name in ("a", "w", "sa", "sw", "out"):
        rc, msg = gemm(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and b"must be non-NULL" in msg, (name, rc, msg)
    for f in (2, 4, -1):
        rc, msg = gemm(lib, p[0], w_fmt=f)
        assert rc == WANQ_E_ARG and b"w_fmt=%d" % f in msg and b"WANQ_MX_E4M3 or WANQ_MX_E2M1" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], out_dtype=I32)
    assert rc == WANQ_E_ARG and b"out dtype 3" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], bias=p[0], bias_dtype=I32)
    assert rc == WANQ_E_ARG and b"bias dtype 3" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], epi=4)
    assert rc == WANQ_E_ARG and b"unknown epilogue flag" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], epi=2)
    assert rc == WANQ_E_ARG and b"needs gate and residual" in msg, (rc, msg)
    off = lambda n: ctypes.c_void_p(p[0].value + n)  # noqa: E731
    for name in ("a", "w", "out"):
        rc, msg = gemm(lib, p[0], **{name: off(8)})
        assert rc == WANQ_E_ARG and b"16-byte aligned" in msg, (name, rc, msg)
    rc, msg = gemm(lib, p[0], epi=2, gate=p[0], residual=off(8))
    assert rc == WANQ_E_ARG and b"16-byte aligned" in msg, (rc, msg)
    for name in ("sa", "sw"):
        rc, msg = gemm(lib, p[0], **{name: off(2)})
        assert rc == WANQ_E_ARG and b"sa_u8 and sw_u8 must be 4-byte aligned" in msg, (name, rc, msg)
    rc, msg = gemm(lib, p[0], bias=off(4), bias_dtype=F32)
    assert rc == WANQ_E_ARG and b"aligned to 4 elements" in msg, (rc, msg)


def test_quantiser_refusals(lib, p):
    for name in ("x", "q", "scale"):
        rc, msg = quant(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and QUANT.encode() in msg and b"non-NULL" in msg, (name, rc, msg)
    rc, msg = quant(lib, p[0], x_dtype=I32)
    assert rc == WANQ_E_ARG and b"bad x dtype 3" in msg, (rc, msg)
    for f in (2, -1):
        rc, msg = quant(lib, p[0], fmt=f)
        assert rc == WANQ_E_ARG and b"fmt=%d" % f in msg, (rc, msg)
    rc, msg = quant(lib, p[0], act=2)
    assert rc == WANQ_E_ARG and b"act must be 0 or 1" in msg, (rc, msg)
    for cols in (0, 12, 16392, 16416):
        rc, msg = quant(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and QUANT.encode() in msg and b"cols=%d" % cols in msg, (rc, msg)
    for cols in (8, 48, 2056):
        rc, msg = quant(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and b"cols=%d must be a multiple of 32" % cols in msg, (rc, msg)
    rc, msg = quant(lib, p[0], q=ctypes.c_void_p(p[0].value + 4))
    assert rc == WANQ_E_ARG and b"q must be 16-byte aligned" in msg, (rc, msg)
    assert quant(lib, p[0], rows=0)[0] == WANQ_OK and quant(lib, p[0], rows=0, fmt=1)[0] == WANQ_OK


def test_python_refusal_text_agrees_with_the_c_entry(lib, p):
    from viditq_extension import qgemm

    assert qgemm.MX_K_STEP == 128
    cases = [(8, 16, 128), (1, 8, 128), (8, 16, 64), (8, 16, 96), (8, 16, 192), (8, 12, 128), (8, 0, 128), (8, 16, 0),
             ((1 << 31) - 256, 128 * 256, 128), (1 << 31, 16, 128), (32760, 8960, 1536), (32760, 1536, 8960), (75600, 5120, 13824)]
    for w_fmt in (FP8, FP4):
        for M, N, K in cases:
            why = qgemm.mx_linear_refusal(M, N, K, w_fmt)
            rc, msg = gemm(lib, p[0], M=M if why else 0, N=N, K=K, w_fmt=0 if w_fmt == FP8 else 1)  # (accepted: sent with M = 0)
            assert (why is None) == (rc == WANQ_OK), (M, N, K, why, msg)
            if why is not None:
                assert why.encode() in msg, (why, msg)
    assert "K=64 must be a positive multiple of 128" == qgemm.mx_linear_refusal(8, 16, 64, FP4)
    assert "w_fmt='fp8_e4m3'" in qgemm.mx_linear_refusal(8, 16, 128, "fp8_e4m3")


# ---- config ---------------------------------------------------------------------------------------------------------------------
def _cfg(path=YAML8, **edits):
    from qdiff import config as qcfg

    cfg = qcfg.load(path)
    for key, v in edits.items():
        sec, k = key.split("__")
        if v is None:
            del cfg[sec][k]
        else:
            cfg[sec][k] = v
    return cfg


def _layer(cfg, cls=None, K=64, N=16, name="blocks.0.ffn.0"):
    from qdiff.base.quant_layer import QuantizedLinear

    g = torch.Generator().manual_seed(3)
    fp = torch.nn.Linear(K, N)
    fp.weight.data.copy_(torch.randn(N, K, generator=g) * K ** -0.5)
    fp.bias.data.copy_(torch.randn(N, generator=g) * 0.1)
    return (cls or QuantizedLinear)(K, N, True, "cpu", cfg, fp, module_name=name)


def test_both_shipped_configs_parse_and_build_a_layer():
    for path, wf, bits in ((YAML8, FP8, 8), (YAML4, FP4, 4)):
        cfg = _cfg(path)
        assert cfg.weight.format == wf and cfg.act.format == FP8
        assert cfg.weight.n_bits == bits and cfg.weight.sym is True and cfg.act.n_bits == 8 and cfg.act.sym is True
        assert cfg.get("viditq") is None and cfg.weight.get("group_size") is None
        ql = _layer(cfg)
        assert ql.mx == wf and not ql.fp8 and ql.group_size is None
        ql = _layer(_cfg(path, weight__group_size=32))   # the format's own block, spelled out
        assert ql.mx == wf and ql.group_size is None


def test_refused_combinations_name_the_layer_and_the_reason():
    from qdiff import config as qcfg
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    L = r"blocks\.0\.ffn\.0: "
    for path, wf, bits in ((YAML8, FP8, 8), (YAML4, FP4, 4)):
        for edits, rx in (({"act__format": FP4}, L + r"act\.format: mxfp4_e2m1.*no fp4 activation quantiser path is built yet"),
                          ({"act__format": "fp8_e4m3"}, L + r"an MX format on one side.*act\.format is 'fp8_e4m3'"),
                          ({"weight__format": "fp8_e4m3"}, L + r"an MX format on one side.*weight\.format is 'fp8_e4m3'"),
                          ({"act__format": None}, L + r"an MX format on one side.*act\.format is None"),
                          ({"weight__format": None}, L + r"an MX format on one side.*weight\.format is None"),
                          ({"weight__group_size": 64}, L + r"weight\.format: " + wf + r" with weight\.group_size=64.*32 input channels"),
                          ({"weight__group_size": 128}, L + r".*weight\.group_size=128"),
                          ({"weight__sym": False}, L + r"weight\.format.*weight\.sym: True"),
                          ({"act__sym": False}, L + r"act\.format.*act\.sym: True"),
                          ({"weight__n_bits": 12 - bits}, L + r"weight\.format: " + wf + r" needs weight\.n_bits: %d \(it is %d\)" % (bits, 12 - bits)),
                          ({"act__n_bits": 4}, L + r"act\.format: mxfp8_e4m3 needs act\.n_bits: 8 \(it is 4\)"),
                          ({"weight__n_bits": qcfg.ListConfig([4, 8])}, L + r"weight\.format with a bit-width list"),
                          ({"act__n_bits": qcfg.ListConfig([4, 8])}, L + r"act\.format with a bit-width list")):
            with pytest.raises(NotImplementedError, match=rx):
                _layer(_cfg(path, **edits))
        for sec in ("weight", "act"):
            with pytest.raises(ValueError, match=L + sec + r"\.format='mxfp6_e2m3' is not a known format"):
                _layer(_cfg(path, **{sec + "__format": "mxfp6_e2m3"}))
        for cls in (SQQuantizedLinear, QuarotQuantizedLinear, ViDiTQuantizedLinear):
            cfg = _cfg(path)
            cfg["smooth_quant"] = cfg["quarot"] = cfg["viditq"] = qcfg.create({"layer_name_regex": "ffn", "alpha": 0.5})
            with pytest.raises(NotImplementedError, match=L + r"weight\.format / act\.format with " + cls.__name__):
                _layer(cfg, cls)
        no_act = _cfg(path)
        del no_act["act"]
        with pytest.raises(NotImplementedError, match=L + r"an MX format on one side.*act\.format is None"):
            _layer(no_act)
    # an fp8 weight against an MX activation, from the fp8 side
    with pytest.raises(NotImplementedError, match=L + r"act\.format: mxfp4_e2m1.*no fp4 activation"):
        _layer(_cfg(YAML8, weight__format="fp8_e4m3", act__format=FP4))


# ---- the host expression, value by value ------------------------------------------------------------------------------------------
def host(x, fmt, gelu=False):
    from qdiff.base.base_quantizer import mx_quant_rows_host

    return mx_quant_rows_host(x, fmt, gelu)


def blocks_of(vals, pin):
    """the values laid out in blocks of 32 whose first element is `pin` (which fixes the block's amax, so its scale)"""
    out = []
    for j in range(0, len(vals), 31):
        chunk = list(vals[j:j + 31])
        out += [pin] + chunk + [0.0] * (31 - len(chunk))
    return torch.tensor(out, dtype=torch.float32)[None, :]


def test_e4m3_every_code_its_midpoints_and_their_neighbours():
    """blocks pinned at 448 (E = 135, s = 127, scale 2^0): the codes are the conversion's alone.  Every finite code's value, the midpoint
    to the next code of its sign (ties to even, the subnormal range included) and the fp32 neighbours of that midpoint, as
    tests/test_gpu_fp8.py asks of the fp8 quantiser"""
    val = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    vals, want = [], []
    for c in range(256):
        if c & 0x7f == 0x7f:
            continue
        v = val[c].item()
        vals.append(v)
        want.append(c)
        if (c + 1) & 0x7f != 0x7f:
            mid = (val[c].double() + val[c + 1].double()) / 2
            assert mid.float().double() == mid
            mid = mid.float()
            even, odd = (c, c + 1) if c % 2 == 0 else (c + 1, c)
            lo, hi = torch.nextafter(mid, torch.zeros(())), torch.nextafter(mid, mid * 2)
            vals += [mid.item(), lo.item(), hi.item()]
            want += [even, c, c + 1]
    x = blocks_of(vals, 448.0)
    codes, s = host(x, FP8)
    assert set(s.view(-1).tolist()) == {127}
    got = codes.view(-1, 32)[:, 1:].reshape(-1)[:len(want)].tolist()
    assert codes.view(-1, 32)[:, 0].tolist() == [0x7e] * (x.shape[1] // 32)
    bad = [(vals[j], hex(got[j]), hex(want[j])) for j in range(len(want)) if got[j] != want[j]]
    assert not bad, bad[:8]
    assert len(set(want)) == 254


def test_e2m1_all_fifteen_values_every_midpoint_and_saturation():
    """blocks pinned at 6 (E = 129, s = 127, scale 2^0).  The 15 distinct values, the seven midpoints and their fp32 neighbours on both
    signs (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), and the sign bit of -0"""
    from qdiff.base.base_quantizer import E2M1_VALUES, mx_unpack_e2m1

    assert E2M1_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    vals, want = [], []
    for sign, sbit in ((1.0, 0), (-1.0, 8)):
        for m, v in enumerate(E2M1_VALUES):
            vals.append(sign * v)
            want.append(m | sbit)
        for mid, to, below, above in ((0.25, 0, 0, 1), (0.75, 2, 1, 2), (1.25, 2, 2, 3), (1.75, 4, 3, 4), (2.5, 4, 4, 5), (3.5, 6, 5, 6),
                                      (5.0, 6, 6, 7)):
            t = torch.tensor(mid)
            vals += [sign * mid, sign * torch.nextafter(t, torch.zeros(())).item(), sign * torch.nextafter(t, t * 2).item()]
            want += [to | sbit, below | sbit, above | sbit]
    x = blocks_of(vals, 6.0)
    codes, s = host(x, FP4)
    assert tuple(codes.shape) == (1, x.shape[1] // 2) and set(s.view(-1).tolist()) == {127}
    got = mx_unpack_e2m1(codes).view(-1, 32)
    assert got[:, 0].tolist() == [7] * got.shape[0]
    got = got[:, 1:].reshape(-1)[:len(want)].tolist()
    assert got == want, [(vals[j], got[j], want[j]) for j in range(len(want)) if got[j] != want[j]][:8]
    assert len(set(want)) == 16   # 15 distinct values: +0 and -0 are two codes of one value
    # values above 6 saturate: a block pinned at 7.9 has E = 129 too, so 6.5, 7 and 7.9 meet the clamp, on both signs
    x = torch.zeros(1, 32)
    x[0, :6] = torch.tensor([7.9, 6.5, 7.0, -7.9, -6.5, -7.0])
    codes, s = host(x, FP4)
    assert s.tolist() == [[127]] and mx_unpack_e2m1(codes)[0, :6].tolist() == [7, 7, 7, 15, 15, 15]


def test_pack_and_unpack_put_even_k_in_the_low_nibble():
    from qdiff.base.base_quantizer import mx_pack_e2m1, mx_unpack_e2m1

    c = (torch.arange(3 * 64) * 7 % 16).to(torch.uint8).view(3, 64)
    pk = mx_pack_e2m1(c)
    assert tuple(pk.shape) == (3, 32) and pk.dtype == torch.uint8
    assert all(pk[r, k // 2].item() == (c[r, k].item() | (c[r, k + 1].item() << 4)) for r in range(3) for k in range(0, 64, 2))
    assert torch.equal(mx_unpack_e2m1(pk), c)


@pytest.mark.parametrize("fmt,emax,vmax,top", [(FP8, 8, 448.0, 0x7e), (FP4, 2, 6.0, 7)])
def test_block_scale_exponent_boundary_zero_subnormal_and_saturation(fmt, emax, vmax, top):
    """block amax exactly at a power of two and one ulp either side: the scale byte steps AT the power of two (E is the exponent field,
    not a rounded logarithm); amax 0 and an fp32 subnormal give s = 0; the largest finite block (E = 254) gives s = 254 - emax, and 255 is never written; amax just below
    2^(e+1) with s = e + 127 - emax scales to just below 2^(emax+1), above the format's largest: it saturates"""
    from qdiff.base.base_quantizer import mx_decode, mx_unpack_e2m1

    one = torch.tensor(1.0)
    below, above = torch.nextafter(one, torch.zeros(())), torch.nextafter(one, one * 2)
    x = torch.zeros(1, 8 * 32)
    pins = [below.item(), 1.0, above.item(), 0.0, 2.0 ** -130, 2.0 ** 127 * 1.5, torch.nextafter(one * 2, one).item() * 2.0 ** 10, 2.0 ** -126]
    for b, v in enumerate(pins):
        x[0, 32 * b] = v
        x[0, 32 * b + 1] = -v / 2
    codes, s = host(x, fmt)
    assert s.tolist() == [[126 - emax, 127 - emax, 127 - emax, 0, 0, min(254, 254 - emax), 137 - emax, max(0, 1 - emax)]]
    flat = (codes if fmt == FP8 else mx_unpack_e2m1(codes)).view(8, 32)
    one_code = {FP8: (8 + 7) << 3, FP4: 4 + 2}[fmt]        # 2^emax: exponent field emax + bias, mantissa 0
    # block 0: amax just under 1 scaled by 2^(emax + 1) is just under 2^(emax + 1): past the largest value, it saturates
    assert flat[0, 0].item() == top
    # blocks 1, 2: amax = 1 (and 1 + ulp, which rounds back) scaled by 2^emax is the code of 2^emax
    assert flat[1, 0].item() == one_code and flat[2, 0].item() == one_code
    assert flat[3].tolist() == [0, 0x80 if fmt == FP8 else 8] + [0] * 30      # a zero block: codes 0 (and the sign of -0)
    assert flat[6, 0].item() == top                                            # just under 2^11: saturates
    assert flat[5, 0].item() != 0 and 255 not in s.view(-1).tolist()
    # dequantisation gives back what the format can hold: exact for the pinned powers of two
    deq = mx_decode(codes, s, fmt, torch.float64).view(8, 32)
    assert deq[1, 0].item() == 1.0 and deq[1, 1].item() == -0.5 and deq[0, 0].item() == vmax * 2.0 ** (-1 - emax)


@pytest.mark.parametrize("fmt", [FP8, FP4])
def test_host_expression_on_random_rows_against_a_scalar_evaluation(fmt):
    """the vectorised expression against the definition evaluated element by element in Python floats (exact power-of-two scaling, then
    the nearest representable value with ties to the even code), on rows whose blocks differ by orders of magnitude"""
    import math

    from qdiff.base.base_quantizer import E2M1_VALUES, mx_unpack_e2m1

    emax, vmax = (8, 448.0) if fmt == FP8 else (2, 6.0)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 96, generator=g) * (10.0 ** torch.randint(-6, 7, (3, 3), generator=g).float()).repeat_interleave(32, dim=1)
    x[1, 32:64] = 0
    codes, s = host(x, fmt)
    flat = codes if fmt == FP8 else mx_unpack_e2m1(codes)
    if fmt == FP8:
        table = [(c, v) for c, v in enumerate(torch.arange(128, dtype=torch.uint8).view(torch.float8_e4m3fn).double().tolist()) if c != 0x7f]
    else:
        table = list(enumerate(E2M1_VALUES))
    for r in range(3):
        for b in range(3):
            blk = x[r, 32 * b:32 * b + 32].tolist()
            amax = max(abs(v) for v in blk)
            E = 0 if amax < 2.0 ** -126 else math.frexp(amax)[1] - 1 + 127
            sb = min(254, max(0, E - emax))
            assert s[r, b].item() == sb
            for j, v in enumerate(blk):
                t = min(vmax, abs(math.ldexp(v, 127 - sb)))
                d = min(abs(t - tv) for _, tv in table)
                best = [c for c, tv in table if abs(t - tv) == d]
                c = best[0] if len(best) == 1 else [c for c in best if c % 2 == 0][0]
                sign = (0x80 if fmt == FP8 else 8) if math.copysign(1.0, v) < 0 else 0
                assert flat[r, 32 * b + j].item() == (c | sign), (r, b, j, v)


# ---- simulation mode in host memory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,wf", [(YAML8, FP8), (YAML4, FP4)])
def test_cpu_simulation_mode_is_f_linear_on_the_dequantised_operands(path, wf):
    from qdiff.base.base_quantizer import MxQuantizer, mx_decode

    ql = _layer(_cfg(path), K=192, N=24)
    assert ql.mx == wf and isinstance(ql.w_quantizer, MxQuantizer) and isinstance(ql.a_quantizer, MxQuantizer)
    assert ql.w_quantizer.format == wf and ql.a_quantizer.format == FP8
    w = ql.fp_module.weight.data
    wc, ws = host(w, wf)
    assert ql._codes.dtype == torch.uint8 and tuple(ql._codes.shape) == (24, 192 if wf == FP8 else 96) and ql.int_weight is ql._codes
    assert torch.equal(ql._codes, wc) and torch.equal(ql.w_quantizer.scale_u8, ws) and tuple(ws.shape) == (24, 6)
    assert torch.equal(ql.w_quantizer.delta, torch.ldexp(torch.ones(24, 6), ws.int() - 127))
    wdq = mx_decode(wc, ws, wf)
    assert torch.equal(ql.weight.data, wdq)
    rel = ((wdq - w).norm() / w.norm()).item()
    assert rel < (0.05 if wf == FP8 else 0.2), rel            # e4m3: 3 mantissa bits; e2m1: one
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 37, 192, generator=g)
    x[0, 3] = 0             # a zero row: scale bytes 0, codes 0
    x[:, :, 7] *= 300       # an outlier channel: only its own block pays for it
    aq, as_ = host(x.view(-1, 192), FP8)
    want = torch.nn.functional.linear(mx_decode(aq, as_, FP8), wdq, ql.bias.detach().float()).view(2, 37, 24)
    got = ql(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 37, 24) and torch.equal(got, want)
    xb = x.to(torch.bfloat16)
    aq, as_ = host(xb.float().view(-1, 192), FP8)
    assert torch.equal(ql(xb), torch.nn.functional.linear(mx_decode(aq, as_, FP8), wdq, ql.bias.detach().float()).to(torch.bfloat16).view(2, 37, 24))
    fpy = ql.fp_module(x)
    assert ((got - fpy).norm() / fpy.norm()).item() < (0.06 if wf == FP8 else 0.25)
    ql.quant_mode = False
    assert torch.equal(ql(x), fpy)


# ---- integer checkpoint -------------------------------------------------------------------------------------------------------------
def _tiny_model(path):
    from qdiff import config as qcfg
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    fp = WanModel(dim=128, ffn_dim=256, num_heads=1, num_layers=2, text_dim=64, freq_dim=64).eval()
    model = QuantWanModel.from_float(fp, qcfg.load(path))
    model.quant_layer_refactor()
    model.set_init_done()
    return model


@pytest.mark.parametrize("path,wf", [(YAML8, FP8), (YAML4, FP4)])
def test_integer_checkpoint_round_trips_bit_for_bit(tmp_path, path, wf):
    from wan.quant_wanx_hip import HipLinearMx

    model = _tiny_model(path)
    file = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(file)
    d = 1 if wf == FP8 else 2
    for base, (N, K) in (("blocks.0.self_attn.q", (128, 128)), ("blocks.1.ffn.0", (256, 128)), ("blocks.1.ffn.2", (128, 256))):
        assert sd[base + ".weight"].dtype == torch.uint8 and tuple(sd[base + ".weight"].shape) == (N, K // d)
        assert sd[base + ".scale_weight"].dtype == torch.uint8 and tuple(sd[base + ".scale_weight"].shape) == (N, K // 32)
        assert sd[base + ".bias"].dtype == torch.float32 and base + ".zp_weight" not in sd and base + ".act_premul" not in sd
    assert not any(("fp_module" in k or "fp_weight" in k or "quantizer" in k) for k in sd)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q.*" + wf):
        model.quantize_and_save_weight(None, reference_format=True)

    # the file alone decides what the reloaded layers hold: shifted scale bytes and biases must come back as saved
    edited = {k: (v + 1 if (k.endswith(".scale_weight") or k.endswith(".bias")) and k.startswith("blocks.") else v) for k, v in sd.items()}
    torch.save(edited, file)
    fresh = _tiny_model(path).hardware_forward_refactor(load_path=file)
    assert len([m for m in fresh.hip_blocks.modules() if isinstance(m, HipLinearMx)]) == 20
    assert torch.equal(fresh.hip_blocks[0].ffn0.scale_weight, sd["blocks.0.ffn.0.scale_weight"] + 1)
    assert torch.equal(fresh.hip_blocks[0].ffn0.bias, sd["blocks.0.ffn.0.bias"] + 1)
    torch.save(sd, file)
    fresh2 = _tiny_model(path).hardware_forward_refactor(load_path=file)
    for n, hb in enumerate(fresh2.hip_blocks):
        for owner, attr, key in [(hb.self_attn, l, f"self_attn.{l}") for l in "qkvo"] + [(hb.cross_attn, l, f"cross_attn.{l}") for l in "qkvo"] + \
                                [(hb, "ffn0", "ffn.0"), (hb, "ffn2", "ffn.2")]:
            lin, sim = getattr(owner, attr), model.get_submodule(f"blocks.{n}.{key}")
            assert isinstance(lin, HipLinearMx) and lin.mx == wf and lin.weight.dtype == torch.uint8 and lin.scale_weight.dtype == torch.uint8
            assert torch.equal(lin.weight, sd[f"blocks.{n}.{key}.weight"]) and torch.equal(lin.weight, sim._codes)
            assert torch.equal(lin.scale_weight, sim.w_quantizer.scale_u8) and torch.equal(lin.bias, sim.bias.detach().float())
    bad = dict(sd)
    bad["blocks.1.ffn.0.scale_weight"] = sd["blocks.1.ffn.0.scale_weight"].float()
    torch.save(bad, file)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0\.scale_weight is \(256, 4\) torch\.float32"):
        _tiny_model(path).hardware_forward_refactor(load_path=file)


def test_kernel_mode_layer_buffers_and_construction_refusal():
    from wan.quant_wanx_hip import HipLinearMx, _to_hip_linear

    for path, wf in ((YAML8, FP8), (YAML4, FP4)):
        ql = _layer(_cfg(path), K=256, N=24)
        hl = _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
        assert isinstance(hl, HipLinearMx) and hl.mx == wf and not hl.fp8 and not hl.quantized and hl.act_key == "mxfp8"
        assert sorted(k for k, _ in hl.named_buffers()) == ["bias", "scale_weight", "weight"]
        assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.scale_u8)
        with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: format: " + wf + r" has no kernel-mode form.*K=192 must be"):
            _to_hip_linear(_layer(_cfg(path), K=192, N=24), None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
