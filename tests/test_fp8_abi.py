"""CPU-only checks of the fp8 (OCP e4m3fn) W8A8 Linears: the two C entries (wanq_quant_rows_fp8, wanq_gemm_fp8) are declared, exported
and prototyped, the header still compiles as C99 and the ABI version stays 6; every refusal returns its code and a message naming the
rule before anything is launched; qgemm.fp8_linear_refusal agrees with the C entry.  Python side: quant_configs/
w8a8_fp8_all_linears.yaml parses; every combination the `format` key does not take is refused by layer name when the layer is built;
simulation mode in host memory is the torch expression; the integer checkpoint of a tiny model reloads bit for bit.
The kernels themselves: tests/test_gpu_fp8.py."""
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
YAML = os.path.join(PKG, "quant_configs", "w8a8_fp8_all_linears.yaml")
GEMM, QUANT = "wanq_gemm_fp8", "wanq_quant_rows_fp8"
F16, BF16, F32, I32 = 0, 1, 2, 3
WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 0, 1, 2
vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
ARGTYPES = {GEMM: [vp, vp, vp, vp, vp, i, vp, i, vp, vp, i, i64, i, i, vp], QUANT: [vp, i, vp, vp, i64, i, i, vp]}


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


def gemm(lib, ptr, **kw):
    """wanq_gemm_fp8 on a well-formed [8, 128] x [16, 128] problem, with the named arguments replaced"""
    a = dict(a=ptr, w=ptr, sa=ptr, sw=ptr, out=ptr, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0, M=8, N=16,
             K=128)
    a.update(kw)
    fn = getattr(lib, GEMM)
    fn.argtypes = ARGTYPES[GEMM]
    rc = fn(a["a"], a["w"], a["sa"], a["sw"], a["out"], a["out_dtype"], a["bias"], a["bias_dtype"], a["gate"], a["residual"], a["epi"],
            a["M"], a["N"], a["K"], None)
    return rc, lib.wanq_last_error()


def quant(lib, ptr, **kw):
    a = dict(x=ptr, x_dtype=F32, q=ptr, scale=ptr, rows=4, cols=64, act=0)
    a.update(kw)
    fn = getattr(lib, QUANT)
    fn.argtypes = ARGTYPES[QUANT]
    return fn(a["x"], a["x_dtype"], a["q"], a["scale"], a["rows"], a["cols"], a["act"], None), lib.wanq_last_error()


# ---- entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first", [(GEMM, ["const uint8_t* a", "const uint8_t* w", "const float* sa", "const float* sw"]),
                                        (QUANT, ["const void* x", "int x_dtype", "uint8_t* q", "float* scale"])])
def test_entries_are_declared_exported_and_prototyped(lib, name, first):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared in include/wanq_hip.h"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert len(params) == len(ARGTYPES[name]) and params[:4] == first, params
    assert hasattr(lib, name), f"{name} is not exported by libwanq_hip.so"
    from viditq_extension import _C

    assert name in _C.PROTOTYPES and list(_C.PROTOTYPES[name]) == ARGTYPES[name]


def test_header_still_compiles_as_c99_and_the_abi_version_stays_6(lib, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wanq_hip.h"\nint main(void) { return (int)(sizeof(&%s) + sizeof(&%s) == 0); }\n' % (GEMM, QUANT))
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert lib.wanq_abi_version() == 6


# ---- refusals of the C entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 32, 96, 100, -64])
def test_k_not_a_multiple_of_the_k_step_is_refused(lib, p, K):
    rc, msg = gemm(lib, p[0], K=K)
    assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"K=%d" % K in msg and b"multiple of 64" in msg, (rc, msg)


def test_n_m_and_the_tile_count_are_refused(lib, p):
    for N in (12, 4, 0):
        rc, msg = gemm(lib, p[0], N=N)
        assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"N=%d" % N in msg and b"multiple of 8" in msg, (rc, msg)
    for M in (-1, 1 << 31):
        rc, msg = gemm(lib, p[0], M=M)
        assert rc == WANQ_E_SHAPE and b"M=%d" % M in msg and b"out of range" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], M=(1 << 31) - 256, N=128 * 256)  # 2^24 - 1 row tiles x 256 column tiles
    assert rc == WANQ_E_SHAPE and GEMM.encode() in msg and b"too many tiles" in msg, (rc, msg)
    assert gemm(lib, p[0], M=0)[0] == WANQ_OK  # nothing to do, nothing launched


def test_arguments_are_refused(lib, p):
    for name in ("a", "w", "sa", "sw", "out"):
        rc, msg = gemm(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and b"must be non-NULL" in msg, (name, rc, msg)
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
    rc, msg = gemm(lib, p[0], sw=off(4))
    assert rc == WANQ_E_ARG and b"sw must be 16-byte aligned" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], sa=off(2))
    assert rc == WANQ_E_ARG and b"sa 4-byte aligned" in msg, (rc, msg)
    rc, msg = gemm(lib, p[0], bias=off(4), bias_dtype=F32)
    assert rc == WANQ_E_ARG and b"aligned to 4 elements" in msg, (rc, msg)


def test_quantiser_refusals(lib, p):
    for name in ("x", "q", "scale"):
        rc, msg = quant(lib, p[0], **{name: None})
        assert rc == WANQ_E_ARG and QUANT.encode() in msg and b"non-NULL" in msg, (name, rc, msg)
    rc, msg = quant(lib, p[0], x_dtype=I32)
    assert rc == WANQ_E_ARG and b"bad x dtype 3" in msg, (rc, msg)
    rc, msg = quant(lib, p[0], act=2)
    assert rc == WANQ_E_ARG and b"act must be 0 or 1" in msg, (rc, msg)
    for cols in (0, 12, 16392):
        rc, msg = quant(lib, p[0], cols=cols)
        assert rc == WANQ_E_SHAPE and QUANT.encode() in msg and b"cols=%d" % cols in msg, (rc, msg)
    assert quant(lib, p[0], rows=0)[0] == WANQ_OK


def test_python_refusal_text_agrees_with_the_c_entry(lib, p):
    from viditq_extension import qgemm

    assert qgemm.FP8_K_STEP == 64
    cases = [(8, 16, 128), (1, 8, 64), (8, 16, 96), (8, 16, 32), (8, 12, 128), (8, 0, 128), (8, 16, 0), ((1 << 31) - 256, 128 * 256, 64),
             (1 << 31, 16, 64), (32760, 8960, 1536), (32760, 1536, 8960)]
    for M, N, K in cases:
        why = qgemm.fp8_linear_refusal(M, N, K)
        rc, msg = gemm(lib, p[0], M=M if why else 0, N=N, K=K)  # (an accepted shape is sent with M = 0: nothing is launched)
        assert (why is None) == (rc == WANQ_OK), (M, N, K, why, msg)
        if why is not None:
            assert why.encode() in msg, (why, msg)
    assert "K=96 must be a positive multiple of 64" == qgemm.fp8_linear_refusal(8, 16, 96)
    assert "N=12" in qgemm.fp8_linear_refusal(8, 12, 128) and "too many tiles" == qgemm.fp8_linear_refusal((1 << 31) - 256, 128 * 256, 64)


# ---- config ---------------------------------------------------------------------------------------------------------------------
def _cfg(**edits):
    from qdiff import config as qcfg

    cfg = qcfg.load(YAML)
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


def test_shipped_config_parses():
    cfg = _cfg()
    assert cfg.weight.format == "fp8_e4m3" and cfg.act.format == "fp8_e4m3"
    assert cfg.weight.n_bits == 8 and cfg.weight.sym is True and cfg.act.n_bits == 8 and cfg.act.sym is True
    assert cfg.get("viditq") is None and cfg.weight.get("group_size") is None


def test_refused_combinations_name_the_layer_and_the_key():
    from qdiff import config as qcfg
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    L = r"blocks\.0\.ffn\.0: "
    for edits, rx in (({"act__format": None}, L + r".*both.*missing from `act:`"),
                      ({"weight__format": None}, L + r".*both.*missing from `weight:`"),
                      ({"weight__group_size": 32}, L + r"weight\.format with weight\.group_size"),
                      ({"weight__sym": False}, L + r"weight\.format.*weight\.sym: True"),
                      ({"act__sym": False}, L + r"act\.format.*act\.sym: True"),
                      ({"weight__n_bits": 4}, L + r"weight\.format.*weight\.n_bits: 8 \(it is 4\)"),
                      ({"act__n_bits": 6}, L + r"act\.format.*act\.n_bits: 8 \(it is 6\)"),
                      ({"weight__n_bits": qcfg.ListConfig([4, 8])}, L + r"weight\.format with a bit-width list"),
                      ({"act__n_bits": qcfg.ListConfig([4, 8])}, L + r"act\.format with a bit-width list")):
        with pytest.raises(NotImplementedError, match=rx):
            _layer(_cfg(**edits))
    with pytest.raises(ValueError, match=L + r"weight\.format='fp8_e5m2' is not a known format"):
        _layer(_cfg(weight__format="fp8_e5m2"))
    for cls in (SQQuantizedLinear, QuarotQuantizedLinear, ViDiTQuantizedLinear):
        cfg = _cfg()
        cfg["smooth_quant"] = cfg["quarot"] = cfg["viditq"] = qcfg.create({"layer_name_regex": "ffn", "alpha": 0.5})
        with pytest.raises(NotImplementedError, match=L + r"weight\.format / act\.format with " + cls.__name__):
            _layer(cfg, cls)
    no_act = _cfg()
    del no_act["act"]
    with pytest.raises(NotImplementedError, match=L + r".*missing from `act:`"):
        _layer(no_act)


# ---- simulation mode in host memory -----------------------------------------------------------------------------------------------
def fq(t):
    """the issue's expression: per-row e4m3 fake quantisation"""
    am = t.abs().amax(dim=-1, keepdim=True)
    s = (am / torch.full_like(am, 448.0)).clamp_min(1e-6)
    return (t / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s


def test_cpu_cast_is_rne_and_keeps_subnormals():
    """what the torch expression relies on: ties to even, the subnormal codes, and no flush"""
    v = torch.tensor([17.0, 19.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, -0.0, 448.0])
    assert v.to(torch.float8_e4m3fn).view(torch.uint8).tolist() == [0x58, 0x5a, 0x01, 0x00, 0x02, 0x80, 0x7e]


def test_cpu_simulation_mode_is_the_torch_expression():
    from qdiff.base.base_quantizer import Fp8Quantizer, fp8_decode

    ql = _layer(_cfg(), K=192, N=24)
    assert ql.fp8 and isinstance(ql.w_quantizer, Fp8Quantizer) and isinstance(ql.a_quantizer, Fp8Quantizer)
    w = ql.fp_module.weight.data
    assert ql._codes.dtype == torch.uint8 and tuple(ql._codes.shape) == (24, 192) and ql.int_weight is ql._codes
    assert torch.equal(ql.w_quantizer.delta.reshape(-1), (w.abs().amax(1) / torch.full((24,), 448.0)).clamp_min(1e-6))
    assert torch.equal(ql.weight.data, fq(w)) and torch.equal(fp8_decode(ql._codes) * ql.w_quantizer.delta, fq(w))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 37, 192, generator=g)
    x[0, 3] = 0      # a zero row: scale 1e-6, codes 0
    x[:, :, 7] *= 30
    want = torch.nn.functional.linear(fq(x), fq(w), ql.bias.detach().float())
    got = ql(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 37, 24) and torch.equal(got, want)
    assert torch.equal(ql(x.to(torch.bfloat16)), torch.nn.functional.linear(fq(x.to(torch.bfloat16).float()), fq(w),
                                                                            ql.bias.detach().float()).to(torch.bfloat16))
    ql.quant_mode = False
    assert torch.equal(ql(x), ql.fp_module(x))


# ---- integer checkpoint -------------------------------------------------------------------------------------------------------------
def _tiny_model():
    from qdiff import config as qcfg
    from wan.modules.model import WanModel
    from wan.quant_wanx import QuantWanModel

    torch.manual_seed(0)
    fp = WanModel(dim=128, ffn_dim=256, num_heads=1, num_layers=2, text_dim=64, freq_dim=64).eval()
    model = QuantWanModel.from_float(fp, qcfg.load(YAML))
    model.quant_layer_refactor()
    model.set_init_done()
    return model


def test_integer_checkpoint_round_trips_bit_for_bit(tmp_path):
    from wan.quant_wanx_hip import HipLinearFp8

    model = _tiny_model()
    path = str(tmp_path / "int_weight.pt")
    sd = model.quantize_and_save_weight(path)
    for base, (N, K) in (("blocks.0.self_attn.q", (128, 128)), ("blocks.1.ffn.0", (256, 128)), ("blocks.1.ffn.2", (128, 256))):
        assert sd[base + ".weight"].dtype == torch.uint8 and tuple(sd[base + ".weight"].shape) == (N, K)
        assert sd[base + ".scale_weight"].dtype == torch.float32 and tuple(sd[base + ".scale_weight"].shape) == (N,)
        assert sd[base + ".bias"].dtype == torch.float32 and base + ".zp_weight" not in sd and base + ".act_premul" not in sd
    assert not any(("fp_module" in k or "fp_weight" in k or "quantizer" in k) for k in sd)
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.self_attn\.q.*fp8_e4m3"):
        model.quantize_and_save_weight(None, reference_format=True)

    # the file alone decides what the reloaded layers hold: scaled copies of the scales and shifted biases must come back as saved
    edited = {k: (v * 2 if k.endswith(".scale_weight") else v + 1 if k.endswith(".bias") and k.startswith("blocks.") else v)
              for k, v in sd.items()}
    torch.save(edited, path)
    fresh = _tiny_model().hardware_forward_refactor(load_path=path)
    assert len([m for m in fresh.hip_blocks.modules() if isinstance(m, HipLinearFp8)]) == 20
    assert torch.equal(fresh.hip_blocks[0].ffn0.scale_weight, sd["blocks.0.ffn.0.scale_weight"] * 2)
    assert torch.equal(fresh.hip_blocks[0].ffn0.bias, sd["blocks.0.ffn.0.bias"] + 1)
    torch.save(sd, path)
    fresh2 = _tiny_model().hardware_forward_refactor(load_path=path)
    for i, hb in enumerate(fresh2.hip_blocks):
        for owner, attr, key in [(hb.self_attn, l, f"self_attn.{l}") for l in "qkvo"] + [(hb.cross_attn, l, f"cross_attn.{l}") for l in "qkvo"] + \
                                [(hb, "ffn0", "ffn.0"), (hb, "ffn2", "ffn.2")]:
            lin, sim = getattr(owner, attr), model.get_submodule(f"blocks.{i}.{key}")
            assert isinstance(lin, HipLinearFp8) and lin.weight.dtype == torch.uint8
            assert torch.equal(lin.weight, sd[f"blocks.{i}.{key}.weight"]) and torch.equal(lin.weight, sim._codes)
            assert torch.equal(lin.scale_weight, sim.w_quantizer.delta.reshape(-1)) and torch.equal(lin.bias, sim.bias.detach().float())
    bad = dict(sd)
    bad["blocks.1.ffn.0.weight"] = sd["blocks.1.ffn.0.weight"].view(torch.int8)
    torch.save(bad, path)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0\.weight is \(256, 128\) torch\.int8"):
        _tiny_model().hardware_forward_refactor(load_path=path)


def test_kernel_mode_layer_buffers_and_construction_refusal():
    from wan.quant_wanx_hip import HipLinearFp8, _to_hip_linear

    ql = _layer(_cfg(), K=192, N=24)
    hl = _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
    assert isinstance(hl, HipLinearFp8) and hl.fp8 and not hl.quantized and hl.act_key == "fp8"
    assert sorted(k for k, _ in hl.named_buffers()) == ["bias", "scale_weight", "weight"]
    assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.delta.reshape(-1))
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: format: fp8_e4m3 has no kernel-mode form.*K=96 must be"):
        _to_hip_linear(_layer(_cfg(), K=96, N=24), None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
