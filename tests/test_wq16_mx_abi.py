"""CPU-only checks of the W4A16 MXFP4 GEMM entry (wanq_gemm_wq16_mx) and the host logic wired to it: bad arguments are refused with
their rule before any launch, M = 0 is a no-op; the config opt-in `weight.weight_only: True` and its refusals by layer name; a
host-memory layer from the shipped config holds the W4A8 MXFP4 layer's codes.  The kernel itself: tests/test_gpu_wq16_mx.py."""
import ctypes
import os

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wan2.1-quantization_amd")
NAME = "wanq_gemm_wq16_mx"
BF16, F32, E_ARG, E_SHAPE = 1, 2, 1, 2
FP4, LAYER = "mxfp4_e2m1", "blocks.1.ffn.0"
W4 = {"n_bits": 4, "sym": True, "format": FP4, "weight_only": True}
BUF = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(BUF) + 15) // 16 * 16  # host memory: never dereferenced by a refused call


def call(**kw):
    """wanq_gemm_wq16_mx on a well-formed [8, 128] x [16, 128] problem with the named arguments replaced (an int: P + that offset)"""
    from viditq_extension import _C

    a = dict(a=0, w=0, dtype=BF16, sw_u8=0, row_exp=0, out=0, out_dtype=BF16, bias=None, bias_dtype=F32, gate=None, residual=None, epi=0,
             M=8, N=16, K=128)
    a.update(kw)
    ptr = {k: ctypes.c_void_p(P + v) if isinstance(v, int) else v for k, v in a.items() if k in ("a", "w", "sw_u8", "row_exp", "out")}
    rc = getattr(_C.lib, NAME)(*{**a, **ptr}.values(), None)
    return rc, _C.lib.wanq_last_error()


@pytest.mark.parametrize("bad,code,rule", [
    (dict(a=None), E_ARG, b"non-NULL"), (dict(sw_u8=None), E_ARG, b"non-NULL"), (dict(row_exp=None), E_ARG, b"non-NULL"),
    (dict(K=96), E_SHAPE, b"K=96 must be a positive multiple of 64"), (dict(N=12), E_SHAPE, b"N=12 must be a positive multiple of 8"),
    (dict(w=8), E_ARG, b"16-byte aligned"), (dict(sw_u8=8), E_ARG, b"sw_u8 and row_exp must be 16-byte aligned"),
    (dict(row_exp=4), E_ARG, b"sw_u8 and row_exp must be 16-byte aligned"), (dict(dtype=F32), E_ARG, b"operand dtype 2"),
    (dict(out_dtype=3), E_ARG, b"out dtype 3"), (dict(epi=2), E_ARG, b"needs gate and residual")])
def test_bad_arguments_are_refused_with_their_rule(bad, code, rule):
    rc, msg = call(**bad)
    assert rc == code and NAME.encode() in msg and rule in msg, (rc, msg)


def test_m_zero_is_ok_and_the_wrapper_refuses_cpu_tensors():
    from viditq_extension import qgemm

    assert call(M=0)[0] == 0  # (no GPU here: a launch would fail)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        qgemm.wq16_mx_linear(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(8, 32, dtype=torch.uint8),
                             torch.zeros(8, 2, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8))
    assert "K=96" in qgemm.wq16_mx_linear_refusal(1, 16, 96) and qgemm.wq16_mx_linear_refusal(1, 8960, 1536) is None
    s = torch.tensor([[120, 131], [255, 140], [3, 9], [255, 255]], dtype=torch.uint8)
    assert qgemm.wq16_mx_row_exp(s).tolist() == [118, 127, 0, 0]  # max - 13 over the bytes below 255, clamped at 0


def _layer(cfg, cls=None, K=256, N=16):
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear

    torch.manual_seed(0)
    fp = torch.nn.Linear(K, N)
    return (cls or QuantizedLinear)(K, N, True, fp.weight.device, qcfg.create(cfg), fp, module_name=LAYER)


@pytest.mark.parametrize("cfg,words", [
    ({"weight": W4, "act": {"n_bits": 8, "sym": True, "format": "mxfp8_e4m3"}}, "`act:` section"),
    ({"weight": dict(W4, format="mxfp8_e4m3", n_bits=8)}, "weight.format='mxfp8_e4m3'"),
    ({"weight": {"n_bits": 4, "sym": False, "weight_only": True}}, "weight.format=None"),
    ({"weight": W4, "mx": {"block_hadamard": True}}, "mx.block_hadamard"),
    ({"weight": W4, "mx": {"outlier_channels": 128}}, "mx.outlier_channels"),
    ({"weight": dict(W4, low_rank=32)}, "weight.low_rank"),
    ({"weight": W4, "smooth_quant": {"alpha": 0.5, "layer_name_regex": ""}}, "SQQuantizedLinear"),
    ({"weight": W4, "quarot": {"alpha": 0.5, "layer_name_regex": ""}}, "QuarotQuantizedLinear"),
    ({"weight": W4, "viditq": {"alpha": 0.5, "layer_name_regex": ""}}, "ViDiTQuantizedLinear")])
def test_weight_only_refusals_name_the_layer(cfg, words):
    """each is raised before any weight is quantised"""
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    cls = {"smooth_quant": SQQuantizedLinear, "quarot": QuarotQuantizedLinear, "viditq": ViDiTQuantizedLinear}.get(list(cfg)[-1])
    with pytest.raises(NotImplementedError) as ex:
        _layer(cfg, cls)
    assert str(ex.value).startswith(LAYER + ": weight.weight_only: True") and words in str(ex.value)


@pytest.mark.parametrize("cfg", [{"weight": dict(W4, weight_only=False)}, {"weight": {k: v for k, v in W4.items() if k != "weight_only"}}])
def test_without_the_opt_in_the_old_refusal_stands(cfg):
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: an MX format on one side needs an MX format on the other \(act\.format is None\)"):
        _layer(cfg)


@pytest.mark.parametrize("yaml", ["w4a16_mxfp4_all_linears", "w4a16_mxfp4_search_all_linears"])
def test_host_layer_from_the_shipped_config_holds_the_w4a8_layers_codes(yaml):
    from qdiff import config as qcfg
    from wan.quant_wanx_hip import _HIP_LINEAR_OF, HipLinearMx, HipLinearWq16Mx

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", "mx", yaml + ".yaml"))
    assert cfg.get("act", None) is None and cfg.weight.weight_only is True
    ql = _layer({"weight": dict(cfg.weight)})
    ref = _layer({"weight": {k: v for k, v in dict(cfg.weight).items() if k != "weight_only"}, "act": {"n_bits": 8, "sym": True, "format": "mxfp8_e4m3"}})
    assert ql.kind == "weight_only_mx" and ref.kind == "mx" and ql.mx_search_w is ("search" in yaml) and ql.a_quantizer is None
    assert torch.equal(ql._codes, ref._codes) and torch.equal(ql.w_quantizer.scale_u8, ref.w_quantizer.scale_u8)
    x = torch.randn(5, 256)
    assert torch.equal(ql(x), torch.nn.functional.linear(x, ref.weight.data, ref.bias))  # simulation mode: the decoded weight, x as it is
    m = HipLinearWq16Mx(256, 16, True, LAYER)
    assert _HIP_LINEAR_OF[ql.kind] is HipLinearWq16Mx and m.sharded == ("weight", "scale_weight")
    assert list(m.state_dict()) == list(HipLinearMx(256, 16, True, FP4).state_dict())
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: format: mxfp4_e2m1 with weight_only: True .*K=96"):
        HipLinearWq16Mx(96, 16, True, LAYER)
