"""CPU-only checks of the fine-grained fp8 Linears (`format: fp8_e4m3` with `group_size: 128` on both sides): the shipped config and the
layer kind it selects, the refusals by layer name and key, the host expression, the refusals of the two C entries and the kernel-mode
layer's buffers.  The kernels: tests/test_gpu_fp8_grouped.py."""
import ctypes
import os

import pytest
import torch

from test_fp8_abi import _cfg as _cfg8, _layer, lib, p  # noqa: F401  (fixtures)

YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wan2.1-quantization_amd", "quant_configs", "fp8",
                    "w8a8_fp8_g128_all_linears.yaml")
F32, BF16, WANQ_OK, WANQ_E_ARG, WANQ_E_SHAPE = 2, 1, 0, 1, 2
vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _cfg(**edits):
    from qdiff import config as qcfg

    cfg = qcfg.load(YAML)
    for key, v in edits.items():
        sec, k = key.split("__")
        if v is None:
            del cfg[sec][k]
        elif k == "section":
            cfg[sec] = qcfg.create(v)
        else:
            cfg[sec][k] = v
    return cfg


def test_shipped_config_selects_the_grouped_kind():
    cfg = _cfg()
    assert cfg.weight.format == cfg.act.format == "fp8_e4m3" and cfg.weight.group_size == cfg.act.group_size == 128
    ql = _layer(cfg, K=256, N=16, name="blocks.0.self_attn.q")
    assert ql.kind == "fp8_grouped" and ql.fp8_group == 128 and "fp8_grouped" in type(ql)._FORWARDS
    assert tuple(ql.w_quantizer.delta.shape) == (16, 2) and _layer(_cfg8(), K=256, N=16).kind == "fp8"


@pytest.mark.parametrize("edits,rx", [
    ({"act__group_size": None}, r"weight\.format with weight\.group_size=128 and act\.group_size=None is not supported.*128"),
    ({"weight__group_size": None}, r"act\.format with act\.group_size=128 and no weight\.group_size"),
    ({"weight__group_size": 64, "act__group_size": 64}, r"weight\.format with weight\.group_size=64"),
    ({"act__group_size": 256}, r"weight\.format with weight\.group_size=128 and act\.group_size=256"),
    ({"weight__low_rank": 8}, r"weight\.low_rank with an `act:` section"),
    ({"gptq__section": {"layer_name_regex": "ffn"}}, r"gptq with weight\.format"),
    ({"viditq__section": {"layer_name_regex": "ffn", "alpha": 0.5}}, r"weight\.format / act\.format with ViDiTQuantizedLinear"),
])
def test_refusals_name_the_layer_and_the_key(edits, rx):
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: " + rx):
        _layer(_cfg(**edits), ViDiTQuantizedLinear if "viditq__section" in edits else None, K=256)


@pytest.mark.parametrize("cols", [128, 384, 192])
def test_host_helper_is_fp8_quant_rows_on_the_128_wide_view(cols):
    """... a row length that is no multiple of 128 leaves a shorter last group; the layer in host memory is F.linear of the decode"""
    from qdiff.base.base_quantizer import fp8_decode, fp8_group_expand, fp8_quant_rows, fp8_quant_rows_grouped

    x = torch.randn(5, cols, generator=torch.Generator().manual_seed(cols))
    x[:, 3] *= 60
    x[2, :128] = 0
    codes, scale = fp8_quant_rows_grouped(x)
    full = cols // 128 * 128
    c, s = fp8_quant_rows(x[:, :full].reshape(-1, 128))
    assert torch.equal(codes[:, :full], c.view(5, full)) and torch.equal(scale[:, :full // 128], s.view(5, -1))
    if full < cols:
        ct, st = fp8_quant_rows(x[:, full:])
        assert torch.equal(codes[:, full:], ct) and torch.equal(scale[:, -1], st)
    assert scale[2, 0] == torch.tensor(1e-6) and not bool(codes[2, :128].any())
    ql = _layer(_cfg(), K=cols, N=24)
    wc, ws = fp8_quant_rows_grouped(ql.fp_module.weight.data)
    assert torch.equal(ql._codes, wc) and torch.equal(ql.w_quantizer.delta, ws)
    want = torch.nn.functional.linear(fp8_decode(codes) * fp8_group_expand(scale, 128, cols),
                                      fp8_decode(wc) * fp8_group_expand(ws, 128, cols), ql.bias.detach().float())
    assert torch.equal(ql(x), want)


def _gemm(lib, ptr, a=1, w=1, sa=1, sw=1, group=128, M=8, K=256):
    lib.wanq_gemm_fp8_grouped.argtypes = [vp, vp, vp, vp, i, vp, i, vp, i, vp, vp, i, i64, i, i, vp]
    return lib.wanq_gemm_fp8_grouped(a and ptr, w and ptr, sa and ptr, sw and ptr, group, ptr, BF16, None, F32, None, None, 0, M, 16, K, None)


def _quant(lib, ptr, scale=1, rows=4, cols=256, group=128):
    lib.wanq_quant_rows_fp8_grouped.argtypes = [vp, i, vp, vp, i64, i, i, i, vp]
    return lib.wanq_quant_rows_fp8_grouped(ptr, F32, ptr, scale and ptr, rows, cols, group, 0, None)


@pytest.mark.parametrize("call,kw,code,words", [
    (_gemm, {"group": 64}, WANQ_E_ARG, b"group=64 must be 128"),
    (_gemm, {"K": 192}, WANQ_E_SHAPE, b"K=192 must be a positive multiple of 128"),
    (_gemm, {"sa": None}, WANQ_E_ARG, b"must be non-NULL"),
    (_gemm, {"sw": None}, WANQ_E_ARG, b"must be non-NULL"),
    (_quant, {"group": 32}, WANQ_E_ARG, b"group=32 must be 128"),
    (_quant, {"cols": 192}, WANQ_E_SHAPE, b"cols=192 must be a multiple of 128"),
    (_quant, {"cols": 16512}, WANQ_E_SHAPE, b"cols=16512"),
    (_quant, {"scale": None}, WANQ_E_ARG, b"must be non-NULL"),
])
def test_c_entries_refuse_with_a_message(lib, p, call, kw, code, words):  # noqa: F811
    rc, msg = call(lib, p[0], **kw), lib.wanq_last_error()
    assert rc == code and words in msg and b"fp8_grouped" in msg, (rc, msg)
    assert call(lib, p[0], **({"M": 0} if call is _gemm else {"rows": 0})) == WANQ_OK  # well formed, nothing to do: nothing launched


def test_kernel_mode_layer_buffers_sharding_and_refusal():
    from viditq_extension import qgemm
    from wan.quant_wanx_hip import _HIP_LINEAR_OF, _ROW_QUANTISERS, HipLinearFp8, _to_hip_linear

    old = HipLinearFp8(256, 24)
    assert sorted(k for k, _ in old.named_buffers()) == ["bias", "scale_weight", "weight"] and tuple(old.scale_weight.shape) == (24,)
    assert old.act_form == old.act_key == "fp8" and old.sharded == ("weight",) and old.group_size is None
    ql = _layer(_cfg(), K=256, N=24)
    hl = _to_hip_linear(ql, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
    assert _HIP_LINEAR_OF["fp8_grouped"] is HipLinearFp8 and isinstance(hl, HipLinearFp8) and hl.checkpointed and hl.plain_rows
    assert sorted(k for k, _ in hl.named_buffers()) == ["bias", "fp8_group", "scale_weight", "weight"] and int(hl.fp8_group) == 128
    assert hl.act_form == hl.act_key == "fp8_g128" and hl.sharded == ("weight", "scale_weight")
    assert _ROW_QUANTISERS["fp8_g128"][0] == "quant_rows_fp8_grouped"
    assert torch.equal(hl.weight, ql._codes) and torch.equal(hl.scale_weight, ql.w_quantizer.delta.t()) and tuple(hl.scale_weight.shape) == (2, 24)
    assert qgemm.fp8_grouped_linear_refusal(8, 16, 192) == "K=192 must be a positive multiple of 128"
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.ffn\.0: format: fp8_e4m3 with group_size: 128 has no kernel-mode form.*K=192"):
        _to_hip_linear(_layer(_cfg(), K=192, N=24), None, False, torch.bfloat16, "torch", "blocks.0.ffn.0")
