"""CPU-only checks of the clip search (csrc/clip_search.hip, `weight.clip`): the two entry points refuse bad arguments on the host
with the rule in the message, the config refusals carry the layer's name and the key, a config without `clip` never reaches the
search, and `search: mse` reaches it from the quantiser's initialisation."""
import ctypes

import pytest
import torch

from test_gptq_abi import GPTQ, _Net, _layer, _torch_weight_kernels

ARGS = {"wanq_clip_search": dict(w=1, chan_w=None, chan_len=0, n_bits=4, sym=0, qmin=-8, qmax=7, steps=20, n_cand=10, delta=1, zp=1, sel=1,
                                 table=None, rows=4, cols=128),
        "wanq_clip_search_blocks": dict(w=1, hblocks=1, g=128, n_bits=4, sym=0, qmin=-8, qmax=7, steps=20, n_cand=10, delta=1, zp=1, sel=1,
                                        table=None, N=4, K=256)}
COMMON = [({"w": None}, 1, b"w, delta, zp and sel must be non-NULL"), ({"sel": None}, 1, b"w, delta, zp and sel must be non-NULL"),
          ({"w": 4}, 1, b"w must be 16-byte aligned"), ({"n_bits": 9}, 1, b"n_bits=9 must be 2..8"), ({"qmin": -129}, 1, b"must be an int8 range"),
          ({"steps": 0}, 1, b"steps=0 must be 1..64"), ({"steps": 65}, 1, b"steps=65 must be 1..64"), ({"n_cand": 21}, 1, b"n_cand=21 must be 1..steps=20")]
RULES = {"wanq_clip_search": COMMON + [({"cols": 100}, 2, b"cols=100 must be a multiple of 8 in [8, 16384]"), ({"rows": -1}, 2, b"rows=-1"),
                                       ({"chan_w": 1, "chan_len": 192}, 2, b"chan_len=192 must be a positive multiple of cols=128")],
         "wanq_clip_search_blocks": COMMON + [({"g": 96}, 2, b"g=96 must be 32, 64 or 128 (the block is held in LDS)"), ({"g": 256}, 2, b"g=256 must be"),
                                              ({"K": 320}, 2, b"K=320 must be a multiple of g=128"), ({"hblocks": None}, 1, b"hblocks must be non-NULL"),
                                              ({"N": -1}, 2, b"N=-1 out of range")]}


@pytest.mark.parametrize("name", list(ARGS))
def test_entry_points_refuse_bad_arguments_with_the_rule(name):
    from viditq_extension import _C, fused

    buf = ctypes.create_string_buffer(4096)  # host memory: never dereferenced by a refused call (or by zero rows)
    base = ctypes.addressof(buf) // 16 * 16 + 16

    def call(**kw):
        a = {k: (base + v - 1 if k in ("w", "chan_w", "hblocks", "delta", "zp", "sel") and v else v) for k, v in dict(ARGS[name], **kw).items()}
        return getattr(_C.lib, name)(*a.values(), None), _C.lib.wanq_last_error()

    for kw, rc_want, text in RULES[name]:
        rc, msg = call(**kw)
        assert rc == rc_want and msg.startswith(name.encode() + b": ") and text in msg, (kw, msg)
    assert call(**{"rows" if name == "wanq_clip_search" else "N": 0})[0] == 0  # nothing to do: no launch
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        getattr(fused, name[5:])(torch.zeros(4, 128), *(() if name == "wanq_clip_search" else (torch.zeros(1, 128, 128),)), 4, False, -8, 7, 20, 10)


W4 = {"n_bits": 4, "sym": False, "group_size": 32}
WPC = {"n_bits": 4, "sym": False}
A8 = {"n_bits": 8, "sym": True}
MSE = {"search": "mse"}
REFUSALS = {  # case -> (config, a piece of the message behind "<layer>: weight.clip", ValueError?)
    "viditq": ({"weight": dict(WPC, clip=MSE), "act": A8, "viditq": {"layer_name_regex": "", "alpha": 0.5}}, "ViDiTQuantizedLinear", False),
    "smooth_quant": ({"weight": dict(WPC, clip=MSE), "act": A8, "smooth_quant": {"layer_name_regex": "", "alpha": 0.5}}, "SQQuantizedLinear", False),
    "quarot": ({"weight": dict(WPC, clip=MSE), "act": A8, "quarot": {"layer_name_regex": ""}}, "QuarotQuantizedLinear", False),
    "fp8": ({"weight": dict(n_bits=8, sym=True, format="fp8_e4m3", clip=MSE), "act": dict(A8, format="fp8_e4m3")}, "weight.format='fp8_e4m3'", False),
    "mxfp4": ({"weight": dict(n_bits=4, sym=True, format="mxfp4_e2m1", clip=MSE), "act": dict(A8, format="mxfp8_e4m3")}, "block_scale: search", False),
    "bit list": ({"weight": dict(n_bits=[4, 8], i_bitwidth=0, sym=False, clip=MSE)}, "bit-width list", False),
    "hessian per channel": ({"weight": dict(WPC, clip={"search": "hessian"})}, "`search: diag` is the per-channel form", False),
    "hessian g16": ({"weight": dict(WPC, group_size=16, clip={"search": "hessian"})}, r"group_size in \(32, 64, 128\) \(it is 16\)", False),
    "unknown key": ({"weight": dict(W4, clip=dict(MSE, ratio=0.9))}, r"\.ratio is not a known key", True),
    "unknown search": ({"weight": dict(W4, clip={"search": "awq"})}, r"\.search='awq' must be one of", True),
    "no search": ({"weight": dict(W4, clip={"steps": 20})}, r"\.search=None must be one of", True),
    "steps": ({"weight": dict(W4, clip=dict(MSE, steps=65))}, r"\.steps=65 must be an integer in 1\.\.64", True),
    "max_shrink": ({"weight": dict(W4, clip=dict(MSE, max_shrink=1.5))}, r"\.max_shrink=1\.5 must be a number in \(0, 1\]", True),
    "no candidate": ({"weight": dict(W4, clip=dict(MSE, max_shrink=0.01))}, r"floor\(max_shrink \* steps\) >= 1", True),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_clip_is_refused_by_layer_name(monkeypatch, case):
    from qdiff.base.base_quantizer import StaticQuantizer
    from qdiff.quarot.quarot_quant_layer import QuarotQuantizedLinear
    from qdiff.smooth_quant.sq_quant_layer import SQQuantizedLinear
    from qdiff.viditq.viditq_quant_layer import ViDiTQuantizedLinear

    _torch_weight_kernels(monkeypatch)
    cfg, text, value_error = REFUSALS[case]
    cls = {"viditq": ViDiTQuantizedLinear, "smooth_quant": SQQuantizedLinear, "quarot": QuarotQuantizedLinear}.get(case)

    def quantised(self, w):
        raise AssertionError("the layer is refused before any weight is quantised")

    monkeypatch.setattr(StaticQuantizer, "codes_and_dequant", quantised)
    with pytest.raises(ValueError if value_error else NotImplementedError, match=r"blocks\.1\.ffn\.0: weight\.clip.*" + text):
        _layer(cfg, 64, 64, cls=cls)


def test_without_clip_the_search_is_never_reached_and_mse_reaches_it(monkeypatch):
    from viditq_extension import fused

    _torch_weight_kernels(monkeypatch)
    calls = []

    def search(w, *args, **kw):
        calls.append((tuple(w.shape), args, kw))
        raise RuntimeError("reached the clip search")

    monkeypatch.setattr(fused, "clip_search", search)
    monkeypatch.setattr(fused, "clip_search_blocks", search)
    plain, _ = _layer({"weight": W4, "gptq": GPTQ}, 24, 64)
    plain.refresh()
    plain.requantize_gptq_(torch.eye(64))
    assert plain.clip is None and plain.w_quantizer.clip is None and not calls
    with pytest.raises(NotImplementedError, match=r"blocks\.1\.ffn\.0: requantize_clip_ needs weight\.clip\.search: diag or hessian"):
        plain.requantize_clip_(torch.eye(64))
    with pytest.raises(RuntimeError, match="reached the clip search"):
        _layer({"weight": dict(W4, clip=MSE)}, 24, 64)
    assert calls == [((24 * 2, 32), (4, False, -8, 7, 20, 10), {"chan_w": None, "want_table": False})]  # the rows of w.view(-1, g), AWQ's defaults
    # `diag` / `hessian` are PTQ steps: the constructor holds the s = 0 grid, which is the un-clipped layer's
    late, _ = _layer({"weight": dict(W4, clip={"search": "hessian"})}, 24, 64)
    assert len(calls) == 1 and torch.equal(late.w_quantizer.delta, plain.w_quantizer.delta)
    with pytest.raises(ValueError, match=r"blocks\.1\.ffn\.0: the Hessian is \(32, 32\)"):
        late.requantize_clip_(torch.eye(32))
    with pytest.raises(RuntimeError, match="reached the clip search"):
        late.requantize_clip_(torch.eye(64))
    assert calls[1][0] == (24, 64) and tuple(calls[1][1][0].shape) == (2, 32, 32)  # the whole weight and the [K / g, g, g] blocks


def test_reference_format_and_a_missing_hessian_name_the_layer(monkeypatch):
    from qdiff import config as qcfg
    from qdiff.base import gptq
    from wan.quant_wanx import QuantWanModel

    _torch_weight_kernels(monkeypatch)
    cfg = {"weight": {"n_bits": 8, "sym": False, "clip": {"search": "diag"}}}
    net = _Net()
    net.lin, _ = _layer(cfg, 24, 64, name="lin")
    net.q_cfg = qcfg.create(cfg)
    with pytest.raises(NotImplementedError, match=r"lin: the reference's int_weight\.pt format derives its grid"):
        QuantWanModel.quantize_and_save_weight(net, reference_format=True)
    with pytest.raises(KeyError, match=r"lin: no Hessian for this layer in /data/hessian\.pth"):
        gptq.clip_model_(net, {}, "/data/hessian.pth")
    assert gptq.clip_needs_hessian(net.q_cfg) and not gptq.clip_needs_hessian(qcfg.create({"weight": dict(W4, clip=MSE)}))
