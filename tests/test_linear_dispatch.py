"""CPU-only pin of kernel mode's Linear dispatch: which GEMM entry a layer of each kind reaches through
WanAttentionBlockWithHipKernel._linear, which producer makes its operands from an _LnSrc and from an _FpSrc, that a second consumer of
a source reuses them, the out dtype, the GELU flag, that the fp32 stream goes in as `out`; the FFN's late-GELU rule over every ordered
pair of kinds; what the integer checkpoint holds and what `--dit_fsdp` shards, per kind; QuantizedLinear's kind for every shipped
config.  Nothing is launched: the qgemm entries and the fused producers are replaced by recorders that return empty tensors of the
right shape and dtype.  The numbers themselves: tests/test_gpu_block.py and the per-format GPU suites."""
import glob
import inspect
import itertools
import os

import pytest
import torch

from test_fp8_abi import PKG, lib  # noqa: F401 (`lib`: builds the library on a clean checkout)

K, N, ROWS = 128, 256, 200   # in_features, out_features; a row count that is no multiple of a tile
BF16, F32 = torch.bfloat16, torch.float32
ENTRIES = ("w8a8_linear", "w8a8_grouped_linear", "fp_linear", "wq16_linear", "wq16_grouped_linear", "fp8_linear", "mx_linear")


# ---- the layer properties this file reads ------------------------------------------------------------------------------------------
def _checkpointed(lin):
    return lin.checkpointed


def _sharded(lin):
    return lin.sharded


def _late_gelu(ffn0, ffn2):
    from wan.quant_wanx_hip import _late_gelu

    return _late_gelu(ffn0, ffn2)


def _kind(ql):
    return ql.kind


# ---- recorders -----------------------------------------------------------------------------------------------------------------------
class _ActQuantizer:
    """stands for a qdiff quantiser the fused producers do not implement (HipLinearW8A8.act_quantizer)"""
    sym = True

    def __init__(self, calls):
        self.calls = calls

    def quantize_int8(self, x, premul, rot):
        self.calls.append(("act_quantizer.quantize_int8", x.dtype))
        return torch.empty(x.shape, dtype=torch.int8), torch.empty(x.shape[0]), torch.empty(x.shape[0])


@pytest.fixture()
def rec(lib, monkeypatch):  # noqa: F811
    """-> (gemm calls [(entry, bound arguments)], producer calls [(name, detail)]) with every entry and producer replaced"""
    from viditq_extension import fused, qgemm

    gemms, prods = [], []

    def entry(name):
        sig = inspect.signature(getattr(qgemm, name))

        def call(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            args = dict(b.arguments)
            gemms.append((name, args))
            act, weight = list(args.values())[:2]
            if args["out"] is not None:
                return args["out"]
            return torch.empty(act.shape[0], weight.shape[0], dtype=args["out_dtype"] or act.dtype)
        return call

    for name in ENTRIES:
        monkeypatch.setattr(qgemm, name, entry(name))

    def ln_quant(name):
        return lambda q, *a: prods.append((name, q.dtype))

    monkeypatch.setattr(fused, "layernorm_nobias_t2i_quant_sum_fuse", ln_quant("layernorm_nobias_t2i_quant_sum_fuse"))
    monkeypatch.setattr(fused, "layernorm_rotate_quant", ln_quant("layernorm_rotate_quant"))
    monkeypatch.setattr(fused, "layernorm_nobias_t2i_fuse", ln_quant("layernorm_nobias_t2i_fuse"))

    def rows_fp8(x, gelu=False):
        prods.append(("quant_rows_fp8", x.dtype, gelu))
        return torch.empty(x.shape, dtype=torch.uint8), torch.empty(x.shape[0], dtype=F32)

    def rows_mx(x, fmt="mxfp8_e4m3", gelu=False):
        prods.append(("quant_rows_mx", x.dtype, gelu))
        assert fmt == "mxfp8_e4m3"
        return torch.empty(x.shape, dtype=torch.uint8), torch.empty(x.shape[0], x.shape[1] // 32, dtype=torch.uint8)

    def to_int8(name):
        def call(t, *a):
            prods.append((name, t.dtype))
            return torch.empty(t.shape, dtype=torch.int8)
        return call

    monkeypatch.setattr(fused, "quant_rows_fp8", rows_fp8)
    monkeypatch.setattr(fused, "quant_rows_mx", rows_mx)
    for name in ("quant_sum", "gelu_quant_sum", "rotate_quant"):
        monkeypatch.setattr(fused, name, to_int8(name))
    monkeypatch.setattr(fused, "gate_residual_into_", lambda residual, y, gate: prods.append(("gate_residual_into_", residual)))
    return gemms, prods


# ---- one layer of each kind ------------------------------------------------------------------------------------------------------------
KINDS = ("w8a8", "w8a8_rot", "w8a8_g128", "w8a8_actq", "fp_torch", "fp_hip", "wq16", "wq16_g64", "fp8", "mxfp8", "mxfp4")
# kind -> (entry, _LnSrc producers, _FpSrc producers, checkpointed, sharded)
EXPECT = {
    "w8a8": ("w8a8_linear", [("layernorm_nobias_t2i_quant_sum_fuse", torch.int8)], [("quant_sum", BF16)], True, ("weight",)),
    "w8a8_rot": ("w8a8_linear", [("layernorm_rotate_quant", torch.int8)], [("rotate_quant", BF16)], True, ("weight",)),
    "w8a8_g128": ("w8a8_grouped_linear", [("layernorm_nobias_t2i_quant_sum_fuse", torch.int8)], [("quant_sum", BF16)], True, ("weight",)),
    "w8a8_actq": ("w8a8_linear", [("layernorm_nobias_t2i_fuse", F32), ("act_quantizer.quantize_int8", F32)],
                  [("act_quantizer.quantize_int8", F32)], True, ("weight",)),
    "fp_torch": (None, [("layernorm_nobias_t2i_fuse", BF16)], [], False, ("weight",)),
    "fp_hip": ("fp_linear", [("layernorm_nobias_t2i_fuse", BF16)], [], False, ("weight",)),
    "wq16": ("wq16_linear", [("layernorm_nobias_t2i_fuse", BF16)], [], True, ("weight",)),
    "wq16_g64": ("wq16_grouped_linear", [("layernorm_nobias_t2i_fuse", BF16)], [], True, ("weight",)),
    "fp8": ("fp8_linear", [("layernorm_nobias_t2i_fuse", F32), ("quant_rows_fp8", F32, False)], [("quant_rows_fp8", BF16, False)], True,
            ("weight",)),
    "mxfp8": ("mx_linear", [("layernorm_nobias_t2i_fuse", F32), ("quant_rows_mx", F32, False)], [("quant_rows_mx", BF16, False)], True,
              ("weight", "scale_weight")),
    "mxfp4": ("mx_linear", [("layernorm_nobias_t2i_fuse", F32), ("quant_rows_mx", F32, False)], [("quant_rows_mx", BF16, False)], True,
              ("weight", "scale_weight")),
}
UNFUSED = ("w8a8_actq", "fp_torch")  # GELU and gate + residual as separate passes behind a plain GEMM


def make(kind, calls=None):
    from wan import quant_wanx_hip as H

    if kind in ("w8a8", "w8a8_rot", "w8a8_actq"):
        m = H.HipLinearW8A8(K, N)
        if kind == "w8a8_rot":
            m.act_premul, m.rot = torch.ones(K), (1, None)
        if kind == "w8a8_actq":
            m.__dict__["act_quantizer"] = _ActQuantizer([] if calls is None else calls)
        return m
    if kind == "w8a8_g128":
        return H.HipLinearW8A8(K, N, w_bits=4, group_size=128)
    if kind in ("fp_torch", "fp_hip"):
        return H.HipLinearFp(torch.zeros(N, K), torch.zeros(N), BF16, kind[3:])
    if kind in ("wq16", "wq16_g64"):
        return H.HipLinearWq16(K, N, group_size=64 if kind == "wq16_g64" else None)
    if kind == "fp8":
        return H.HipLinearFp8(K, N)
    return H.HipLinearMx(K, N, w_fmt={"mxfp8": "mxfp8_e4m3", "mxfp4": "mxfp4_e2m1"}[kind])


def sources(blk, gelu=False):
    from wan.quant_wanx_hip import _FpSrc, _LnSrc

    return {"ln": _LnSrc(blk, torch.zeros(ROWS, K), None, torch.zeros(1, K), torch.zeros(1, K)),
            "fp": _FpSrc(torch.zeros(ROWS, K, dtype=BF16), gelu=gelu)}


@pytest.fixture()
def blk(lib):  # noqa: F811
    from wan.quant_wanx_hip import WanAttentionBlockWithHipKernel

    return WanAttentionBlockWithHipKernel(K, N, 1)


# ---- _linear ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_name", ["ln", "fp"])
@pytest.mark.parametrize("kind", KINDS)
def test_linear_reaches_the_entry_of_its_kind_with_operands_made_once(rec, blk, kind, src_name):
    gemms, prods = rec
    lin = make(kind, prods)
    entry, want_ln, want_fp = EXPECT[kind][:3]
    want = want_ln if src_name == "ln" else want_fp
    src = sources(blk)[src_name]
    y = blk._linear(lin, src)
    assert [p for p in prods if p[0] != "gate_residual_into_"] == want, prods
    assert [g[0] for g in gemms] == ([entry] if entry else [])
    assert y.dtype == BF16 and tuple(y.shape) == (ROWS, N)
    if entry:
        args = gemms[0][1]
        assert args["out_dtype"] == (F32 if kind == "w8a8_actq" else BF16)
        assert args["gelu"] is False and args["gate"] is None and args["residual"] is None and args["out"] is None
        if entry == "mx_linear":
            assert args["w_fmt"] == lin.mx
        if "grouped" in entry:
            assert args["group_size"] == lin.group_size
    # a second consumer of the same source and form: the operands are there already (the unfused path quantises per layer)
    n = len(prods)
    first = list(gemms[0][1].values())[0] if entry else None
    blk._linear(make(kind, prods) if kind not in ("w8a8_rot", "w8a8_actq") else lin, src)
    if kind == "w8a8_actq":
        assert prods[n:] == [("act_quantizer.quantize_int8", F32)]
    else:
        assert prods[n:] == []
        assert entry is None or list(gemms[1][1].values())[0] is first


@pytest.mark.parametrize("src_name", ["ln", "fp"])
@pytest.mark.parametrize("kind", KINDS)
def test_linear_with_gelu(rec, blk, kind, src_name):
    gemms, prods = rec
    lin = make(kind, prods)
    y = blk._linear(lin, sources(blk)[src_name], gelu=True)
    assert y.dtype == BF16 and tuple(y.shape) == (ROWS, N)
    assert not any(p[0] == "gate_residual_into_" for p in prods)
    if EXPECT[kind][0]:
        args = gemms[0][1]
        assert args["gelu"] is (kind not in UNFUSED) and args["out_dtype"] == (F32 if kind == "w8a8_actq" else BF16)
        assert args["gate"] is None and args["residual"] is None and args["out"] is None


@pytest.mark.parametrize("src_name", ["ln", "fp"])
@pytest.mark.parametrize("kind", KINDS)
def test_linear_with_gate_and_residual_updates_the_stream_in_place(rec, blk, kind, src_name):
    gemms, prods = rec
    lin = make(kind, prods)
    gate, stream = torch.ones(N), torch.zeros(ROWS, N)
    y = blk._linear(lin, sources(blk)[src_name], gate=gate, residual=stream)
    assert y is stream
    unfused = [p for p in prods if p[0] == "gate_residual_into_"]
    if kind in UNFUSED:
        assert len(unfused) == 1 and unfused[0][1] is stream
    else:
        assert not unfused
    if EXPECT[kind][0]:
        args = gemms[0][1]
        assert args["out_dtype"] == F32 and args["gelu"] is False
        if kind == "w8a8_actq":
            assert args["gate"] is None and args["residual"] is None and args["out"] is None
        else:
            assert args["gate"] is gate and args["residual"] is stream and args["out"] is stream   # no copy of the gate


@pytest.mark.parametrize("kind,want", [("w8a8", [("gelu_quant_sum", BF16)]), ("fp8", [("quant_rows_fp8", BF16, True)]),
                                       ("mxfp8", [("quant_rows_mx", BF16, True)]), ("w8a8_actq", [("act_quantizer.quantize_int8", F32)])])
def test_a_pre_activation_source_hands_the_gelu_to_the_quantiser(rec, blk, kind, want):
    gemms, prods = rec
    blk._linear(make(kind, prods), sources(blk, gelu=True)["fp"])
    assert prods == want and gemms[0][1]["gelu"] is False


# ---- late GELU, checkpoint, shards -----------------------------------------------------------------------------------------------------
def test_late_gelu_truth_table_over_all_ordered_pairs_of_kinds():
    """true when ffn.0 and ffn.2 consume the same quantised form and ffn.2's quantiser takes the plain row (it applies the GELU itself)"""
    int8 = ("w8a8", "w8a8_rot", "w8a8_g128", "w8a8_actq")
    mx = ("mxfp8", "mxfp4")
    for a, b in itertools.product(KINDS, KINDS):
        want = (a in int8 and b in int8 and b != "w8a8_rot") or (a == b == "fp8") or (a in mx and b in mx)
        assert bool(_late_gelu(make(a), make(b))) is want, (a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_checkpointed_and_sharded_per_kind(kind):
    lin = make(kind)
    assert bool(_checkpointed(lin)) is EXPECT[kind][3]
    assert tuple(_sharded(lin)) == EXPECT[kind][4]


def test_the_kinds_that_hold_a_zero_point_or_a_premultiplier_still_read_their_buffers():
    for kind in ("w8a8", "w8a8_g128", "wq16", "wq16_g64"):   # asymmetric weights: the zero point is a buffer, and the GEMM's operand
        lin = make(kind)
        assert lin.zp_weight is not None and "zp_weight" in dict(lin.named_buffers())
        assert lin.zp is (lin.zp_gemm if lin.w_bits == 4 else lin.zp_weight)
    rot = make("w8a8_rot")
    assert rot.act_premul is not None and "act_premul" in dict(rot.named_buffers()) and rot.rot == (1, None)
    for kind in ("fp8", "mxfp8", "mxfp4", "wq16"):
        assert make(kind).act_premul is None
    for kind in ("fp8", "mxfp8", "mxfp4"):
        assert make(kind).zp_weight is None


@pytest.mark.parametrize("kind", ["w8a8", "fp_torch", "wq16", "fp8", "mxfp4"])
def test_fsdp_slots_follow_the_layers_sharded_names_in_layer_order(blk, kind):
    from wan.distributed.fsdp import _weight_slots

    lins = [make(kind) for _ in range(10)]
    for attn, four in ((blk.self_attn, lins[:4]), (blk.cross_attn, lins[4:8])):
        attn.q, attn.k, attn.v, attn.o = four
    blk.ffn0, blk.ffn2 = lins[8:]
    slots = _weight_slots(blk)
    assert [(id(o), a) for o, a in slots] == [(id(l), a) for l in lins for a in EXPECT[kind][4]]


# ---- QuantizedLinear names its kind ---------------------------------------------------------------------------------------------------
CONFIG_KIND = {"config": "int8", "w4a16_all_linears": "weight_only", "w4a16_g128_all_linears": "weight_only",
               "w4a8_g128_all_linears": "int8_grouped", "w4a8_mixed": "int8", "w4a8_mixed_viditq": "int8",
               "w4a8_mxfp4_all_linears": "mx", "w8a16_all_linears": "weight_only", "w8a8_all_linears": "int8",
               "w8a8_all_linears_attn_full": "int8", "w8a8_all_linears_attn_map": "int8", "w8a8_all_linears_attn_map_cross": "int8",
               "w8a8_all_linears_qk8": "int8", "w8a8_fp8_all_linears": "fp8", "w8a8_mxfp8_all_linears": "mx", "w8a8_plain": "int8"}


def test_every_shipped_config_is_listed():
    found = {os.path.basename(f)[:-5] for f in glob.glob(os.path.join(PKG, "quant_configs", "*.yaml"))}
    assert found == set(CONFIG_KIND)


@pytest.mark.parametrize("cfg_name", sorted(CONFIG_KIND))
def test_quantized_linear_kind_for_every_shipped_config(lib, monkeypatch, cfg_name):  # noqa: F811
    """one self_attn.q of each config, built without a GPU: on the meta device and without quantising the weight for the integer
    formats (their weight quantiser has no host path), in host memory for fp8 / MX, as tests/test_fp8_abi.py builds its layers"""
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from qdiff.base.quant_model import pick_layer_type

    cfg = qcfg.load(os.path.join(PKG, "quant_configs", cfg_name + ".yaml"))
    name = "blocks.0.self_attn.q"
    host = CONFIG_KIND[cfg_name] in ("fp8", "mx")
    if not host:
        monkeypatch.setattr(QuantizedLinear, "_requantize", lambda self, w: None)
    fp = torch.nn.Linear(K, N, device="cpu" if host else "meta")
    ql = pick_layer_type(cfg, name)(K, N, True, fp.weight.device, cfg, fp, module_name=name)
    assert _kind(ql) == CONFIG_KIND[cfg_name]
    ql.quant_mode = False            # mixed_precision index 0, or the caller's switch: the FP module
    assert _kind(ql) == "fp"
    ql.quant_mode = True
    ql.w_quantizer = None            # no `weight:` section
    assert _kind(ql) == "fp"
