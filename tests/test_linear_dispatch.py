"""CPU-only pin of kernel mode's Linear dispatch: which GEMM entry a layer of each kind reaches through
WanAttentionBlockWithHipKernel._linear, which producer makes its operands from an _LnSrc and from an _FpSrc, that a second consumer of
a source reuses them, the out dtype, the GELU flag, that the fp32 stream goes in as `out`; the FFN's late-GELU rule over every ordered
pair of kinds; what the integer checkpoint holds and what `--dit_fsdp` shards, per kind; QuantizedLinear's kind for every shipped
config; and the same for every form of HipLinearMx (MX_FORMS), each built from a QuantizedLinear of its shipped config.  Nothing is
launched: the qgemm entries and the fused producers are replaced by recorders that return empty tensors of the right shape and
dtype.  The numbers themselves: tests/test_gpu_block.py and the per-format GPU suites."""
import glob
import inspect
import itertools
import os

import pytest
import torch

from test_fp8_abi import PKG, lib  # noqa: F401 (`lib`: builds the library on a clean checkout)

K, N, ROWS = 128, 256, 200   # in_features, out_features; a row count that is no multiple of a tile
BF16, F32 = torch.bfloat16, torch.float32
ENTRIES = ("w8a8_linear", "w8a8_grouped_linear", "fp_linear", "wq16_linear", "wq16_grouped_linear", "fp8_linear", "mx_linear", "mx4_linear",
           "mx6_linear", "mx_mixed_linear", "mx4_lowrank_linear")
MX_BLOCK_BYTES = {"mxfp8_e4m3": 32, "mxfp6_e2m3fn": 24, "mxfp4_e2m1": 16}   # bytes of 32 codes, by format


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

    def rows_mx(x, fmt="mxfp8_e4m3", gelu=False, had32=False):
        """(the e4m3 form without a rotation is recorded as it always was; every other form adds its fmt and had32)"""
        prods.append(("quant_rows_mx", x.dtype, gelu) + (() if (fmt, had32) == ("mxfp8_e4m3", False) else (fmt, had32)))
        return (torch.empty(x.shape[0], x.shape[1] // 32 * MX_BLOCK_BYTES[fmt], dtype=torch.uint8),
                torch.empty(x.shape[0], x.shape[1] // 32, dtype=torch.uint8))

    def rows_mx_mixed(x, perm, n8, gelu=False):
        prods.append(("quant_rows_mx_mixed", x.dtype, gelu, perm, n8))
        return (torch.empty(x.shape[0], n8 + (x.shape[1] - n8) // 2, dtype=torch.uint8),
                torch.empty(x.shape[0], x.shape[1] // 32, dtype=torch.uint8))

    def rows_mxfp4_project(x, a16, gelu=False, had32=False, ldt=None, out=None):
        prods.append(("quant_rows_mxfp4_project", x.dtype, gelu, had32, a16))
        return (torch.empty(x.shape[0], x.shape[1] // 2, dtype=torch.uint8), torch.empty(x.shape[0], x.shape[1] // 32, dtype=torch.uint8),
                torch.empty(x.shape[0], a16.shape[0], dtype=a16.dtype))

    def to_int8(name):
        def call(t, *a):
            prods.append((name, t.dtype))
            return torch.empty(t.shape, dtype=torch.int8)
        return call

    monkeypatch.setattr(fused, "quant_rows_fp8", rows_fp8)
    monkeypatch.setattr(fused, "quant_rows_mx", rows_mx)
    monkeypatch.setattr(fused, "quant_rows_mx_mixed", rows_mx_mixed)
    monkeypatch.setattr(fused, "quant_rows_mxfp4_project", rows_mxfp4_project)
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


# ---- every form of HipLinearMx, built from a QuantizedLinear of its shipped config -------------------------------------------------------
FP8, FP6, FP4 = "mxfp8_e4m3", "mxfp6_e2m3fn", "mxfp4_e2m1"
# form -> (config, in_features, entry, how its input is made: the row quantiser's (fmt, had32), "project" or "mixed"; act form;
#          weight columns; the buffers it registers beyond weight / scale_weight / bias, in order)
MX_FORMS = {
    "w8a8": ("w8a8_mxfp8_all_linears", K, "mx_linear", (FP8, False), "mxfp8", K, []),
    "w4a8": ("w4a8_mxfp4_all_linears", K, "mx_linear", (FP8, False), "mxfp8", K // 2, []),
    "w4a4": ("mx/w4a4_mxfp4_all_linears", K, "mx4_linear", (FP4, False), "mxfp4", K // 2, []),
    "w4a4_h32": ("mx/w4a4_mxfp4_had32_all_linears", K, "mx4_linear", (FP4, True), "mxfp4_h32", K // 2, ["mx_had32"]),
    "w6a6": ("mx/w6a6_mxfp6_all_linears", K, "mx6_linear", (FP6, False), "mxfp6", K // 4 * 3, ["mx_fmt"]),
    "w4a6": ("mx/w4a6_mxfp4_mxfp6_all_linears", K, "mx6_linear", (FP6, False), "mxfp6", K // 2, ["mx_fmt"]),
    "w4a4_lr": ("lowrank/w4a4_mxfp4_lr32_all_linears", K, "mx4_lowrank_linear", "project", "mxfp4", K // 2, ["lr_a", "lr_b"]),
    "w4a4_h32_lr": ("lowrank/w4a4_mxfp4_had32_lr32_all_linears", K, "mx4_lowrank_linear", "project", "mxfp4_h32", K // 2,
                    ["mx_had32", "lr_a", "lr_b"]),
    "w4a4_o128": ("mx/w4a4_mxfp4_o128_all_linears", 256, "mx_mixed_linear", "mixed", "mxmix128", 128 + 64, ["mx_perm", "mx_n8"]),
}
MX_W_FMT = {"w8a8": FP8, "w6a6": FP6}   # (every other form: e2m1 weights)
_QL = {}


def make_mx(form, name="blocks.0.self_attn.q"):
    """a HipLinearMx of `form`, converted from a QuantizedLinear of the shipped config (made once per form and name, in host memory)"""
    from qdiff import config as qcfg
    from qdiff.base.quant_layer import QuantizedLinear
    from wan.quant_wanx_hip import _to_hip_linear

    cfg_name, k = MX_FORMS[form][:2]
    if (form, name) not in _QL:
        g = torch.Generator().manual_seed(5)
        fp = torch.nn.Linear(k, N)
        fp.weight.data.copy_(torch.randn(N, k, generator=g) * k ** -0.5)
        ql = QuantizedLinear(k, N, True, "cpu", qcfg.load(os.path.join(PKG, "quant_configs", cfg_name + ".yaml")), fp, module_name=name)
        if ql.mx_n8 is not None:   # the order of an outlier layer: from a seeded calibration absmax, the same for every layer made here
            ql.select_outlier_perm(torch.rand(k, generator=torch.Generator().manual_seed(6)))
        _QL[form, name] = ql
    return _to_hip_linear(_QL[form, name], None, False, BF16, "torch", name)


def mx_sources(blk, k, gelu=False):
    from wan.quant_wanx_hip import _FpSrc, _LnSrc

    return {"ln": _LnSrc(blk, torch.zeros(ROWS, k), None, torch.zeros(1, k), torch.zeros(1, k)),
            "fp": _FpSrc(torch.zeros(ROWS, k, dtype=BF16), gelu=gelu)}


def _mx_producers(lin, how, row_dtype, gelu=False):
    """what one consumer of a fresh source asks of the producers, behind the _LnSrc's fp32 row when there is one"""
    if how == "project":
        return [("quant_rows_mxfp4_project", row_dtype, gelu, lin.had32, lin.lr_a)]
    if how == "mixed":
        return [("quant_rows_mx_mixed", row_dtype, gelu, lin.mx_perm, 128)]
    return [("quant_rows_mx", row_dtype, gelu) + (() if how == (FP8, False) else how)]


def _same(got, want):
    """producer records compared with tensors by identity (a perm or a factor is the layer's own buffer, not a copy)"""
    return len(got) == len(want) and all(len(g) == len(w) and all(a is b if isinstance(b, torch.Tensor) else a == b for a, b in zip(g, w))
                                         for g, w in zip(got, want))


@pytest.mark.parametrize("src_name", ["ln", "fp"])
@pytest.mark.parametrize("form", sorted(MX_FORMS))
def test_every_mx_form_reaches_its_entry_with_operands_made_once(rec, blk, form, src_name):
    gemms, prods = rec
    _, k, entry, how, act_form, w_cols, _ = MX_FORMS[form]
    lin = make_mx(form)
    assert lin.act_form == lin.act_key == act_form and lin.plain_rows
    src = mx_sources(blk, k)[src_name]
    y = blk._linear(lin, src)
    ln = [("layernorm_nobias_t2i_fuse", F32)] if src_name == "ln" else []
    assert _same(prods, ln + _mx_producers(lin, how, F32 if src_name == "ln" else BF16)), prods
    assert [g[0] for g in gemms] == [entry] and y.dtype == BF16 and tuple(y.shape) == (ROWS, N)
    args = gemms[0][1]
    assert args["out_dtype"] == BF16 and args["gelu"] is False and args["gate"] is None and args["residual"] is None and args["out"] is None
    assert args["w_q"] is lin.weight and args["w_scale"] is lin.scale_weight and args["bias"] is lin.bias
    a_cols = {"mxfp8": k, "mxfp6": k // 4 * 3, "mxfp4": k // 2, "mxfp4_h32": k // 2, "mxmix128": 128 + (k - 128) // 2}[act_form]
    assert tuple(args["a_q"].shape) == (ROWS, a_cols) and tuple(args["a_scale"].shape) == (ROWS, k // 32)
    assert tuple(lin.weight.shape) == (N, w_cols)
    if entry in ("mx_linear", "mx6_linear"):
        assert args["w_fmt"] == lin.mx == MX_W_FMT.get(form, FP4)
    if entry == "mx_mixed_linear":
        assert args["n8"] == 128
    if entry == "mx4_lowrank_linear":
        assert args["b"] is lin.lr_b and tuple(args["t"].shape) == (ROWS, 64) and args["t"].dtype == BF16
    # a second consumer of the same source and form is served the copy; with a branch it asks for its own t, and gets the same codes
    n = len(prods)
    other = make_mx(form, "blocks.0.self_attn.k")
    blk._linear(other, src)
    assert gemms[1][1]["a_q"] is args["a_q"] and gemms[1][1]["a_scale"] is args["a_scale"]
    assert _same(prods[n:], _mx_producers(other, how, F32 if src_name == "ln" else BF16) if how == "project" else [])
    blk._linear(lin, src)        # ... and the first consumer again: nothing is made twice
    assert len(prods) == n + (how == "project")
    if how == "project":
        assert gemms[2][1]["t"] is args["t"]


@pytest.mark.parametrize("form", sorted(MX_FORMS))
def test_every_mx_form_with_gelu_and_with_gate_and_residual(rec, blk, form):
    gemms, prods = rec
    k, how = MX_FORMS[form][1], MX_FORMS[form][3]
    lin = make_mx(form)
    blk._linear(lin, mx_sources(blk, k)["fp"], gelu=True)
    assert gemms[0][1]["gelu"] is True and gemms[0][1]["out_dtype"] == BF16
    gate, stream = torch.ones(N), torch.zeros(ROWS, N)
    assert blk._linear(lin, mx_sources(blk, k)["ln"], gate=gate, residual=stream) is stream
    args = gemms[1][1]
    assert args["out_dtype"] == F32 and args["gelu"] is False and args["gate"] is gate and args["residual"] is stream and args["out"] is stream
    del prods[:]                 # a pre-activation source hands the GELU to the producer of the form
    blk._linear(lin, mx_sources(blk, k, gelu=True)["fp"])
    assert _same(prods, _mx_producers(lin, how, BF16, gelu=True)) and gemms[2][1]["gelu"] is False
    assert not any(p[0] == "gate_residual_into_" for p in prods)


@pytest.mark.parametrize("form", ["w4a4_lr", "w4a4_h32_lr"])
def test_q_k_v_with_branches_get_one_projection_of_the_stacked_factor(rec, blk, form):
    gemms, prods = rec
    lins = [make_mx(form, f"blocks.0.self_attn.{l}") for l in "qkv"]
    src = mx_sources(blk, K)["fp"]
    src.project(lins)
    assert len(prods) == 1 and prods[0][:4] == ("quant_rows_mxfp4_project", BF16, False, form == "w4a4_h32_lr")
    stacked = prods[0][4]
    assert tuple(stacked.shape) == (192, K) and torch.equal(stacked, torch.cat([l.lr_a for l in lins], 0))
    for i, lin in enumerate(lins):
        blk._linear(lin, src)
        t = gemms[i][1]["t"]
        assert tuple(t.shape) == (ROWS, 64) and t.stride() == (192, 1) and t.storage_offset() == 64 * i
        assert t._base is gemms[0][1]["t"]._base and gemms[i][1]["a_q"] is gemms[0][1]["a_q"] and gemms[i][1]["b"] is lin.lr_b
    assert len(prods) == 1       # the three GEMMs asked for nothing more
    src2 = mx_sources(blk, K)["fp"]     # the stacked factor is kept on its first consumer: the next source gets the same tensor
    src2.project(lins)
    assert prods[1][4] is stacked


@pytest.mark.parametrize("form", sorted(MX_FORMS))
def test_every_mx_form_holds_its_buffers_and_shards_its_codes(form):
    _, k, _, _, _, w_cols, extra = MX_FORMS[form]
    lin = make_mx(form)
    ql = _QL[form, "blocks.0.self_attn.q"]
    assert tuple(lin.weight.shape) == (N, w_cols) and lin.weight.dtype == torch.uint8 and torch.equal(lin.weight, ql._codes)
    assert tuple(lin.scale_weight.shape) == (N, k // 32) and lin.scale_weight.dtype == torch.uint8
    assert [n for n, _ in lin.named_buffers()] == ["weight", "scale_weight", "bias"] + extra
    assert tuple(_sharded(lin)) == ("weight", "scale_weight") and bool(_checkpointed(lin))
    assert lin.act_premul is None and lin.zp_weight is None and not lin.quantized and not lin.fp8 and not lin.weight_only
    if "mx_fmt" in extra:
        assert lin.mx_fmt.dtype == torch.uint8 and lin.mx_fmt.tolist() == [2 if form == "w6a6" else 1, 2]
    if "mx_had32" in extra:
        assert lin.mx_had32.dtype == torch.uint8 and lin.mx_had32.tolist() == [1] and lin.had32 is True
    if "mx_n8" in extra:
        assert lin.mx_n8.dtype == torch.int32 and lin.mx_n8.tolist() == [128] and lin.n8 == 128
        assert lin.mx_perm.dtype == torch.int32 and torch.equal(lin.mx_perm, ql.mx_perm) and sorted(lin.mx_perm.tolist()) == list(range(k))
    if "lr_a" in extra:
        assert tuple(lin.lr_a.shape) == (64, k) and tuple(lin.lr_b.shape) == (N, 64) and lin.lr_a.dtype == lin.lr_b.dtype == BF16
        assert lin.low_rank == 32 and lin.has_branch
    else:
        assert not lin.has_branch


def test_late_gelu_of_every_mx_form_against_every_form_and_kind():
    """true exactly when both layers consume one activation form: W8A8 with W4A8 (and the KINDS' "mxfp8" / "mxfp4", which are those two), W4A4
    with its low-rank form, each rotated form with the other, W6A6 with W4A6, the outlier form with itself; never with another kind"""
    forms = {f: make_mx(f) for f in MX_FORMS}
    act = {f: MX_FORMS[f][4] for f in MX_FORMS}
    for a, b in itertools.product(MX_FORMS, MX_FORMS):
        assert bool(_late_gelu(forms[a], forms[b])) is (act[a] == act[b]), (a, b)
    for f, kind in itertools.product(MX_FORMS, KINDS):
        want = act[f] == "mxfp8" and kind in ("mxfp8", "mxfp4")
        assert bool(_late_gelu(forms[f], make(kind))) is want and bool(_late_gelu(make(kind), forms[f])) is want, (f, kind)


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
