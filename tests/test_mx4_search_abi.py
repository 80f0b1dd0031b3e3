"""CPU-only checks of the e2m1 block-scale rule `search` (wanq_quant_rows_mx4_search; `block_scale: search` of a `weight:` / `act:`
section): the host expression takes s0 + 1 exactly
where the float64 errors say so and never does worse than OCP's byte; the two shipped configs, the refusals by layer name, the key's
absence leaving today's codes, simulation mode's forward, kernel mode's activation forms and the checkpoint's record.
The kernel itself: tests/test_gpu_mx4_search.py."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_mx4_abi import FP4, FP8, YAML44, YAML44H
from test_mx_abi import YAML4, _cfg, _layer, _tiny_model

PKG = os.path.dirname(os.path.dirname(YAML4))
YAML44S = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_search_all_linears.yaml")
YAML44HS = os.path.join(PKG, "quant_configs", "mx", "w4a4_mxfp4_had32_search_all_linears.yaml")
CFGS = pytest.mark.parametrize("path,plain,had", [(YAML44S, YAML44, False), (YAML44HS, YAML44H, True)], ids=["plain", "had32"])


def search_rows(kind):
    """64 x 512 seeded rows, each with a scale of its own: "gauss", or "outlier" with one 8-sigma element in every block"""
    g = torch.Generator().manual_seed({"gauss": 11, "outlier": 12}[kind])
    x = torch.randn(64, 512, generator=g) * 2.0 ** torch.randint(-6, 7, (64, 1), generator=g).float()
    if kind == "outlier":
        x.view(64, 16, 32)[:, :, 3] = 8.0 * x.std(dim=1, keepdim=True)
    return x


def check_against_float64(x, codes, s, had32, kind):
    """The quantiser's (codes, bytes) for x against a float64 reference built from the format's table alone: OCP's byte from frexp,
    both candidates' codes as the nearest table value (ties to the even code), decoded by mx_decode, block errors summed in float64.
    The chosen byte is the argmin wherever the two errors differ by more than a relative 1e-5 (at most 1 % of the blocks are
    closer), the chosen error never exceeds OCP's, and on the outlier rows both branches are taken."""
    from qdiff.base.base_quantizer import E2M1_VALUES, mx_decode, mx_hadamard32_host, mx_pack_e2m1

    xr = (mx_hadamard32_host(x) if had32 else x).double().view(64, 16, 32)
    s0 = (torch.frexp(xr.abs().amax(-1))[1] - 1 + 127 - 2).clamp(0, 254)
    lut = torch.tensor(E2M1_VALUES, dtype=torch.float64)

    def err(sc, c=None):
        if c is None:
            t = (xr * 2.0 ** (127 - sc.double()).unsqueeze(-1)).reshape(64, 512)
            dist = (t.abs().clamp(max=6).unsqueeze(-1) - lut).abs()
            dist[..., 1::2] += 1e-12                      # a tie goes to the even code
            c = mx_pack_e2m1(dist.argmin(-1).to(torch.uint8) | (torch.signbit(t).to(torch.uint8) << 3))
        return ((mx_decode(c, sc.to(torch.uint8), FP4, torch.float64).view(64, 16, 32) - xr) ** 2).sum(-1)

    s = s.long()
    e0, e1, e = err(s0), err(s0 + 1), err(s, codes)
    assert bool(((s == s0) | (s == s0 + 1)).all())
    assert bool((e <= e0).all()), (e > e0).nonzero()[:4].tolist()
    clear = (e0 - e1).abs() > 1e-5 * torch.maximum(e0, e1)
    assert clear.float().mean() >= 0.99 and torch.equal((s != s0)[clear], (e1 < e0)[clear])
    if kind == "outlier":
        assert bool((s != s0).any()) and bool((s == s0).any())


@pytest.mark.parametrize("kind", ["gauss", "outlier"])
@pytest.mark.parametrize("had32", [False, True], ids=["plain", "had32"])
def test_host_expression_takes_the_float64_argmin_and_never_does_worse_than_ocp(had32, kind):
    """(the rows and seeds of tests/test_gpu_mx4_search.py: the host expression alone meets the conditions the kernel is held to)"""
    from qdiff.base.base_quantizer import mx_quant_rows_host

    x = search_rows(kind)
    check_against_float64(x, *mx_quant_rows_host(x, FP4, had32=had32, search=True), had32, kind)
    # the rule off is today's expression, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(mx_quant_rows_host(x, FP4, had32=had32, search=False), mx_quant_rows_host(x, FP4, False, had32)))
    with pytest.raises(ValueError, match="built for mxfp4_e2m1 only"):
        mx_quant_rows_host(x, FP8, search=True)


@CFGS
def test_shipped_configs_build_a_layer_whose_forward_is_the_decoded_product(path, plain, had):
    from qdiff.base.base_quantizer import mx_decode, mx_quant_rows_host

    cfg = _cfg(path)
    assert cfg.weight.block_scale == "search" and cfg.act.block_scale == "search" and cfg.weight.format == FP4 and cfg.act.format == FP4
    ql = _layer(cfg, K=256, N=24)
    assert ql.kind == "mx" and ql.mx_search_w and ql.mx_search_act and ql.mx_had32 is had
    w = ql.fp_module.weight.data * (0.03125 if had else 1.0)
    wc, ws = mx_quant_rows_host(w, FP4, had32=had, search=True)
    assert torch.equal(ql._codes, wc) and torch.equal(ql.w_quantizer.scale_u8, ws)
    x = torch.randn(1, 9, 256, generator=torch.Generator().manual_seed(2))
    a = mx_decode(*mx_quant_rows_host(x[0], FP4, had32=had, search=True), FP4)
    assert torch.equal(ql(x)[0], F.linear(a, mx_decode(wc, ws, FP4), ql.bias))
    # the key absent (and `floor` spelled out): today's layer, byte for byte
    old = _layer(_cfg(plain), K=256, N=24)
    assert not torch.equal(old._codes, ql._codes) and not old.mx_search_w and not old.mx_search_act
    for edits in ({"weight__block_scale": None, "act__block_scale": None}, {"weight__block_scale": "floor", "act__block_scale": "floor"}):
        off = _layer(_cfg(path, **edits), K=256, N=24)
        assert torch.equal(off._codes, old._codes) and torch.equal(off.w_quantizer.scale_u8, old.w_quantizer.scale_u8)
        assert torch.equal(off(x), old(x))


@pytest.mark.parametrize("base,edits,exc,text", [
    (YAML4, {"act__block_scale": "search"}, NotImplementedError, r"act\.block_scale: search is not supported with act\.format 'mxfp8_e4m3'"),
    (YAML44, {"weight__block_scale": "ceil"}, ValueError, r"weight\.block_scale='ceil' must be one of \('floor', 'search'\)"),
    (YAML44, {"act__block_scale": True}, ValueError, r"act\.block_scale=True must be one of"),
    (YAML44, {"act__block_scale": "search", "weight__low_rank": 8}, NotImplementedError, r"act\.block_scale: search with weight\.low_rank"),
    (YAML44, {"act__block_scale": "search", "mx__outlier_channels": 128}, NotImplementedError,
     r"act\.block_scale: search with mx\.outlier_channels"),
], ids=["other-format", "value", "bool", "low-rank", "outliers"])
def test_refusals_name_the_layer_and_the_key(base, edits, exc, text):
    cfg = _cfg(base)
    if "mx__outlier_channels" in edits:
        cfg["mx"] = type(cfg)({})
    for key, v in edits.items():
        sec, k = key.split("__")
        cfg[sec][k] = v
    with pytest.raises(exc, match=r"blocks\.0\.ffn\.0: " + text):
        _layer(cfg, K=256, N=24)


@pytest.mark.parametrize("option", ["low_rank", "outlier_channels"])
def test_weight_side_search_goes_with_the_options_the_act_side_refuses(option):
    """the weight is quantised offline: with `weight.low_rank` and with `mx.outlier_channels` (mx_quant_rows_mixed(search=True): the
    MXFP8 gather as ever, the MXFP4 gather under the rule), and the layer's activation form stays today's"""
    from qdiff.base.base_quantizer import mx_quant_rows_host
    from wan.quant_wanx_hip import _late_gelu, _to_hip_linear

    def build(rule):
        cfg = _cfg(YAML44, weight__block_scale=rule)
        if option == "low_rank":
            cfg["weight"]["low_rank"] = 8
        else:
            cfg["mx"] = type(cfg)({"outlier_channels": 128})
        ql = _layer(cfg, K=256, N=24)
        if option == "outlier_channels":
            ql.select_outlier_perm(torch.arange(256.0))
        return ql

    ql, old = build("search"), build("floor")
    assert ql.mx_search_w and not ql.mx_search_act and not torch.equal(ql.w_quantizer.scale_u8, old.w_quantizer.scale_u8)
    if option == "outlier_channels":
        w4 = ql.fp_module.weight.data[:, ql.mx_perm.long()[128:]]
        assert torch.equal(ql._codes[:, :128], old._codes[:, :128]) and torch.equal(ql._codes[:, 128:], mx_quant_rows_host(w4, FP4, search=True)[0])
    else:
        assert ql.lr_a is not None and torch.equal(ql._codes, mx_quant_rows_host(ql.fp_module.weight.data, FP4, search=True)[0])
    hl, ho = (_to_hip_linear(m, None, False, torch.bfloat16, "torch", "blocks.0.ffn.0") for m in (ql, old))
    assert not hl.search and hl.act_form == ho.act_form and _late_gelu(hl, ho) and [k for k, _ in hl.named_buffers()] == [k for k, _ in ho.named_buffers()]


def test_the_checkpoint_round_trips_the_rule_and_refuses_the_other_setting(tmp_path):
    from wan.quant_wanx_hip import HipLinearMx

    file = str(tmp_path / "search.pt")
    sd = _tiny_model(YAML44S).quantize_and_save_weight(file)
    rec = [k for k in sd if k.endswith(".mx_search")]
    assert len(rec) == 20 and all(sd[k].dtype == torch.uint8 and sd[k].tolist() == [1] for k in rec)
    fresh = _tiny_model(YAML44S).hardware_forward_refactor(load_path=file)
    lins = [m for m in fresh.hip_blocks.modules() if isinstance(m, HipLinearMx)]
    assert len(lins) == 20 and all(m.search and m.act_form == "mxfp4_s" and m._gemm == "mx4_linear" for m in lins)
    assert torch.equal(fresh.hip_blocks[1].ffn0.weight, sd["blocks.1.ffn.0.weight"])
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved with act\.block_scale: search.*built without it"):
        _tiny_model(YAML44).hardware_forward_refactor(load_path=file)
    plain = str(tmp_path / "plain.pt")
    assert not any(k.endswith(".mx_search") for k in _tiny_model(YAML44).quantize_and_save_weight(plain))
    with pytest.raises(ValueError, match=r"blocks\.0\.self_attn\.q was saved without act\.block_scale: search.*built with it"):
        _tiny_model(YAML44S).hardware_forward_refactor(load_path=plain)
