"""LayerNorm + modulate fused into the fp8 / MX row quantisers (csrc/rowwise.hip ln_modulate_row; fused.layernorm_quant_rows_*;
_LnSrc.prefetch_rows).  (a) codes and scales EQUAL those of the two launches replaced, layernorm_nobias_t2i_fuse into fp32 then
quant_rows_*.  (b) against LayerNorm + modulate in float64 in host memory, rounded once to fp32, through the host quantisers, both
sides dequantised: fp32 and fp64 statistics differ by ulps, which can move an element over a rounding boundary or a block maximum
over a power of two, so per element, with S = max(scale, reference scale) and (emin, mbits) = (-6, 3) e4m3, (0, 1) e2m1, (0, 3) e2m3,
|a - b| <= S 2^(max(floor(log2(max(|a|, |b|) / S)), emin) - mbits)   (one scale: neighbouring codes; two: each within half a step of its grid or, where the finer grid clips, one step of the coarser);
fp8's row scales S, S' are fp32 quotients that differ in their last bits: + max(|a|, |b|) |S - S'| / min(S, S').  The share of
elements that differ at all is measured for the two launches and must be the same SET for the fused entry (profiles/PARITY_NOTES.md).
(c) a kernel-mode block forward with prefetch_rows equals the forward without it and launches no LayerNorm of its own."""
import os

import pytest
import torch

from test_gpu_fp8 import _tiny_model
from test_gpu_wq16 import DEV, PKG

pytestmark = pytest.mark.gpu
EPS = 1e-6
E4M3, E2M1, MX8, MX4 = (-6, 3), (0, 1), {"fmt": "mxfp8_e4m3"}, {"fmt": "mxfp4_e2m1"}
# form -> (the quantiser's name behind "quant_rows_" / "layernorm_quant_rows_", its arguments, (emin, mbits) of its codes)
FORMS = {"fp8": ("fp8", {}, E4M3), "mxfp8": ("mx", MX8, E4M3), "mxfp4": ("mx", MX4, E2M1), "mxfp6": ("mx", {"fmt": "mxfp6_e2m3fn"}, (0, 3)),
         "mxfp8_h32": ("mx", {**MX8, "had32": True}, E4M3), "mxfp4_h32": ("mx", {**MX4, "had32": True}, E2M1),
         "mxfp4_s": ("mx4_search", {}, E2M1), "mxfp4_h32_s": ("mx4_search", {"had32": True}, E2M1)}
MODS = ("gamma+shift+scale", "gamma+shift", "shift+scale")   # norm3 is the second (no mscale), norm1 / norm2 the third (no gamma)


def inputs(rows, cols, mods, dtype=torch.float32, seed=0):
    # x with outlier channels and a row offset; two batches of modulation rows as strided views of one [2, 6, cols]
    g = torch.Generator().manual_seed(seed + cols)
    x = torch.randn(rows, cols, generator=g) * (1 + 4 * (torch.rand(cols, generator=g) > 0.97)) + torch.randn(rows, 1, generator=g)
    e = (torch.randn(2, 6, cols, generator=g) * 0.3).to(DEV)
    gamma = (1 + 0.2 * torch.randn(cols, generator=g)).to(DEV) if "gamma" in mods else None
    return x.to(dtype).to(DEV), gamma, e[:, 0], e[:, 1] if "scale" in mods else None


def fused_and_two_launch(form, x, gamma, shift, scale):
    from viditq_extension import fused
    name, args, _ = FORMS[form]
    y = torch.empty(x.shape, dtype=torch.float32, device=DEV)
    fused.layernorm_nobias_t2i_fuse(y, x, gamma, shift, scale, EPS)
    return getattr(fused, "layernorm_quant_rows_" + name)(x, gamma, shift, scale, EPS, **args), getattr(fused, "quant_rows_" + name)(y, **args)


@pytest.mark.parametrize("cols", (64, 1536, 2080, 8960, 13824))   # one chunk, lanes idle; WPR 1, NCH 3; first WPR 4 width; the FFN widths
@pytest.mark.parametrize("form", FORMS)
def test_fused_entry_equals_the_two_launches_it_replaces(form, cols):
    # 262 = 2 x 131 rows: a surplus wave, two batches; 7 rows: one batch; 16-bit rows at one width; fp8 alone takes a width off 32
    cases = [(262, m, torch.float32, cols) for m in MODS] + [(7, MODS[0], torch.float32, cols)]
    cases += [(262, MODS[0], torch.bfloat16, cols), (262, MODS[2], torch.float16, cols)] if cols == 1536 else []
    cases += [(262, MODS[0], torch.float32, 2088)] if form == "fp8" and cols == 2080 else []
    for rows, mods, dtype, width in cases:
        x, gamma, shift, scale = inputs(rows, width, mods, dtype)
        (c, s), (c2, s2) = fused_and_two_launch(form, x, gamma, shift[:2 - rows % 2], scale[:2 - rows % 2] if scale is not None else None)
        assert c.dtype == c2.dtype and s.dtype == s2.dtype and torch.equal(s, s2) and torch.equal(c, c2), (rows, mods, dtype)


def dequant(form, codes, scales):
    from qdiff.base import base_quantizer as bq
    codes, scales = codes.cpu(), scales.cpu()
    if form == "fp8":
        return bq.fp8_decode(codes).double() * scales.double()[:, None], scales.double()[:, None].expand(codes.shape)
    return bq.mx_decode(codes, scales, FORMS[form][1].get("fmt", "mxfp4_e2m1"), torch.float64), torch.pow(2.0, scales.double() - 127).repeat_interleave(32, -1)


def host_reference(form, x, gamma, shift, scale):
    from qdiff.base import base_quantizer as bq
    name, args, _ = FORMS[form]
    x, rpb = x.double().cpu(), x.shape[0] // shift.shape[0]
    y = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + EPS)
    y = y * gamma.double().cpu() if gamma is not None else y
    y = y * (1 + scale.double().cpu().repeat_interleave(rpb, 0)) if scale is not None else y
    y = (y + shift.double().cpu().repeat_interleave(rpb, 0)).float()
    return dequant(form, *(bq.fp8_quant_rows(y) if form == "fp8" else
                           bq.mx_quant_rows_host(y, args.get("fmt", "mxfp4_e2m1"), had32=args.get("had32", False), search=name == "mx4_search")))


@pytest.mark.parametrize("cols", (64, 1536))
@pytest.mark.parametrize("form", FORMS)
def test_fused_entry_within_one_step_of_the_float64_reference(form, cols):
    emin, mbits = FORMS[form][2]
    for mods in MODS:
        x, gamma, shift, scale = inputs(262, cols, mods, seed=1)
        (c, s), (c2, s2) = fused_and_two_launch(form, x, gamma, shift, scale)
        (ref, ref_s), (got, got_s), (two, _) = host_reference(form, x, gamma, shift, scale), dequant(form, c, s), dequant(form, c2, s2)
        S, top = torch.maximum(got_s, ref_s), torch.maximum(got.abs(), ref.abs())
        step = S * torch.pow(2.0, torch.floor(torch.log2((top / S).clamp_min(2.0 ** emin))) - mbits)
        if form == "fp8":
            step = step + top * (got_s - ref_s).abs() / torch.minimum(got_s, ref_s)
        print(f"{form} cols {cols} {mods}: share of elements off the float64 reference {(got != ref).double().mean().item():.2e} "
              f"(two launches {(two != ref).double().mean().item():.2e}), worst err / step {((got - ref).abs() / step).max().item():.3f}")
        assert not ((got - ref).abs() > step).any() and torch.equal(got != ref, two != ref)


@pytest.mark.parametrize("cfg", ("w8a8_fp8_all_linears.yaml", "w8a8_mxfp8_all_linears.yaml", "mx/w4a4_mxfp4_had32_search_all_linears.yaml"))
def test_kernel_mode_block_with_prefetch_rows_equals_the_lazy_two_launch_path(cfg, monkeypatch):
    from qdiff import config as qcfg
    from viditq_extension import fused
    from wan import quant_wanx_hip as hip
    model, _, seq_len, ctx, lat0 = _tiny_model(qcfg.load(os.path.join(PKG, "quant_configs", cfg)), layers=1)
    model.hardware_forward_refactor()
    calls, real = [], fused.layernorm_nobias_t2i_fuse
    monkeypatch.setattr(fused, "layernorm_nobias_t2i_fuse", lambda out, *a: (calls.append(out.dtype), real(out, *a))[1])
    fused_out = model([lat0], torch.tensor([700], device=DEV), [ctx], seq_len)[0].float().clone()
    assert torch.isfinite(fused_out).all() and calls == []
    monkeypatch.setattr(hip._LnSrc, "prefetch_rows", lambda self, lins: None)
    lazy_out = model([lat0], torch.tensor([700], device=DEV), [ctx], seq_len)[0].float()
    assert calls == [torch.float32] * 3 and torch.equal(fused_out, lazy_out)
