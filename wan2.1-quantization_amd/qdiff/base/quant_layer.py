"""QuantizedLinear: the base of the SmoothQuant / QuaRot / ViDiT variants (smooth_quant/, quarot/, viditq/), with everything they share.

Interface of ViDiT-Q/quant_utils/qdiff/base/quant_layer.py:8-74 (+ smooth_quant/sq_quant_layer.py,
quarot/quarot_quant_layer.py, viditq/viditq_quant_layer.py): ctor signature, attributes `fp_module`, `fp_weight`,
`w_quantizer`, `a_quantizer`, `quant_mode`, `use_kernel`, `module_name`, `channel_mask`, `rotation_matrix`, methods
`get_channel_mask`, `get_rotation_matrix`, `update_quantized_weight_*`.

What differs: `weight.data` still holds the fake-quantised (dequantised) weight for inspection / serialisation,
but forward() does not use it.  It uses int8 codes of that same weight and runs
    per-token quantise (optionally fused with x*mask -> Hadamard rotate)  ->  int8-MFMA GEMM + dequant epilogue.
The rotation is stored as its +-1 sign vector (`rotation_signs`); `rotation_matrix` materialises on demand."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from viditq_extension import qgemm

from ..config import ListConfig
from ..quarot import quarot_utils
from .base_quantizer import (FP8_FORMAT, MX_BLOCK, MX_FORMATS, MXFP4_FORMAT, MXFP6_FORMAT, MXFP8_FORMAT, DynamicQuantizer, Fp8Quantizer, MxQuantizer,
                             StaticQuantizer, fp8_decode, mx_decode)
from .gptq import BLOCK_MAX, gptq_prepare, gptq_section, gptq_solve
from .low_rank import RANK_MAX, LowRankBranch, fit_low_rank, padded_rank
from .mixed_precision_quantizer import MixedPrecisionDynamicQuantizer, MixedPrecisionStaticQuantizer


# format key -> (its n_bits, its name in "... is one N-bit format")
_FORMAT_BITS = {FP8_FORMAT: (8, "e4m3"), MXFP8_FORMAT: (8, MXFP8_FORMAT), MXFP4_FORMAT: (4, MXFP4_FORMAT), MXFP6_FORMAT: (6, MXFP6_FORMAT)}


class QuantizedLinear(LowRankBranch, nn.Linear):
    uses_mask = False
    uses_rotation = False

    def __init__(self, in_features, out_features, bias, device, quant_config, fp_module, module_name=None):
        super().__init__(in_features, out_features, bias, device)
        self.fp_module, self.q_cfg = fp_module, quant_config
        self.low_rank = self._checked_low_rank(quant_config, module_name)  # `weight.low_rank`: the LoRC rank (low_rank.py), or None
        self.mx = None  # the weight's MX format name (`format: mxfp8_e4m3` / `mxfp4_e2m1`), set by _checked_format
        self.mx_act = None  # ... and the activation's
        self.fp8 = self._checked_format(quant_config, module_name)
        self.mx_had32 = self._checked_mx_section(quant_config, module_name)  # `mx: {block_hadamard: True}`, W4A4 MX layers only
        # (an MX layer's `weight.group_size: 32` names the format's own block: there is no integer group-wise path behind it)
        self.group_size = None if self.mx else self._checked_group_size(quant_config, module_name, fp_module.weight.device)
        self.gptq = self._checked_gptq(quant_config, module_name)  # the `gptq:` section when it names this layer (gptq.py), or None
        self.w_quantizer = self.a_quantizer = None
        self.channel_mask = None
        self.rotation_signs = None
        self._premul = self._rot = None
        self.register_buffer("_codes", None, persistent=False)  # int8 [N,K], or uint8 [N,K/2] packed nibbles (4-bit weights)
        self._zp_gemm = self._wq16_vecs = None
        if quant_config.get("weight", None) is not None:
            wq = quant_config["weight"]
            self.w_quantizer = MxQuantizer(wq, self.mx_had32, weight_side=True) if self.mx else \
                (Fp8Quantizer if self.fp8 else
                 MixedPrecisionStaticQuantizer if isinstance(wq["n_bits"], ListConfig) else StaticQuantizer)(wq)
            self._requantize(fp_module.weight.data)
            self.w_quantizer.init_done = True
        else:
            self.weight.data = fp_module.weight.data
        self.fp_weight = fp_module.weight
        self.bias = fp_module.bias
        if quant_config.get("act", None) is not None:
            aq = quant_config["act"]
            self.a_quantizer = MxQuantizer(aq, self.mx_had32) if self.mx else \
                (Fp8Quantizer if self.fp8 else
                 MixedPrecisionDynamicQuantizer if isinstance(aq["n_bits"], ListConfig) else DynamicQuantizer)(aq)
        self.use_kernel = False
        self.quant_mode = True
        self.module_name = module_name

    def _checked_format(self, quant_config, module_name):
        """True when the config's `weight:` and `act:` sections both say `format: fp8_e4m3` (per-token dynamic e4m3 activations against
        per-channel e4m3 weights, wanq_gemm_fp8), False when neither has the key; every other combination is refused here, before
        any weight is quantised, and the message names the layer and the key."""
        wq, aq = quant_config.get("weight", None), quant_config.get("act", None)
        fw, fa = (None if wq is None else wq.get("format", None)), (None if aq is None else aq.get("format", None))
        if fw is None and fa is None:
            return False
        name = module_name or type(self).__name__
        for sec, f in (("weight", fw), ("act", fa)):
            if f is not None and f not in _FORMAT_BITS:
                raise ValueError(f"{name}: {sec}.format={f!r} is not a known format (the format keys are {FP8_FORMAT!r}, "
                                 f"{MXFP8_FORMAT!r} and {MXFP4_FORMAT!r}); OCP MXFP6 e2m3, a finite-only format, is spelled "
                                 f"{MXFP6_FORMAT!r}")
        if fw in MX_FORMATS or fa in MX_FORMATS:
            self._check_mx_format(name, wq, aq, fw, fa)
            self.mx, self.mx_act = fw, fa
            return False
        if fw is None or fa is None:
            raise NotImplementedError(f"{name}: format: {FP8_FORMAT} must be set in both the `weight:` and the `act:` section (it is "
                                      f"missing from `{'weight' if fw is None else 'act'}:`): the fp8 GEMM takes e4m3 codes on both sides")
        self._check_format_sections(name, (("weight", wq, fw), ("act", aq, fa)))
        if wq.get("group_size", None) is not None:
            raise NotImplementedError(f"{name}: weight.format with weight.group_size is not supported: the fp8 GEMM applies one weight "
                                      "scale per output channel")
        self._refuse_format_on_a_transformed_layer(name)
        return True

    def _check_format_sections(self, name, sections):
        """What every format asks of the section that names it: one bit width, the format's own (_FORMAT_BITS), and `sym: True`."""
        for sec, q, f in sections:
            bits, one = _FORMAT_BITS[f]
            if isinstance(q["n_bits"], ListConfig):
                raise NotImplementedError(f"{name}: {sec}.format with a bit-width list (mixed precision) is not supported: {one} is one "
                                          f"{bits}-bit format")
            if q["n_bits"] != bits:
                raise NotImplementedError(f"{name}: {sec}.format: {f} needs {sec}.n_bits: {bits} (it is {q['n_bits']!r})")
            if not q.get("sym", False):
                raise NotImplementedError(f"{name}: {sec}.format: {f} needs {sec}.sym: True: a floating-point code has no zero point")

    def _refuse_format_on_a_transformed_layer(self, name):
        if self.uses_mask or self.uses_rotation:
            raise NotImplementedError(f"{name}: weight.format / act.format with {type(self).__name__} is not supported: the SmoothQuant "
                                      "/ QuaRot / ViDiT layer classes condition an integer quantiser (leave the layer to the plain "
                                      "QuantizedLinear)")

    def _check_mx_format(self, name, wq, aq, fw, fa):
        """The accepted OCP MX pairs are (weight mxfp8_e4m3, act mxfp8_e4m3), (weight mxfp4_e2m1, act mxfp8_e4m3), the W4A4 pair
        (weight mxfp4_e2m1, act mxfp4_e2m1) and the two with e2m3 activations, W6A6 (weight mxfp6_e2m3fn, act mxfp6_e2m3fn) and W4A6
        (weight mxfp4_e2m1, act mxfp6_e2m3fn), with n_bits 8 / 6 / 4, sym True and weight.group_size absent or 32 (the format's
        block); everything else is refused by layer name."""
        if MXFP6_FORMAT in (fw, fa):
            built = (f"(the built pairs with {MXFP6_FORMAT} are weight {MXFP6_FORMAT} n_bits 6 or weight {MXFP4_FORMAT} n_bits 4 against "
                     f"act {MXFP6_FORMAT} n_bits 6: wanq_gemm_mx6)")
            if fw == MXFP6_FORMAT and fa in (MXFP8_FORMAT, MXFP4_FORMAT, FP8_FORMAT):
                raise NotImplementedError(f"{name}: weight.format: {MXFP6_FORMAT} against act.format: {fa} is not supported: no GEMM takes "
                                          f"e2m3 weights against {'8-bit' if fa != MXFP4_FORMAT else 'e2m1'} activations {built}")
            if fa == MXFP6_FORMAT and fw in (MXFP8_FORMAT, FP8_FORMAT):
                raise NotImplementedError(f"{name}: act.format: {MXFP6_FORMAT} against weight.format: {fw} is not supported: an e4m3 "
                                          f"weight would hold the matrix cores to the fp8 rate {built}")
        if fa == MXFP4_FORMAT:
            built = f"(the built pair is weight {MXFP4_FORMAT} n_bits 4 against act {MXFP4_FORMAT} n_bits 4)"
            if not isinstance(aq["n_bits"], ListConfig) and aq["n_bits"] == 8:
                raise NotImplementedError(f"{name}: act.format: {MXFP4_FORMAT} with act.n_bits: 8 is not supported: no fp4 activation "
                                          f"quantiser path is built yet for 8-bit codes {built}")
            if fw in (MXFP8_FORMAT, FP8_FORMAT):
                raise NotImplementedError(f"{name}: act.format: {MXFP4_FORMAT} against weight.format: {fw} is not supported: no fp4 "
                                          f"activation quantiser path is built yet for an e4m3 weight {built}")
        if fw not in MX_FORMATS or fa not in MX_FORMATS:
            sec, other = ("weight", fw) if fw not in MX_FORMATS else ("act", fa)
            raise NotImplementedError(f"{name}: an MX format on one side needs an MX format on the other ({sec}.format is "
                                      f"{other!r}): the MX GEMMs take block-scaled codes on both sides, weight {MXFP8_FORMAT} or "
                                      f"{MXFP4_FORMAT} against act {MXFP8_FORMAT}, or weight {MXFP4_FORMAT} against act {MXFP4_FORMAT}, or weight "
                                      f"{MXFP6_FORMAT} or {MXFP4_FORMAT} against act {MXFP6_FORMAT}")
        self._check_format_sections(name, (("weight", wq, fw), ("act", aq, fa)))
        g = wq.get("group_size", None)
        if g is not None and (isinstance(g, bool) or g != MX_BLOCK):
            raise NotImplementedError(f"{name}: weight.format: {fw} with weight.group_size={g!r} is not supported: an MX block is "
                                      f"{MX_BLOCK} input channels (leave the key out, or say {MX_BLOCK})")
        self._refuse_format_on_a_transformed_layer(name)
        if self.in_features % MX_BLOCK:
            raise ValueError(f"{name}: weight.format: {fw} needs in_features={self.in_features} to be a multiple of {MX_BLOCK}")

    def _checked_mx_section(self, quant_config, module_name):
        """`mx.block_hadamard` of the config (False without the section): both sides of the layer are quantised behind a 32-point
        Hadamard rotation of every MX block (MxQuantizer).  Accepted only with the W4A4 pair, weight mxfp4_e2m1 against act
        mxfp4_e2m1; with any other pair, or without a format, it is refused by layer name.  Unknown keys of the section are refused."""
        sec = quant_config.get("mx", None)
        if sec is None:
            return False
        name = module_name or type(self).__name__
        unknown = [k for k in sec.keys() if k != "block_hadamard"]
        if unknown:
            raise ValueError(f"{name}: mx.{unknown[0]} is not a known key of the `mx:` section (it has one: block_hadamard)")
        on = sec.get("block_hadamard", False)
        if not isinstance(on, bool):
            raise ValueError(f"{name}: mx.block_hadamard={on!r} must be True or False")
        if on and MXFP6_FORMAT in (self.mx, self.mx_act):
            raise NotImplementedError(f"{name}: mx.block_hadamard: True is not supported with weight.format {self.mx!r} against "
                                      f"act.format {self.mx_act!r}: no rotating e2m3 quantiser is built; the block rotation is built for "
                                      f"the W4A4 pair only (weight.format: {MXFP4_FORMAT} against act.format: {MXFP4_FORMAT})")
        if on and not (self.mx == MXFP4_FORMAT and self.mx_act == MXFP4_FORMAT):
            pair = f"weight.format {self.mx!r} against act.format {self.mx_act!r}" if self.mx else "no MX format"
            raise NotImplementedError(f"{name}: mx.block_hadamard: True is not supported with {pair}: the block rotation is built for "
                                      f"the W4A4 pair only (weight.format: {MXFP4_FORMAT} against act.format: {MXFP4_FORMAT})")
        return on

    def _checked_low_rank(self, quant_config, module_name):
        """`weight.low_rank` of the config (None: no low-rank branch), or the refusal of what has none, before any weight is
        quantised: the message names the layer and the key.  The branch lives in the weight-only GEMM alone: a plain QuantizedLinear
        with an integer StaticQuantizer (per channel or `group_size`) and no `act:` section."""
        wq = quant_config.get("weight", None)
        r = None if wq is None else wq.get("low_rank", None)
        if r is None:
            return None
        name = module_name or type(self).__name__
        if isinstance(r, bool) or not isinstance(r, int) or r <= 0:
            raise ValueError(f"{name}: weight.low_rank={r!r} must be a positive integer")
        if quant_config.get("act", None) is not None:
            raise NotImplementedError(f"{name}: weight.low_rank with an `act:` section is not supported: the low-rank branch is summed "
                                      "in the weight-only GEMM (16-bit activations); the int8, fp8 and MX GEMMs have none")
        if wq.get("format", None) is not None:
            raise NotImplementedError(f"{name}: weight.low_rank with weight.format={wq.get('format')!r} is not supported: the low-rank "
                                      "branch goes with integer weight codes (StaticQuantizer)")
        if isinstance(wq["n_bits"], ListConfig):
            raise NotImplementedError(f"{name}: weight.low_rank with a bit-width list (MixedPrecisionStaticQuantizer) is not supported")
        if self.uses_mask or self.uses_rotation:
            raise NotImplementedError(f"{name}: weight.low_rank with {type(self).__name__} is not supported: the SmoothQuant / QuaRot "
                                      "/ ViDiT layer classes condition an activation quantiser (leave the layer to the plain "
                                      "QuantizedLinear)")
        if r > min(self.in_features, self.out_features):
            raise ValueError(f"{name}: weight.low_rank={r} exceeds min(out_features, in_features)="
                             f"{min(self.in_features, self.out_features)}")
        if padded_rank(r) > RANK_MAX:
            raise ValueError(f"{name}: weight.low_rank={r} makes a padded rank of {padded_rank(r)}, above the GEMM's {RANK_MAX}")
        return r

    def _checked_gptq(self, quant_config, module_name):
        """The config's `gptq:` section when its layer_name_regex matches this layer (None otherwise), or the refusal of what GPTQ has
        no form for, before any weight is quantised: the message names the layer and the key.  GPTQ chooses integer codes on a
        StaticQuantizer's grid for a plain QuantizedLinear."""
        sec = gptq_section(quant_config, module_name)
        if sec is None:
            return None
        name = module_name or type(self).__name__
        wq = quant_config.get("weight", None)
        if wq is None:
            raise NotImplementedError(f"{name}: gptq needs a `weight:` section: it chooses the weight's integer codes")
        if self.uses_mask or self.uses_rotation:
            raise NotImplementedError(f"{name}: gptq with {type(self).__name__} is not supported: the SmoothQuant / QuaRot / ViDiT "
                                      "layer classes re-derive their weight after a transform (leave the layer to the plain "
                                      "QuantizedLinear)")
        if wq.get("format", None) is not None:
            raise NotImplementedError(f"{name}: gptq with weight.format={wq.get('format')!r} is not supported: GPTQ chooses integer "
                                      "codes on a StaticQuantizer's grid")
        if isinstance(wq["n_bits"], ListConfig):
            raise NotImplementedError(f"{name}: gptq with a bit-width list (MixedPrecisionStaticQuantizer) is not supported")
        damp, block = sec.get("damp", 0.01), sec.get("block", BLOCK_MAX)
        if isinstance(damp, bool) or not isinstance(damp, (int, float)) or damp < 0:
            raise ValueError(f"{name}: gptq.damp={damp!r} must be a non-negative number")
        if isinstance(block, bool) or not isinstance(block, int) or not 1 <= block <= BLOCK_MAX:
            raise ValueError(f"{name}: gptq.block={block!r} must be an integer in 1..{BLOCK_MAX}")
        act_order = sec.get("act_order", False)
        if not isinstance(act_order, bool):
            raise ValueError(f"{name}: gptq.act_order={act_order!r} must be True or False")
        # (act_order solves on wanq_gptq_block_gidx, which keeps a grid per column: no pair of columns has to share a group)
        if not act_order and self.group_size is not None and (self.group_size % 2 or block % 2):
            raise ValueError(f"{name}: gptq with weight.group_size={self.group_size} needs an even group size and an even gptq.block")
        return sec

    def _refuse_adapter(self):
        if self.w_quantizer is None or self.a_quantizer is not None or self.fp8 or self.mx or self.uses_mask or self.uses_rotation \
                or not isinstance(self.w_quantizer, StaticQuantizer):
            raise NotImplementedError(f"{self._lr_name()}: set_low_rank needs a plain weight-only QuantizedLinear with integer codes "
                                      "(a `weight:` section, no `act:` section, no format): the low-rank branch is summed in the "
                                      "weight-only GEMM")

    def _checked_group_size(self, quant_config, module_name, device=None):
        """`weight.group_size` of the config (None: one scale per output channel), or the refusal of what has no group-wise form,
        before any weight is quantised: the message names the layer and the key.  `device`: where the layer's weight lives.  With an
        `act:` section the layer runs on wanq_gemm_w8a8_grouped, which exists on the GPU only: a weight in host memory is refused
        here, by name, instead of by the first kernel that meets it."""
        wq = quant_config.get("weight", None)
        g = None if wq is None else wq.get("group_size", None)
        if g is None:
            return None
        name = module_name or type(self).__name__
        if isinstance(g, bool) or not isinstance(g, int) or g <= 0:
            raise ValueError(f"{name}: weight.group_size={g!r} must be a positive integer")
        if isinstance(wq["n_bits"], ListConfig):
            raise NotImplementedError(f"{name}: weight.group_size with a bit-width list (MixedPrecisionStaticQuantizer) is not supported")
        if quant_config.get("act", None) is not None and device is not None and torch.device(device).type == "cpu":
            raise NotImplementedError(f"{name}: weight.group_size together with an `act:` section needs the layer's weight on the GPU "
                                      f"(it is on {device}): only wanq_gemm_w8a8_grouped applies per-group scales to int8 activations "
                                      "and it has no host form; every other int8 GEMM applies one weight scale per output channel")
        if self.uses_mask or self.uses_rotation:
            raise NotImplementedError(f"{name}: weight.group_size with {type(self).__name__} is not supported: the SmoothQuant / "
                                      "QuaRot / ViDiT layer classes quantise one scale per output channel")
        if self.in_features % g:
            raise ValueError(f"{name}: weight.group_size={g} does not divide in_features={self.in_features}")
        return g

    # ---- weight side --------------------------------------------------------------------------------
    def _requantize(self, w, precomputed=None):
        """weight.data <- fake-quant(w) and int_weight <- its integer codes, with the quantizer's current state; `precomputed`: a
        (codes, dequantised weight) pair chosen elsewhere on the quantiser's grid (GPTQ), taken instead of round-to-nearest.  With
        `weight.low_rank: r` the LoRC factors are fitted here too, wherever the codes are (re)derived: the best rank-r approximation
        of E = w - W_hat (low_rank.fit_low_rank: float64 SVD on the weight's device where this build has one, else on the host), kept
        as the fp32 buffers lr_a [Rp, K] / lr_b [N, Rp].  weight.data stays W_hat, without the branch."""
        codes, deq = precomputed if precomputed is not None else self.w_quantizer.codes_and_dequant(w.detach().float())
        self.weight.data = deq
        self.int_weight = codes
        if self.low_rank is not None:
            a, b = fit_low_rank(w.detach().double() - deq.double(), self.low_rank)
            self.register_buffer("lr_a", a, persistent=False)  # (as `_codes`: saved by quantize_and_save_weight)
            self.register_buffer("lr_b", b, persistent=False)
            self._lr16 = None

    def requantize_gptq_(self, H):
        """Choose the layer's codes by GPTQ (qdiff/base/gptq.py) on its calibration Hessian H = X^T X (fp32 [K, K], from
        get_calib_data_wanx.py --hessian).  Scales and zero points are derived from the original weight exactly as round-to-nearest
        derives them (init_quant_params), so they are bit-equal to the round-to-nearest layer's; the codes and weight.data change,
        and a `weight.low_rank` branch is fitted again, on GPTQ's residual.  In place; -> self."""
        name = self.module_name or type(self).__name__
        if self.gptq is None:
            raise NotImplementedError(f"{name}: requantize_gptq_ needs a `gptq:` section whose layer_name_regex names the layer")
        w = self.fp_module.weight.data.detach().float()
        if tuple(H.shape) != (self.in_features, self.in_features):
            raise ValueError(f"{name}: the Hessian is {tuple(H.shape)}, expected {(self.in_features, self.in_features)}")
        self.w_quantizer.init_quant_params(w)
        self.w_quantizer.init_done = True
        damp, block = float(self.gptq.get("damp", 0.01)), int(self.gptq.get("block", BLOCK_MAX))
        if self.gptq.get("act_order", False):  # channels in order of descending diag H; codes and deq come back in the original order
            U, w0, perm = gptq_prepare(H, w, damp, act_order=True)
            codes, deq = gptq_solve(w0, U, self.w_quantizer, block, act_order=True, perm=perm)
        else:
            U, w0 = gptq_prepare(H, w, damp)
            codes, deq = gptq_solve(w0, U, self.w_quantizer, block)
        self._requantize(w, (codes, deq))
        return self

    def set_codes_(self, codes):
        """Take integer codes chosen elsewhere on this layer's grid (a GPTQ checkpoint's `<name>.weight`: int8 [N, K], or the packed
        nibbles of a 4-bit layer) instead of round-to-nearest ones: int_weight <- codes, weight.data <- (codes + zero_point) * delta."""
        name = self.module_name or type(self).__name__
        wq, N, K = self.w_quantizer, self.out_features, self.in_features
        codes = codes.to(self.fp_module.weight.device)
        if codes.dtype == torch.uint8:
            codes = qgemm.unpack_w4(codes.contiguous(), bias=8)
        if codes.dtype != torch.int8 or tuple(codes.shape) != (N, K):
            raise ValueError(f"{name}: codes are {tuple(codes.shape)} {codes.dtype}, expected {(N, K)} int8 (or packed nibbles)")
        G = wq.delta.numel() // N
        deq = ((codes.float().view(N, G, -1) + wq.zero_point.float().view(N, G, 1)) * wq.delta.float().view(N, G, 1)).view(N, K)
        self._requantize(self.fp_module.weight.data, (codes, deq))
        return self

    @property
    def packed_w4(self):
        return self.w_quantizer is not None and self.w_quantizer.n_bits == 4 and self.in_features % 32 == 0 and not self.mx

    @property
    def int_weight(self):
        """int8 codes [N, K].  4-bit layers keep them PACKED in HBM (two per byte, qgemm.pack_w4 layout); this view unpacks."""
        c = self._codes
        if c is not None and c.dtype == torch.uint8 and not self.fp8 and not self.mx:  # (fp8 / MX layers: e4m3 bytes, e2m1 nibbles)
            return qgemm.unpack_w4(c, bias=8)
        return c

    @int_weight.setter
    def int_weight(self, codes):
        if codes is not None and self.packed_w4:
            self._codes = qgemm.pack_w4(codes.contiguous(), bias=8)
        else:
            self._codes = codes
        self._zp_gemm = self._wq16_vecs = None

    def refresh(self):
        """Re-derive the quantized weight after the quantizer changed (bitwidth_refactor, load): the SAME derivation the
        layer's PTQ step uses -- scale / rotate / double quantisation for the SmoothQuant / QuaRot / ViDiT variants once
        their mask / rotation exist (as load_quant_param_dict_ dispatches) -- so that the integer codes always match the
        transform forward() applies to the activations."""
        if self.w_quantizer is None:
            return
        if self.uses_mask and self.uses_rotation and self.channel_mask is not None and self.rotation_signs is not None:
            self.update_quantized_weight_rotated_and_scaled()
        elif self.uses_rotation and not self.uses_mask and self.rotation_signs is not None:
            self.update_quantized_weight_rotated()
        elif self.uses_mask and not self.uses_rotation and self.channel_mask is not None:
            self.update_quantized_weight_scaled()
        elif (self.uses_mask and self.channel_mask is not None) or (self.uses_rotation and self.rotation_signs is not None):
            raise NotImplementedError(f"{type(self).__name__}: transform is only partly initialised (mask / rotation)")
        else:
            self.w_quantizer.init_done = True
            self._requantize(self.fp_module.weight.data.float())

    # ---- activation side ----------------------------------------------------------------------------
    def _act_transform(self):
        """(premul fp32 [C] or None, (had_k, hadk) or None) for the fused quantiser; cached."""
        if self._premul is None and (self.channel_mask is not None or self.rotation_signs is not None):
            dev = self.fp_module.weight.device
            pm = torch.ones(self.in_features, device=dev)
            if self.uses_mask and self.channel_mask is not None:
                pm = pm * self.channel_mask.float().to(dev)
            if self.uses_rotation and self.rotation_signs is not None:
                pm = pm * self.rotation_signs.float().to(dev)
                rot = quarot_utils.kernel_rotation_params(self.in_features, dev)
                if rot is None:
                    raise NotImplementedError(f"no fused rotation for in_features={self.in_features}")
                self._rot = rot
            self._premul = pm.contiguous()
        return self._premul, self._rot

    @property
    def kind(self):
        """What this layer is now, the one place that says so: "fp" (quantisation off, or no `weight:` section: the FP module),
        "weight_only" (no `act:` section), else by its format "fp8", "mx", "int8_grouped" (a `weight.group_size`) or "int8".  `forward`
        dispatches on it and kernel mode maps it to a layer class (wan/quant_wanx_hip.py::_to_hip_linear).  A SmoothQuant / QuaRot /
        ViDiT layer without an `act:` section is "weight_only" too: `forward` runs its FP module, kernel mode refuses it by name."""
        if not self.quant_mode or self.w_quantizer is None:
            return "fp"
        if self.a_quantizer is None:
            return "weight_only"
        return "fp8" if self.fp8 else "mx" if self.mx else "int8_grouped" if self.group_size is not None else "int8"

    def forward(self, x, *args, **kwargs):
        """x: [B, N_token, C] (or [tokens, C]) on the GPU."""
        kind = self.kind
        if kind == "fp" or (kind == "weight_only" and (self.uses_mask or self.uses_rotation)):
            return self.fp_module(x, *args, **kwargs)
        if kind == "weight_only":
            return self._forward_weight_only(x)
        out_dtype = x.dtype if x.dtype in (torch.float16, torch.bfloat16, torch.float32) else torch.float32
        bias = None if self.bias is None else self.bias.detach().float().contiguous()
        y = self._FORWARDS[kind](self, x.reshape(-1, x.shape[-1]), out_dtype, bias)
        return y.view(*x.shape[:-1], self.out_features)

    def _forward_int8(self, x2, out_dtype, bias):
        premul, rot = self._act_transform()
        q, scale, ssum = self.a_quantizer.quantize_int8(x2, premul, rot)
        wq = self.w_quantizer
        zp = None if wq.sym else wq.zero_point.reshape(-1).float().contiguous()
        w4 = self._codes.dtype == torch.uint8
        if w4:  # nibbles are stored as code + 8: fold the 8 into the zero point of the epilogue
            if self._zp_gemm is None:
                self._zp_gemm = ((zp if zp is not None else torch.zeros_like(wq.delta.reshape(-1).float())) - 8.0).contiguous()
            zp = self._zp_gemm
        y = qgemm.w8a8_linear(q, self._codes, scale, wq.delta.reshape(-1).float().contiguous(), bias,
                              ssum if zp is not None else None, zp, out_dtype=out_dtype, w4=w4)
        return self._add_act_zero_point_term(y, scale)

    def _add_act_zero_point_term(self, y, scale):
        """asymmetric activations x_dq = (q + zp_a) * s_a: the zero point's share of x_dq . w_dq^T is the rank-one term
        (zp_a s_a)[token] x rowsum(w_dq)[channel], row sums of the dequantised weight, so group-agnostic
        (Q/base/base_quantizer.py:130-162; no Wan configuration uses this branch)"""
        if self.a_quantizer.sym:
            return y
        t_a = (self.a_quantizer.zero_point.reshape(-1).float() * scale).to(y.dtype)
        return torch.addcmul(y, t_a.unsqueeze(1), self.weight.data.float().sum(dim=1).to(y.dtype).unsqueeze(0))

    def _forward_format(self, x2, out_dtype, bias):
        """`format: fp8_e4m3`: the activation is quantised per token to e4m3 (Fp8Quantizer) and multiplied by the layer's e4m3 weight
        codes, one fp32 scale per token and per output channel.  `format: mxfp8_e4m3` activations against `mxfp8_e4m3` / `mxfp4_e2m1`
        weights, `format: mxfp4_e2m1` activations against `mxfp4_e2m1` weights (W4A4, optionally behind `mx.block_hadamard`), or
        `format: mxfp6_e2m3fn` activations against `mxfp6_e2m3fn` / `mxfp4_e2m1` weights (W6A6 / W4A6, qgemm.mx6_linear):
        quantised per block of 32 channels (MxQuantizer), both sides' E8M0 scales applied by the matrix cores.  On the GPU
        these are kernel mode's two entries per format, fused.quant_rows_fp8 + qgemm.fp8_linear and fused.quant_rows_mx +
        qgemm.mx_linear / qgemm.mx4_linear.  In host memory, and for a shape the GEMM refuses, the same numbers through torch: F.linear of the
        dequantised activation and the dequantised weight, in fp32."""
        a_q, a_s = self.a_quantizer.codes_and_scale(x2)
        refusal, gemm, fmt = (qgemm.mx6_linear_refusal, qgemm.mx6_linear, (self.mx,)) if self.mx_act == MXFP6_FORMAT else \
            (qgemm.mx4_linear_refusal, qgemm.mx4_linear, ()) if self.mx_act == MXFP4_FORMAT else \
            (qgemm.mx_linear_refusal, qgemm.mx_linear, (self.mx,)) if self.mx else (qgemm.fp8_linear_refusal, qgemm.fp8_linear, ())
        if x2.is_cuda and refusal(x2.shape[0], self.out_features, self.in_features, *fmt) is None:
            w_s = self.w_quantizer.scale_u8 if self.mx else self.w_quantizer.delta.reshape(-1).float().contiguous()
            return gemm(a_q, self._codes, a_s, w_s, *fmt, bias, out_dtype=out_dtype)
        # (with mx.block_hadamard the decoded activation and weight.data are both in the rotated domain: their product is x w^T's)
        a = mx_decode(a_q, a_s, self.mx_act) if self.mx else fp8_decode(a_q) * a_s.unsqueeze(-1)
        return F.linear(a, self.weight.data.float(), bias).to(out_dtype)

    def _forward_grouped(self, x2, out_dtype, bias):
        """A `weight.group_size` with an `act:` section: the activation is quantised per token as in `_forward_int8` and multiplied on
        the int8 matrix cores by wanq_gemm_w8a8_grouped, on the layer's codes and the [K / g, N] operands of `weight_only_operands`
        (the 4-bit `zp - 8` convention is the same).  What that entry refuses -- a group that is not a multiple of 128, 8-bit
        asymmetric weights -- goes through the reference's own expression, F.linear(a_quantizer(x), W_hat, bias) on the
        dequantised weight."""
        w4 = self._codes.dtype == torch.uint8
        if qgemm.w8a8_grouped_linear_refusal(x2.shape[0], self.out_features, self.in_features, self.group_size, 4 if w4 else 8,
                                             bool(self.w_quantizer.sym)) is not None:
            return F.linear(self.a_quantizer(x2).float(), self.weight.data.float(), bias).to(out_dtype)
        q, scale, _ = self.a_quantizer.quantize_int8(x2, want_sum=False)
        codes, sw, zp, w4 = self.weight_only_operands()
        y = qgemm.w8a8_grouped_linear(q, codes, scale, sw, zp, self.group_size, bias, out_dtype=out_dtype, w4=w4)
        return self._add_act_zero_point_term(y, scale)

    _FORWARDS = {"int8": _forward_int8, "int8_grouped": _forward_grouped, "fp8": _forward_format, "mx": _forward_format}

    def weight_only_operands(self):
        """(codes, scale fp32 [N], zp fp32 [N] or None, w4) of wanq_gemm_wq16 for this layer's quantised weight: int8 codes, or the
        packed nibbles u = code + 8 with the 8 folded into the zero point (the W4A8 convention).  With a `group_size` scale and zp
        are the [K / g, N] operands of wanq_gemm_wq16_grouped and wanq_gemm_w8a8_grouped (the quantiser's [N, K / g], transposed).  The two tensors are made
        once and kept until the codes are set again (`int_weight`)."""
        if self._wq16_vecs is None or self._wq16_vecs[0].device != self._codes.device:
            wq, N = self.w_quantizer, self.out_features
            w4 = self._codes.dtype == torch.uint8
            if self.group_size is not None:
                sw = wq.delta.float().reshape(N, -1).t().contiguous()
                zp = None if wq.sym else wq.zero_point.float().reshape(N, -1).t().contiguous()
            else:
                sw = wq.delta.reshape(-1).float().expand(N).contiguous()
                zp = None if wq.sym else wq.zero_point.reshape(-1).float().expand(N).contiguous()
            if w4:
                zp = ((zp if zp is not None else torch.zeros_like(sw)) - 8.0).contiguous()
            self._wq16_vecs = (sw, zp, w4)
        sw, zp, w4 = self._wq16_vecs
        return self._codes, sw, zp, w4

    def _forward_weight_only(self, x):
        """A `weight:` section without an `act:` section: y = x @ W_hat^T + bias on the unquantised activations
        (ViDiT-Q/quant_utils/qdiff/base/quant_layer.py:68-72 with a_quantizer None).  16-bit activations on the GPU go through
        wanq_gemm_wq16 -- with a `group_size` wanq_gemm_wq16_grouped -- on the integer codes (exact weight operand, scale in fp32);
        anything else, a group size the kernel does not take (not a multiple of 64) included, through the reference's own
        expression, F.linear on the dequantised weight.
        With a low-rank branch (`weight.low_rank` and / or `set_low_rank`; factors A16 [Rp, K], B16 [N, Rp] in the activation dtype):
        on the GPU t = qgemm.fp_linear(x, A16), rounded once to that dtype, then wanq_gemm_wq16_lowrank adds t B16^T inside the
        GEMM; otherwise the host expression F.linear(x, W_hat, bias) + F.linear((x @ A16^T).to(x.dtype), B16)."""
        if self.low_rank is not None or self._adapter is not None:
            return self._forward_low_rank(x)
        if x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and self._codes is not None and self._codes.is_cuda:
            x2 = x.reshape(-1, x.shape[-1])
            if qgemm.wq16_linear_refusal(x2.shape[0], self.out_features, self.in_features, self.group_size) is None:
                codes, sw, zp, w4 = self.weight_only_operands()
                bias = None if self.bias is None else self.bias.detach()
                if self.group_size is not None:
                    y = qgemm.wq16_grouped_linear(x2.contiguous(), codes, sw, zp, self.group_size, bias, w4=w4)
                else:
                    y = qgemm.wq16_linear(x2.contiguous(), codes, sw, zp, bias, w4=w4)
                return y.view(*x.shape[:-1], self.out_features)
        w = self.weight if self.weight.dtype == x.dtype else self.weight.to(x.dtype)
        b = self.bias if self.bias is None or self.bias.dtype == x.dtype else self.bias.to(x.dtype)
        return F.linear(x, w, b)

    def _forward_low_rank(self, x):
        a16, b16 = self.low_rank_operands(x.dtype, x.device)
        if x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and self._codes is not None and self._codes.is_cuda:
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            if qgemm.wq16_lowrank_refusal(x2.shape[0], self.out_features, self.in_features, self.group_size, a16.shape[0]) is None:
                codes, sw, zp, w4 = self.weight_only_operands()
                bias = None if self.bias is None else self.bias.detach()
                t = qgemm.fp_linear(x2, a16)
                y = qgemm.wq16_lowrank_linear(x2, codes, sw, zp, self.group_size, t, b16, bias, w4=w4)
                return y.view(*x.shape[:-1], self.out_features)
        w = self.weight if self.weight.dtype == x.dtype else self.weight.to(x.dtype)
        b = self.bias if self.bias is None or self.bias.dtype == x.dtype else self.bias.to(x.dtype)
        return F.linear(x, w, b) + F.linear((x @ a16.t()).to(x.dtype), b16)

    # ---- PTQ hooks shared by the variants ------------------------------------------------------------
    def get_channel_mask(self, act_mask):
        """w_absmax_in**alpha / act_absmax**(1-alpha) (viditq_quant_layer.py:30-35, sq_quant_layer.py:27-32)."""
        wm = self.fp_module.weight.data.float().abs().amax(dim=0)
        self.channel_mask = (wm.abs() ** self.alpha) / (act_mask.to(wm.device).float().abs() ** (1 - self.alpha))
        assert not torch.isnan(self.channel_mask).any() and not torch.isinf(self.channel_mask).any(), "bad channel mask"
        self._premul = self._rot = None

    def get_rotation_matrix(self, generator=None):
        """Draw the random +-1 diagonal (quarot_utils.random_hadamard_matrix draws it from the global RNG)."""
        self.rotation_signs = quarot_utils.random_hadamard_signs(self.in_features, generator)
        self._premul = self._rot = None

    @property
    def rotation_matrix(self):
        if self.rotation_signs is None:
            return None
        return quarot_utils.random_hadamard_matrix(self.in_features, self.fp_module.weight.device, self.rotation_signs)

    def _rotate_weight(self, w):
        """(w.double() @ R).float() evaluated as hadU(w * signs) in float64 (row i of R = sign_i * hadU(e_i))."""
        s = self.rotation_signs.to(w.device)
        return quarot_utils.matmul_hadU(w.double() * s).float()
