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

from viditq_extension import fused, qgemm

from ..config import ListConfig
from ..quarot import quarot_utils
from .base_quantizer import (CLIP_BLOCK_GROUPS, CLIP_SEARCHES, CLIP_STEPS_MAX, clip_candidates, BLOCK_SCALES, FP8_FORMAT, FP8_GROUP, MX_BLOCK, MX_FORMATS, MXFP4_FORMAT, MXFP6_FORMAT, MXFP8_FORMAT, DynamicQuantizer, Fp8Quantizer,
                             MxQuantizer, StaticQuantizer, _pow2_f64, fp8_decode, fp8_group_expand, mx_decode, mx_decode_mixed, mx_pair, mx_quant_rows_mixed)
from .gptq import BLOCK_MAX, gptq_prepare, gptq_section, gptq_solve
from .low_rank import RANK_MAX, LowRankBranch, fit_low_rank, padded_rank
from .mixed_precision_quantizer import MixedPrecisionDynamicQuantizer, MixedPrecisionStaticQuantizer


# format key -> (its n_bits, its name in "... is one N-bit format")
_FORMAT_BITS = {FP8_FORMAT: (8, "e4m3"), MXFP8_FORMAT: (8, MXFP8_FORMAT), MXFP4_FORMAT: (4, MXFP4_FORMAT), MXFP6_FORMAT: (6, MXFP6_FORMAT)}


def _hadamard32(device):
    """H[i][j] = (-1)^popcount(i & j), float64 [32, 32]: the block rotation of MxQuantizer(had32=True)"""
    i = torch.arange(MX_BLOCK, device=device)
    bits = (i[:, None] & i[None, :])
    pop = sum((bits >> k) & 1 for k in range(5))
    return (1 - 2 * (pop & 1)).double()


class QuantizedLinear(LowRankBranch, nn.Linear):
    uses_mask = False
    uses_rotation = False

    def __init__(self, in_features, out_features, bias, device, quant_config, fp_module, module_name=None):
        super().__init__(in_features, out_features, bias, device)
        self.fp_module, self.q_cfg = fp_module, quant_config
        self.mx_weight_only = self._checked_weight_only(quant_config, module_name)  # `weight.weight_only: True`: the W4A16 MXFP4 form
        self.low_rank = self._checked_low_rank(quant_config, module_name)  # `weight.low_rank`: the LoRC rank (low_rank.py), or None
        self.mx = None  # the weight's MX format name (`format: mxfp8_e4m3` / `mxfp4_e2m1`), set by _checked_format
        self.mx_act = None  # ... and the activation's
        self.mx_n8 = None  # `mx: {outlier_channels: n8}`: the first n8 channels of the order `mx_perm` are kept in MXFP8
        self.register_buffer("mx_perm", None, persistent=False)  # int32 [K], chosen from calibration statistics (select_outlier_perm)
        self.fp8_group = None  # `group_size: 128` in both sections beside `format: fp8_e4m3` (set by _checked_format): the grouped form
        self.fp8 = self._checked_format(quant_config, module_name)
        self.mx_had32 = self._checked_mx_section(quant_config, module_name)  # `mx: {block_hadamard: True}`, W4A4 MX layers only
        # `block_scale: search` of the `weight:` / `act:` section, each side for itself (mxfp4_e2m1 sides only)
        self.mx_search_w, self.mx_search_act = self._checked_block_scale(quant_config, module_name)
        # (an MX layer's `weight.group_size: 32` names the format's own block: there is no integer group-wise path behind it)
        # (... and an fp8 layer's is the grouped fp8 form's, checked with the format: no integer group-wise path either)
        self.group_size = None if self.mx else self.fp8_group if self.fp8 else \
            self._checked_group_size(quant_config, module_name, fp_module.weight.device)
        self.gptq = self._checked_gptq(quant_config, module_name)  # the `gptq:` section when it names this layer (gptq.py), or None
        self.clip = self._checked_clip(quant_config, module_name)  # the `weight.clip` section (StaticQuantizer.search_clip), or None
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

    def _checked_weight_only(self, quant_config, module_name):
        """`weight.weight_only` of the config (False without the key): the opt-in to MXFP4 weights against unquantised 16-bit
        activations, `weight: {format: mxfp4_e2m1, n_bits: 4, sym: True, weight_only: True}` and no `act:` section (W4A16 MXFP4,
        wanq_gemm_wq16_mx).  Without it an MX weight format without an MX `act:` section stays refused as before.  What the form has
        no kernel for is refused here, before any weight is quantised, and the message names the layer: an `act:` section, any other
        weight format, `mx.block_hadamard` (the activation side would need the rotation), `mx.outlier_channels`, `weight.low_rank`,
        and the SmoothQuant / QuaRot / ViDiT layer classes.  `weight.block_scale: search` is offline and weight-side: it goes with it."""
        wq = quant_config.get("weight", None)
        on = False if wq is None else wq.get("weight_only", False)
        name = module_name or type(self).__name__
        if not isinstance(on, bool):
            raise ValueError(f"{name}: weight.weight_only={on!r} must be True or False")
        if not on:
            return False
        why = None
        mx = quant_config.get("mx", None)
        if quant_config.get("act", None) is not None:
            why = "together with an `act:` section is not supported: the form leaves the activations unquantised (drop the section, or drop the key)"
        elif wq.get("format", None) != MXFP4_FORMAT:
            why = (f"with weight.format={wq.get('format', None)!r} is not supported: the key opts in to {MXFP4_FORMAT} weights, whose "
                   "block scale is exact in a 16-bit operand's exponent (integer weight-only configs need no key; an e2m3 or e4m3 value "
                   "times a power of two is not exact in fp16)")
        elif mx is not None and mx.get("block_hadamard", False):
            why = "with mx.block_hadamard is not supported: the activation side would need the rotation, and it is not quantised"
        elif mx is not None and mx.get("outlier_channels", None) is not None:
            why = "with mx.outlier_channels is not supported: the outlier channels are built for the W4A4 pair only"
        elif wq.get("low_rank", None) is not None:
            why = "with weight.low_rank is not supported: wanq_gemm_wq16_mx sums no low-rank branch"
        elif self.uses_mask or self.uses_rotation:
            why = (f"with {type(self).__name__} is not supported: the SmoothQuant / QuaRot / ViDiT layer classes condition an activation "
                   "quantiser (leave the layer to the plain QuantizedLinear)")
        if why is not None:
            raise NotImplementedError(f"{name}: weight.weight_only: True {why}")
        return True

    def _checked_format(self, quant_config, module_name):
        """True when the config's `weight:` and `act:` sections both say `format: fp8_e4m3` (per-token dynamic e4m3 activations against
        per-channel e4m3 weights, wanq_gemm_fp8; with `group_size: 128` in both sections too, one scale per token or channel and per
        128 input channels, wanq_gemm_fp8_grouped: `fp8_group`), False when neither has the key; every other combination is refused
        here, before any weight is quantised, and the message names the layer and the key."""
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
        if self.mx_weight_only:  # (no `act:` section and fw mxfp4_e2m1: _checked_weight_only) the weight side's rules alone
            self._check_format_sections(name, (("weight", wq, fw),))
            self._check_mx_layer(name, wq, fw)
            self.mx = fw
            return False
        if fw in MX_FORMATS or fa in MX_FORMATS:
            self._check_mx_format(name, wq, aq, fw, fa)
            self.mx, self.mx_act = fw, fa
            return False
        if fw is None or fa is None:
            raise NotImplementedError(f"{name}: format: {FP8_FORMAT} must be set in both the `weight:` and the `act:` section (it is "
                                      f"missing from `{'weight' if fw is None else 'act'}:`): the fp8 GEMM takes e4m3 codes on both sides")
        self._check_format_sections(name, (("weight", wq, fw), ("act", aq, fa)))
        gw, ga = wq.get("group_size", None), aq.get("group_size", None)
        built = (f"the fp8 GEMM applies one weight scale per output channel; the built fine-grained form is weight.group_size: "
                 f"{FP8_GROUP} together with act.group_size: {FP8_GROUP} (wanq_gemm_fp8_grouped)")
        is_group = lambda g: not isinstance(g, bool) and g == FP8_GROUP  # noqa: E731
        if gw is not None and not (is_group(gw) and is_group(ga)):
            raise NotImplementedError(f"{name}: weight.format with weight.group_size={gw!r} and act.group_size={ga!r} is not supported: "
                                      f"{built}")
        if ga is not None and gw is None:
            raise NotImplementedError(f"{name}: act.format with act.group_size={ga!r} and no weight.group_size is not supported: {built}")
        self._refuse_format_on_a_transformed_layer(name)
        self.fp8_group = gw
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
        """The accepted OCP MX pairs are the rows of base_quantizer.MX_PAIRS, with n_bits 8 / 6 / 4, sym True and weight.group_size
        absent or 32 (the format's block); everything else is refused by layer name."""
        a4_as_8 = fa == MXFP4_FORMAT and not isinstance(aq["n_bits"], ListConfig) and aq["n_bits"] == 8
        if mx_pair(fw, fa) is None or a4_as_8:
            raise NotImplementedError(f"{name}: {self._mx_pair_refusal(a4_as_8, fw, fa)}")
        self._check_format_sections(name, (("weight", wq, fw), ("act", aq, fa)))
        self._check_mx_layer(name, wq, fw)

    def _check_mx_layer(self, name, wq, fw):
        """What an MX weight format asks of its layer beyond the sections' own rules, with or without an `act:` section."""
        g = wq.get("group_size", None)
        if g is not None and (isinstance(g, bool) or g != MX_BLOCK):
            raise NotImplementedError(f"{name}: weight.format: {fw} with weight.group_size={g!r} is not supported: an MX block is "
                                      f"{MX_BLOCK} input channels (leave the key out, or say {MX_BLOCK})")
        self._refuse_format_on_a_transformed_layer(name)
        if self.in_features % MX_BLOCK:
            raise ValueError(f"{name}: weight.format: {fw} needs in_features={self.in_features} to be a multiple of {MX_BLOCK}")

    @staticmethod
    def _mx_pair_refusal(a4_as_8, fw, fa):
        """The words for a (weight format, act format) that is no row of MX_PAIRS, or for e2m1 activations declared 8 bits wide: what
        the nearest built pair lacks."""
        if MXFP6_FORMAT in (fw, fa):
            built = (f"(the built pairs with {MXFP6_FORMAT} are weight {MXFP6_FORMAT} n_bits 6 or weight {MXFP4_FORMAT} n_bits 4 against "
                     f"act {MXFP6_FORMAT} n_bits 6: wanq_gemm_mx6)")
            if fw == MXFP6_FORMAT and fa in (MXFP8_FORMAT, MXFP4_FORMAT, FP8_FORMAT):
                return (f"weight.format: {MXFP6_FORMAT} against act.format: {fa} is not supported: no GEMM takes e2m3 weights against "
                        f"{'8-bit' if fa != MXFP4_FORMAT else 'e2m1'} activations {built}")
            if fa == MXFP6_FORMAT and fw in (MXFP8_FORMAT, FP8_FORMAT):
                return (f"act.format: {MXFP6_FORMAT} against weight.format: {fw} is not supported: an e4m3 weight would hold the matrix "
                        f"cores to the fp8 rate {built}")
        if fa == MXFP4_FORMAT:
            built = f"(the built pair is weight {MXFP4_FORMAT} n_bits 4 against act {MXFP4_FORMAT} n_bits 4)"
            if a4_as_8:
                return (f"act.format: {MXFP4_FORMAT} with act.n_bits: 8 is not supported: no fp4 activation quantiser path is built yet "
                        f"for 8-bit codes {built}")
            if fw in (MXFP8_FORMAT, FP8_FORMAT):
                return (f"act.format: {MXFP4_FORMAT} against weight.format: {fw} is not supported: no fp4 activation quantiser path is "
                        f"built yet for an e4m3 weight {built}")
        sec, other = ("weight", fw) if fw not in MX_FORMATS else ("act", fa)
        return (f"an MX format on one side needs an MX format on the other ({sec}.format is {other!r}): the MX GEMMs take block-scaled "
                f"codes on both sides, weight {MXFP8_FORMAT} or {MXFP4_FORMAT} against act {MXFP8_FORMAT}, or weight {MXFP4_FORMAT} against "
                f"act {MXFP4_FORMAT}, or weight {MXFP6_FORMAT} or {MXFP4_FORMAT} against act {MXFP6_FORMAT}")

    def _checked_mx_section(self, quant_config, module_name):
        """`mx.block_hadamard` of the config (False without the section): both sides of the layer are quantised behind a 32-point
        Hadamard rotation of every MX block (MxQuantizer).  Accepted only with the W4A4 pair, weight mxfp4_e2m1 against act
        mxfp4_e2m1; with any other pair, or without a format, it is refused by layer name.  Unknown keys of the section are refused."""
        sec = quant_config.get("mx", None)
        if sec is None:
            return False
        name = module_name or type(self).__name__
        unknown = [k for k in sec.keys() if k not in ("block_hadamard", "outlier_channels")]
        if unknown:
            raise ValueError(f"{name}: mx.{unknown[0]} is not a known key of the `mx:` section (it has two: block_hadamard, "
                             "outlier_channels)")
        on = sec.get("block_hadamard", False)
        self.mx_n8 = self._checked_outlier_channels(sec, on, name)
        if not isinstance(on, bool):
            raise ValueError(f"{name}: mx.block_hadamard={on!r} must be True or False")
        if on and MXFP6_FORMAT in (self.mx, self.mx_act):
            raise NotImplementedError(f"{name}: mx.block_hadamard: True is not supported with weight.format {self.mx!r} against "
                                      f"act.format {self.mx_act!r}: no rotating e2m3 quantiser is built; the block rotation is built for "
                                      f"the W4A4 pair only (weight.format: {MXFP4_FORMAT} against act.format: {MXFP4_FORMAT})")
        if on and not self._mx_admits("had32"):
            pair = f"weight.format {self.mx!r} against act.format {self.mx_act!r}" if self.mx else "no MX format"
            raise NotImplementedError(f"{name}: mx.block_hadamard: True is not supported with {pair}: the block rotation is built for "
                                      f"the W4A4 pair only (weight.format: {MXFP4_FORMAT} against act.format: {MXFP4_FORMAT})")
        return on

    def _checked_outlier_channels(self, sec, had32, name):
        """`mx.outlier_channels: n8` (None without the key): the n8 input channels with the largest calibration absmax are kept in
        MXFP8 on both sides, the others in MXFP4 (wanq_gemm_mx_mixed).  Accepted only with the W4A4 pair; refused by layer name with
        `mx.block_hadamard`, with `weight.low_rank`, and for an n8 that is not a multiple of 128 in [128, in_features - 128]."""
        n8 = sec.get("outlier_channels", None)
        if n8 is None:
            return None
        if not self._mx_admits("n8"):
            pair = f"weight.format {self.mx!r} against act.format {self.mx_act!r}" if self.mx else "no MX format"
            raise NotImplementedError(f"{name}: mx.outlier_channels is not supported with {pair}: the outlier channels are built for "
                                      f"the W4A4 pair only (weight.format: {MXFP4_FORMAT} against act.format: {MXFP4_FORMAT})")
        if had32 is True:
            raise NotImplementedError(f"{name}: mx.outlier_channels with mx.block_hadamard: True is not supported: the rotation mixes "
                                      "the channels of a block, and the mixed quantiser has no rotating form")
        if self.low_rank is not None:
            raise NotImplementedError(f"{name}: mx.outlier_channels with weight.low_rank is not supported: wanq_gemm_mx_mixed sums no "
                                      "low-rank branch")
        K = self.in_features
        if isinstance(n8, bool) or not isinstance(n8, int) or n8 < 128 or n8 % 128 or K - n8 < 128 or K % 128:
            raise ValueError(f"{name}: mx.outlier_channels={n8!r} must be a multiple of 128 with 128 <= n8 <= in_features - 128 "
                             f"(in_features={K}, a multiple of 128)")
        return n8

    def _checked_block_scale(self, quant_config, module_name):
        """(weight side, act side): whether the section says `block_scale: search` -- each block of 32 takes OCP's scale byte or the
        next one, whichever has the smaller squared error (base_quantizer.mx_quant_rows_host; wanq_quant_rows_mx4_search).  `floor`,
        the default, is OCP's rule.  Accepted where that side's format is mxfp4_e2m1; on the act side not together with
        `weight.low_rank` or `mx.outlier_channels`, whose fused producers quantise by OCP's rule (the weight side is quantised
        offline and goes with both).  Everything else is refused by layer name."""
        name = module_name or type(self).__name__
        on = []
        for sec, fmt in (("weight", self.mx), ("act", self.mx_act)):
            q = quant_config.get(sec, None)
            rule = BLOCK_SCALES[0] if q is None else q.get("block_scale", BLOCK_SCALES[0])
            if rule not in BLOCK_SCALES:
                raise ValueError(f"{name}: {sec}.block_scale={rule!r} must be one of {BLOCK_SCALES}")
            if rule == "search" and fmt != MXFP4_FORMAT:
                raise NotImplementedError(f"{name}: {sec}.block_scale: search is not supported with {sec}.format {fmt!r}: the block-scale "
                                          f"search is built for {MXFP4_FORMAT}, where OCP's rule clips a quarter of the top binade")
            on.append(rule == "search")
        if on[1] and (self.low_rank is not None or self.mx_n8 is not None):
            opt = "weight.low_rank" if self.low_rank is not None else "mx.outlier_channels"
            raise NotImplementedError(f"{name}: act.block_scale: search with {opt} is not supported: that option's fused activation "
                                      "producer quantises by OCP's rule (weight.block_scale: search goes with it)")
        return tuple(on)

    def _checked_low_rank(self, quant_config, module_name):
        """`weight.low_rank` of the config (None: no low-rank branch), or the refusal of what has none, before any weight is
        quantised: the message names the layer and the key.  The branch has two hosts: the weight-only GEMM (a plain QuantizedLinear
        with an integer StaticQuantizer, per channel or `group_size`, and no `act:` section) and the W4A4 MX GEMM (weight.format and
        act.format both mxfp4_e2m1, with or without `mx.block_hadamard`)."""
        wq = quant_config.get("weight", None)
        r = None if wq is None else wq.get("low_rank", None)
        if r is None:
            return None
        name = module_name or type(self).__name__
        if isinstance(r, bool) or not isinstance(r, int) or r <= 0:
            raise ValueError(f"{name}: weight.low_rank={r!r} must be a positive integer")
        aq = quant_config.get("act", None)
        # the W4A4 MX pair carries the branch too (wanq_gemm_mx4_lowrank); every other quantised activation is refused as before
        pair = None if aq is None else mx_pair(wq.get("format", None), aq.get("format", None))
        mx4 = pair is not None and pair.low_rank
        if aq is not None and not mx4:
            raise NotImplementedError(f"{name}: weight.low_rank with an `act:` section is not supported: the low-rank branch is summed "
                                      "in the weight-only GEMM (16-bit activations); the int8, fp8 and MX GEMMs have none")
        if wq.get("format", None) is not None and not mx4:
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

    def _checked_clip(self, quant_config, module_name):
        """The `weight.clip` section, `{search: mse | diag | hessian, steps: 20, max_shrink: 0.5}` (None without the key), or the
        refusal of what the clip search has no form for, before any weight is quantised: the message names the layer and the key.
        The search scales the extremes a plain QuantizedLinear's StaticQuantizer takes its grid from."""
        wq = quant_config.get("weight", None)
        sec = None if wq is None else wq.get("clip", None)
        if sec is None:
            return None
        name = module_name or type(self).__name__
        if self.uses_mask or self.uses_rotation:
            raise NotImplementedError(f"{name}: weight.clip with {type(self).__name__} is not supported: the SmoothQuant / QuaRot / "
                                      "ViDiT layer classes re-derive their weight after a transform (leave the layer to the plain "
                                      "QuantizedLinear)")
        if wq.get("format", None) is not None:
            raise NotImplementedError(f"{name}: weight.clip with weight.format={wq.get('format')!r} is not supported: the clip search "
                                      f"scales an integer grid's extremes ({MXFP4_FORMAT} has weight.block_scale: search)")
        if isinstance(wq["n_bits"], ListConfig):
            raise NotImplementedError(f"{name}: weight.clip with a bit-width list (MixedPrecisionStaticQuantizer) is not supported")
        unknown = [k for k in sec.keys() if k not in ("search", "steps", "max_shrink")]
        if unknown:
            raise ValueError(f"{name}: weight.clip.{unknown[0]} is not a known key of the `clip:` section (it has three: search, steps, "
                             "max_shrink)")
        search, steps, shrink = sec.get("search", None), sec.get("steps", 20), sec.get("max_shrink", 0.5)
        if search not in CLIP_SEARCHES:
            raise ValueError(f"{name}: weight.clip.search={search!r} must be one of {CLIP_SEARCHES}")
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= CLIP_STEPS_MAX:
            raise ValueError(f"{name}: weight.clip.steps={steps!r} must be an integer in 1..{CLIP_STEPS_MAX}")
        if isinstance(shrink, bool) or not isinstance(shrink, (int, float)) or not 0 < shrink <= 1 or clip_candidates(steps, shrink) < 1:
            raise ValueError(f"{name}: weight.clip.max_shrink={shrink!r} must be a number in (0, 1] with floor(max_shrink * steps) >= 1 "
                             f"(steps={steps})")
        if search == "hessian" and self.group_size not in CLIP_BLOCK_GROUPS:
            why = ("a whole-row block is in_features x in_features per row; `search: diag` is the per-channel form"
                   if self.group_size is None else "the block is held in LDS")
            raise NotImplementedError(f"{name}: weight.clip.search: hessian needs weight.group_size in {CLIP_BLOCK_GROUPS} (it is "
                                      f"{self.group_size!r}): {why}")
        return {"search": search, "steps": steps, "max_shrink": shrink}

    def _refuse_adapter(self):
        if self.mx_n8 is not None:
            raise NotImplementedError(f"{self._lr_name()}: set_low_rank with mx.outlier_channels is not supported: wanq_gemm_mx_mixed "
                                      "sums no low-rank branch")
        if self.mx_search_act:
            raise NotImplementedError(f"{self._lr_name()}: set_low_rank with act.block_scale: search is not supported: the fused "
                                      "quantise + project producer quantises by OCP's rule")
        if self._mx_admits("low_rank") and not (self.uses_mask or self.uses_rotation):
            return
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

    def _mx_admits(self, option):
        """Whether this layer's MX pair admits `option` ("had32", "low_rank", "n8": the columns of base_quantizer.MX_PAIRS)."""
        pair = mx_pair(self.mx, self.mx_act)
        return pair is not None and getattr(pair, option)

    # ---- weight side --------------------------------------------------------------------------------
    def _requantize(self, w, precomputed=None):
        """weight.data <- fake-quant(w) and int_weight <- its integer codes, with the quantizer's current state; `precomputed`: a
        (codes, dequantised weight) pair chosen elsewhere on the quantiser's grid (GPTQ), taken instead of round-to-nearest.  With
        `weight.low_rank: r` the LoRC factors are fitted here too, wherever the codes are (re)derived: the best rank-r approximation
        of E = w - W_hat (low_rank.fit_low_rank: float64 SVD on the weight's device where this build has one, else on the host), kept
        as the fp32 buffers lr_a [Rp, K] / lr_b [N, Rp].  weight.data stays W_hat, without the branch."""
        if self.mx_n8 is not None:
            return self._requantize_mixed(w)
        codes, deq = precomputed if precomputed is not None else self.w_quantizer.codes_and_dequant(w.detach().float())
        self.weight.data = deq
        self.int_weight = codes
        if self.low_rank is not None:
            w_hat = deq.double()
            if self.mx and self.w_quantizer.had32:  # deq is (w / 32) H block by block; H H = 32 I, so W_hat = deq H
                w_hat = (w_hat.reshape(-1, MX_BLOCK) @ _hadamard32(w_hat.device)).reshape(deq.shape)
            a, b = fit_low_rank(w.detach().double() - w_hat, self.low_rank)
            self.register_buffer("lr_a", a, persistent=False)  # (as `_codes`: saved by quantize_and_save_weight)
            self.register_buffer("lr_b", b, persistent=False)
            self._lr16 = None

    def _requantize_mixed(self, w):
        """`mx.outlier_channels`: the codes are the mixed quantiser's on w in the order `mx_perm` (wanq_quant_rows_mx_mixed; in host
        memory the host expression on w[:, perm]), weight.data their decode put back into the original channel order.  Before the
        order is chosen (select_outlier_perm) there are no codes and weight.data is the FP weight."""
        if self.mx_perm is None:
            self.weight.data, self.int_weight = w.detach().float(), None
            return
        codes, s = mx_quant_rows_mixed(w.detach().float(), self.mx_perm, self.mx_n8, search=self.mx_search_w)
        deq = torch.empty_like(w, dtype=torch.float32)
        deq[:, self.mx_perm.long()] = mx_decode_mixed(codes, s, self.mx_n8)
        self.weight.data, self.int_weight = deq, codes
        wq = self.w_quantizer
        wq.scale_u8, wq.delta = s, _pow2_f64(s.long() - 127).float()
        wq.zero_point = torch.zeros_like(wq.delta)

    def select_outlier_perm(self, act_mask):
        """The channel order of an `mx.outlier_channels` layer from the calibration absmax of its INPUT (the vector PTQ hands to
        get_channel_mask): the n8 channels with the largest absmax first, ties to the lower index, then the others; both segments in
        ascending original order.  Input statistics only, so every consumer of one activation gets the same order.  The weight is
        quantised again in that order."""
        if self.mx_n8 is None:
            raise NotImplementedError(f"{self.module_name or type(self).__name__}: select_outlier_perm needs mx.outlier_channels")
        a = act_mask.reshape(-1).float()
        if a.numel() != self.in_features:
            raise ValueError(f"{self.module_name or type(self).__name__}: the activation statistics have {a.numel()} channels, expected "
                             f"{self.in_features}")
        order = torch.sort(-a.cpu(), stable=True).indices
        top = torch.zeros(self.in_features, dtype=torch.bool)
        top[order[:self.mx_n8]] = True
        idx = torch.arange(self.in_features)
        self.mx_perm = torch.cat((idx[top], idx[~top])).to(device=self.fp_module.weight.device, dtype=torch.int32)
        self._requantize(self.fp_module.weight.data)

    def _forward_mx_mixed(self, x2, out_dtype, bias):
        """`mx.outlier_channels` in simulation mode: both operands are decoded (the activation from the mixed quantiser's codes, in
        permuted order; the weight is weight.data) and multiplied in fp32.  Kernel mode (HipLinearMx) runs wanq_gemm_mx_mixed."""
        if self.mx_perm is None:
            raise RuntimeError(f"{self.module_name or type(self).__name__}: mx.outlier_channels needs calibration activation statistics "
                               "and none were given (PTQ: get_channel_mask(act_mask) / select_outlier_perm); the outlier channels "
                               "are chosen from the input's absmax, there is no weight-only proxy")
        a_q, a_s = mx_quant_rows_mixed(x2, self.mx_perm, self.mx_n8)
        a = mx_decode_mixed(a_q, a_s, self.mx_n8)
        return F.linear(a, self.weight.data.float()[:, self.mx_perm.long()], bias).to(out_dtype)

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
        if self.clip is None or self.clip["search"] == "mse":
            self.w_quantizer.init_quant_params(w)  # (a `diag` / `hessian` clip layer keeps the grid requantize_clip_ fitted)
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

    def requantize_clip_(self, H):
        """Fit the layer's grid by the `weight.clip` search on its calibration Hessian H = X^T X (fp32 [K, K], from
        get_calib_data_wanx.py --hessian; `search: diag` reads its diagonal, `hessian` its g x g diagonal blocks), then re-derive
        codes and weight.data by round-to-nearest on that grid.  A PTQ step: it runs before requantize_gptq_, which then solves on
        the clipped grid; delta / zero_point travel in the quant-parameter file.  In place; -> self."""
        name = self.module_name or type(self).__name__
        if self.clip is None or self.clip["search"] == "mse":
            raise NotImplementedError(f"{name}: requantize_clip_ needs weight.clip.search: diag or hessian (`mse` needs no Hessian and "
                                      "is part of the quantiser's initialisation)")
        if tuple(H.shape) != (self.in_features, self.in_features):
            raise ValueError(f"{name}: the Hessian is {tuple(H.shape)}, expected {(self.in_features, self.in_features)}")
        w = self.fp_module.weight.data.detach().float()
        self.w_quantizer.search_clip(w, H)
        self.w_quantizer.init_done = True
        self._requantize(w)
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
        "weight_only" (no `act:` section), else by its format "fp8", "fp8_grouped" (fp8 with `group_size: 128` on both sides), "mx", "int8_grouped" (a `weight.group_size`) or "int8".  `forward`
        dispatches on it and kernel mode maps it to a layer class (wan/quant_wanx_hip.py::_to_hip_linear).  A SmoothQuant / QuaRot /
        ViDiT layer without an `act:` section is "weight_only" too: `forward` runs its FP module, kernel mode refuses it by name."""
        if not self.quant_mode or self.w_quantizer is None:
            return "fp"
        if self.a_quantizer is None:  # ("weight_only_mx": `weight.weight_only: True`, MXFP4 codes against 16-bit activations)
            return "weight_only_mx" if self.mx_weight_only else "weight_only"
        if self.fp8:
            return "fp8" if self.fp8_group is None else "fp8_grouped"
        return "mx" if self.mx else "int8_grouped" if self.group_size is not None else "int8"

    def forward(self, x, *args, **kwargs):
        """x: [B, N_token, C] (or [tokens, C]) on the GPU."""
        kind = self.kind
        if kind == "fp" or (kind == "weight_only" and (self.uses_mask or self.uses_rotation)):
            return self.fp_module(x, *args, **kwargs)
        if kind == "weight_only":
            return self._forward_weight_only(x)
        if kind == "weight_only_mx":
            return self._forward_weight_only_mx(x)
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
        if self.fp8_group is not None:
            return self._forward_fp8_grouped(x2, out_dtype, bias)
        if self.mx_n8 is not None:
            return self._forward_mx_mixed(x2, out_dtype, bias)
        if self._mx_admits("low_rank") and (self.low_rank is not None or self._adapter is not None):
            return self._forward_mx4_low_rank(x2, out_dtype, bias)
        a_q, a_s = self.a_quantizer.codes_and_scale(x2)
        pair = mx_pair(self.mx, self.mx_act)   # (None: fp8)
        gemm, fmt = (pair.gemm, (self.mx,) if pair.takes_w_fmt else ()) if pair is not None else ("fp8_linear", ())
        if x2.is_cuda and getattr(qgemm, gemm + "_refusal")(x2.shape[0], self.out_features, self.in_features, *fmt) is None:
            w_s = self.w_quantizer.scale_u8 if self.mx else self.w_quantizer.delta.reshape(-1).float().contiguous()
            return getattr(qgemm, gemm)(a_q, self._codes, a_s, w_s, *fmt, bias, out_dtype=out_dtype)
        # (with mx.block_hadamard the decoded activation and weight.data are both in the rotated domain: their product is x w^T's)
        a = mx_decode(a_q, a_s, self.mx_act) if self.mx else fp8_decode(a_q) * a_s.unsqueeze(-1)
        return F.linear(a, self.weight.data.float(), bias).to(out_dtype)

    def _forward_fp8_grouped(self, x2, out_dtype, bias):
        """`format: fp8_e4m3` with `group_size: 128` on both sides: activation and weight are quantised per row and per group of 128
        input channels (Fp8Quantizer's group form).  On the GPU the two entries of kernel mode, fused.quant_rows_fp8_grouped and
        qgemm.fp8_grouped_linear on the layer's codes and its scales transposed to [G, N]; in host memory, and for a shape the GEMM
        refuses (in_features % 128 != 0: a shorter last group), F.linear of the two decoded operands in fp32."""
        a_q, a_s = self.a_quantizer.codes_and_scale(x2)
        if x2.is_cuda and qgemm.fp8_grouped_linear_refusal(x2.shape[0], self.out_features, self.in_features) is None:
            return qgemm.fp8_grouped_linear(a_q, self._codes, a_s, self.w_quantizer.delta.float().t().contiguous(), self.fp8_group, bias,
                                            out_dtype=out_dtype)
        a = fp8_decode(a_q) * fp8_group_expand(a_s, self.fp8_group, self.in_features)
        return F.linear(a, self.weight.data.float(), bias).to(out_dtype)

    def _forward_mx4_low_rank(self, x2, out_dtype, bias):
        """The W4A4 MX layer with a low-rank branch (`weight.low_rank` and / or `set_low_rank`; factors A16 [Rp, K], B16 [N, Rp] in T =
        the activation's dtype when that is 16 bits wide, else bf16): y = Q(x) W_hat^T + t B16^T + bias with t = round_T(round_T(x)
        A16^T), the row rounded once to T in front of the rotation and the product summed in fp32.  On the GPU one producer,
        fused.quant_rows_mxfp4_project (codes, scale bytes and t in one pass over x), and qgemm.mx4_lowrank_linear; in host memory, and
        for a shape they refuse, the same numbers through torch with the same roundings."""
        T = x2.dtype if x2.dtype in (torch.bfloat16, torch.float16) else torch.bfloat16
        a16, b16 = self.low_rank_operands(T, x2.device)
        if x2.is_cuda and qgemm.mx4_lowrank_refusal(x2.shape[0], self.out_features, self.in_features, a16.shape[0]) is None:
            a_q, a_s, t = fused.quant_rows_mxfp4_project(x2.contiguous(), a16, had32=self.mx_had32)
            return qgemm.mx4_lowrank_linear(a_q, self._codes, a_s, self.w_quantizer.scale_u8, t, b16, bias, out_dtype=out_dtype)
        a_q, a_s = self.a_quantizer.codes_and_scale(x2)
        t = (x2.to(T).float() @ a16.float().t()).to(T)
        y = F.linear(mx_decode(a_q, a_s, self.mx_act), self.weight.data.float()) + t.float() @ b16.float().t()
        return (y if bias is None else y + bias).to(out_dtype)

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

    _FORWARDS = {"int8": _forward_int8, "int8_grouped": _forward_grouped, "fp8": _forward_format, "fp8_grouped": _forward_format,
                 "mx": _forward_format}

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

    def _forward_weight_only_mx(self, x):
        """`weight: {format: mxfp4_e2m1, weight_only: True}` without an `act:` section (W4A16 MXFP4): the weight was quantised by
        MxQuantizer and the activation is left alone, y = F.linear(x, mx_decode(codes, scales), bias) -- `_forward_weight_only`'s
        expression on the decoded MX weight, which `_requantize` keeps in weight.data (fp32; every value is exact in bf16, and in
        fp16 wherever it is a normal fp16 number).  Kernel mode (HipLinearWq16Mx) runs wanq_gemm_wq16_mx on the codes."""
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
        if self.mx_n8 is not None:  # an outlier-channel MX layer takes the same statistics for its channel order
            return self.select_outlier_perm(act_mask)
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
