"""Kernel-mode ("hardware") Wan DiT block on MI355X: every Linear of the block runs as an int8-MFMA GEMM with
its producer (LayerNorm+modulate+quant, attention-output quant, GELU+quant) and consumer (gate*y+residual)
fused around it.

Counterpart of ViDiT-Q/examples/Wan2.1/wan/quant_wanx_cuda.py (WanAttentionBlockWithCudaKernel :112-310,
WanSelfAttentionWithCudaKernel :331-474, WANT2VCrossAttentionWithCudaKernel :477-517, the commented FFN path
:520-564), with these deliberate differences:
  * all ten Linears of a block are quantized (the reference wires q/k/v only: use_kernel=[True,False,False]);
  * the residual stream stays fp32 and per-token scales fp32 (simulation-path semantics; the reference casts
    to fp16);
  * no host padding to 128 rows (ragged tile in-kernel), no per-call clones of the scale buffers, no
    torch.cuda.synchronize() inside the block, everything on the current stream (D8);
  * RMSNorm + RoPE is one fp32 kernel instead of float64 complex math.
"""
import torch
import torch.nn as nn

from qdiff.base.low_rank import LowRankBranch, padded_rank
from viditq_extension import _C, fused, qgemm

from . import ops
from .modules.model import WanModel


def _gelu_gate_residual(y, gelu, gate, residual):
    """The unfused tail of a Linear: tanh-GELU, then residual <- residual + y * gate in place (the fp32 stream), as separate passes."""
    if gelu:
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if residual is not None:
        fused.gate_residual_into_(residual, y, gate.view(1, -1))
        return residual
    return y


class _HipLinear(nn.Module):
    """What the block, the checkpoint loader and --dit_fsdp ask of a kernel-mode Linear of any kind, with the answers of a layer that
    takes the block's 16-bit activations as they are; a subclass overrides what it is.  Called as lin(*lin.operands(src), out_dtype,
    gelu=, gate=, residual=, out=)."""
    quantized = False      # an int8 consumer: the block's int8 producers and their prefetch serve it
    fp8 = False
    mx = None              # HipLinearMx: the weight's MX format name
    weight_only = False
    act_form = "fp"        # what its input is made into: "fp" (16 bits, no quantiser), "int8", "fp8", "mxfp8", "mxfp6", "mxfp4" or "mxfp4_h32"
    act_key = "fp"         # layers with the same key share one copy of their input
    plain_rows = False     # its quantiser takes the source's row without a transform, so it can apply the FFN's GELU itself
    rot = act_quantizer = None
    # (`act_premul` and `zp_weight` are buffers in the kinds that hold one, and a class attribute here would shadow a buffer: the
    # kinds that hold none say None themselves)
    checkpointed = True    # the integer checkpoint holds this layer (quant_wanx.py)
    sharded = ("weight",)  # the tensors --dit_fsdp shards (distributed/fsdp.py)
    fuses_epilogue = True  # GELU and gate + residual run in its GEMM's epilogue

    def refresh_zp_gemm(self):
        """(the checkpoint loader's hook: nothing is derived from the loaded buffers)"""

    def operands(self, src):
        """The leading arguments of forward, made from a source (_LnSrc / _FpSrc) in the form this layer consumes."""
        return (src.fp(),)


class _HipLinearInt(_HipLinear):
    """The buffers HipLinearW8A8 and HipLinearWq16 both hold (described there), and the zero point their GEMMs take."""

    def __init__(self, in_features, out_features, bias, sym, w_bits, group_size=None):
        """group_size (the config's `weight.group_size`): scale_weight / zp_weight / zp_gemm are [K / group_size, N] instead of [N]."""
        super().__init__()
        assert w_bits in (4, 8), "integer storage exists for 8-bit and packed 4-bit weights"
        self.in_features, self.out_features, self.w_bits, self.group_size = in_features, out_features, w_bits, group_size
        vec = (out_features,) if group_size is None else (in_features // group_size, out_features)
        self.register_buffer("weight", torch.empty(out_features, in_features // 2 if w_bits == 4 else in_features,
                                                   dtype=torch.uint8 if w_bits == 4 else torch.int8))
        self.register_buffer("scale_weight", torch.empty(vec, dtype=torch.float32))
        self.register_buffer("zp_weight", None if sym else torch.empty(vec, dtype=torch.float32))
        self.register_buffer("zp_gemm", torch.empty(vec, dtype=torch.float32) if w_bits == 4 else None)
        self.register_buffer("bias", torch.empty(out_features, dtype=torch.float32) if bias else None)

    def refresh_zp_gemm(self):
        """After scale_weight / zp_weight were loaded from a checkpoint."""
        if self.w_bits == 4:
            self.zp_gemm.copy_((self.zp_weight if self.zp_weight is not None else torch.zeros_like(self.scale_weight)) - 8.0)

    @property
    def zp(self):  # the zero point the GEMM takes (None: symmetric 8-bit codes)
        return self.zp_gemm if self.w_bits == 4 else self.zp_weight


class HipLinearW8A8(_HipLinearInt):
    """Integer weight + per-output-channel fp32 (delta, zero_point) + fp32 bias.
    weight_dequant = (code + zero_point) * delta  (StaticQuantizer.forward, qdiff/base/base_quantizer.py:56-59).
    w_bits 8: `weight` int8 [N, K].  w_bits 4: `weight` uint8 [N, K/2], the codes + 8 as nibbles in the library's packed layout
    (include/wanq_hip.h); they stay packed in HBM and are expanded in registers inside the GEMM (wanq_gemm_w4a8), the +8 being
    folded into the zero point the epilogue uses (`zp_gemm` = zero_point - 8).
    Optional ViDiT activation transform: `act_premul` fp32 [K] (= channel_mask * rotation signs) and `rot`
    (had_k, hadk) -- the producer kernel applies hadU(x * premul) before quantising this layer's input.
    `act_quantizer`: None for the activation quantiser the fused producers implement (8-bit symmetric per token, eps 1e-6: every Wan
    configuration and the reference's kernels, fused.cu:330-370); otherwise the layer's own qdiff quantiser object (asymmetric,
    below 8 bits, or the mixed-precision class), and the block takes the UNFUSED path for this layer: fp32 activation -> that
    quantiser's HIP kernels -> int8 GEMM -> the zero point's rank-one term (WanAttentionBlockWithHipKernel._linear_any_act).
    With a `group_size` (the config's `weight.group_size`, a multiple of 128 that divides in_features; W4A8-g128) the three parameter
    buffers are [K / group_size, N] and the product is qgemm.w8a8_grouped_linear (csrc/gemm_i8_grouped.hip): the zero point rides
    in the integer operand, one fp32 fma per group and element applies the scales, and every fused epilogue is the same.  8-bit
    asymmetric weights and a non-default activation quantiser have no group-wise form and are refused, by layer name."""
    quantized = True
    act_form = "int8"

    def __init__(self, in_features, out_features, bias=True, sym=False, w_bits=8, group_size=None, name="linear"):
        if group_size is not None:
            why = qgemm.w8a8_grouped_linear_refusal(1, out_features, in_features, group_size, w_bits, sym)
            if why is not None and w_bits == 8 and not sym:
                raise NotImplementedError(f"{name}: weight.group_size={group_size} with 8-bit asymmetric weights (weight.sym: False) has "
                                          f"no kernel-mode form: {why}; the zero point's correction would need per-group token sums")
            if why is not None:
                raise NotImplementedError(f"{name}: weight.group_size={group_size} has no kernel-mode form: {why} (simulation mode "
                                          "runs any group size)")
        super().__init__(in_features, out_features, bias, sym, w_bits, group_size)
        assert w_bits == 8 or in_features % 32 == 0, "packed 4-bit weights need in_features % 32 == 0"
        self.register_buffer("act_premul", None)

    @staticmethod
    def quant_params(w, n_bits=8, sym=False):
        """delta, zero_point of StaticQuantizer.init_quant_params (base_quantizer.py:70-90)."""
        from qdiff.base.base_quantizer import static_params

        return static_params(w, n_bits, sym)

    def _set_codes(self, codes, delta, zero_point):
        """codes: int8 [N, K] in [-2^(b-1), 2^(b-1)-1]."""
        if self.w_bits == 4:
            self.weight.copy_(qgemm.pack_w4(codes.clamp(-8, 7).contiguous(), bias=8))
            self.zp_gemm.copy_((zero_point if zero_point is not None else torch.zeros_like(delta)) - 8.0)
        else:
            self.weight.copy_(codes)
        self.scale_weight.copy_(delta)
        if self.zp_weight is not None:
            self.zp_weight.copy_(zero_point)

    def w_rowsum(self):
        """sum_k w_dq[n, k] = (sum_k code + K * zero_point) * delta, fp32 [N]: the channel factor of an asymmetric activation
        quantiser's rank-one term (x_dq = (q + zp_a) * s_a).  From the integer codes the layer holds; cached until they change."""
        r = self.__dict__.get("_w_rowsum")
        if r is None:
            codes = qgemm.unpack_w4(self.weight, bias=8) if self.w_bits == 4 else self.weight
            zp = self.zp_weight if self.zp_weight is not None else torch.zeros_like(self.scale_weight)
            r = (codes.sum(dim=1, dtype=torch.float32) + self.in_features * zp) * self.scale_weight
            self.__dict__["_w_rowsum"] = r
        return r

    def refresh_zp_gemm(self):
        self.__dict__.pop("_w_rowsum", None)
        super().refresh_zp_gemm()

    @classmethod
    def from_float(cls, weight, bias=None, n_bits=8, sym=False, delta=None, zero_point=None):
        weight = weight.detach().float().contiguous()
        m = cls(weight.shape[1], weight.shape[0], bias is not None, sym, n_bits).to(weight.device)
        if delta is None:
            delta, zero_point = cls.quant_params(weight, n_bits, sym)
        delta, zero_point = delta.float().contiguous().view(-1), zero_point.float().contiguous().view(-1)
        codes, _ = fused.weight_quant(weight, delta, zero_point, -128, 127)
        m._set_codes(codes, delta, None if sym else zero_point)
        if bias is not None:
            m.bias.copy_(bias.detach().float())
        return m

    @classmethod
    def from_quantized(cls, ql, name="linear"):
        """From a qdiff QuantizedLinear (any variant): same integer codes, same parameters, same transform."""
        wq = ql.w_quantizer
        group = ql.group_size
        aq = ql.a_quantizer
        if group is not None and (not aq.sym or aq.n_bits != 8 or aq._sym_floor != 1e-6):
            raise NotImplementedError(f"{name}: weight.group_size={group} with this `act:` section has no kernel-mode form: the fused "
                                      "producers quantise 8-bit symmetric per token, and the unfused path's weight row sums are "
                                      "per channel")
        m = cls(ql.in_features, ql.out_features, ql.bias is not None, wq.sym, wq.n_bits, group, name).to(ql.fp_module.weight.device)
        if group is not None:  # the [K / g, N] operands the simulation-mode layer hands the same entry
            codes, sw, _, _ = ql.weight_only_operands()
            if tuple(codes.shape) != tuple(m.weight.shape) or codes.dtype != m.weight.dtype:
                raise ValueError(f"{name}: codes {tuple(codes.shape)} {codes.dtype} do not fit {tuple(m.weight.shape)} {m.weight.dtype}")
            m.weight.copy_(codes)
            m.scale_weight.copy_(sw)
            if m.zp_weight is not None:
                m.zp_weight.copy_(wq.zero_point.float().reshape(ql.out_features, -1).t())
            m.refresh_zp_gemm()
        else:
            m._set_codes(ql.int_weight, wq.delta.reshape(-1).float(), None if wq.sym else wq.zero_point.reshape(-1).float())
        if ql.bias is not None:
            m.bias.copy_(ql.bias.detach().float())
        premul, rot = ql._act_transform()
        m.act_premul, m.rot = premul, rot
        if not aq.sym or aq.n_bits != 8 or aq._sym_floor != 1e-6:
            m.__dict__["act_quantizer"] = aq  # (not a submodule: the quantiser belongs to the qdiff layer)
        return m

    @property
    def act_key(self):
        """Layers with the same key can share one quantised copy of their input."""
        return None if self.act_premul is None and self.rot is None else id(self)

    @property
    def plain_rows(self):
        return self.act_key is None

    def operands(self, src):
        return src.int8(self)

    def forward(self, a_q, a_scale, a_sum, out_dtype=torch.bfloat16, gelu=False, gate=None, residual=None, out=None):
        zp = self.zp
        if self.group_size is not None:
            return qgemm.w8a8_grouped_linear(a_q, self.weight, a_scale, self.scale_weight, zp, self.group_size, self.bias,
                                             out_dtype=out_dtype, gelu=gelu, gate=gate, residual=residual, out=out, w4=self.w_bits == 4)
        return qgemm.w8a8_linear(a_q, self.weight, a_scale, self.scale_weight, self.bias, a_sum if zp is not None else None, zp,
                                 out_dtype=out_dtype, gelu=gelu, gate=gate, residual=residual, out=out, w4=self.w_bits == 4)


FP_GEMMS = ("torch", "hip")


class HipLinearFp(_HipLinear):
    """A Linear the quant config leaves FP (remain_fp_regex), as the reference's kernel-mode block keeps nn.Linear for those
    (quant_wanx_cuda.py:360,510).  fp_gemm="torch": the bf16 GEMM through torch (hipBLASLt), GELU and gate + residual as separate
    passes; "hip": qgemm.fp_linear (csrc/gemm_bf16.hip) with both in its epilogue, and rows whose bits do not depend on M."""
    checkpointed = False   # its weight stays in the model's own state dict
    act_premul = zp_weight = None

    def __init__(self, weight, bias, dtype=torch.bfloat16, fp_gemm="torch", name="linear"):
        super().__init__()
        if fp_gemm not in FP_GEMMS:
            raise ValueError(f"fp_gemm={fp_gemm!r}: expected one of {FP_GEMMS}")
        if fp_gemm == "hip":
            why = qgemm.fp_linear_refusal(1, weight.shape[0], weight.shape[1])
            if dtype not in (torch.bfloat16, torch.float16):
                why = f"act_dtype {dtype} is not bf16 or fp16"
            if why is not None:
                raise ValueError(f"{name}: fp_gemm='hip' cannot take this layer ({tuple(weight.shape)}): {why}")
        self.fp_gemm = fp_gemm
        self.register_buffer("weight", weight.detach().to(dtype).contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().to(dtype).contiguous())

    @property
    def fuses_epilogue(self):
        return self.fp_gemm == "hip"

    def forward(self, x, out_dtype=None, gelu=False, gate=None, residual=None, out=None):
        """HipLinearWq16.forward's call.  "hip": fused epilogue; reads `weight` as it is now (--dit_fsdp re-points it at views of the
        gathered buffer).  "torch": the result has x's dtype and the update lands in `residual` (`out_dtype` is the fused form's)."""
        if self.fuses_epilogue:
            return qgemm.fp_linear(x, self.weight, self.bias, out_dtype, gelu=gelu, gate=gate, residual=residual, out=out)
        assert out is None or out is residual, "fp_gemm='torch' writes into `residual` only"
        return _gelu_gate_residual(torch.nn.functional.linear(x, self.weight, self.bias), gelu, gate, residual)


class HipLinearWq16(LowRankBranch, _HipLinearInt):
    """A weight-only quantised Linear (a `weight:` section and no `act:` section: W8A16 / W4A16): HipLinearW8A8's integer codes,
    per-channel fp32 (delta, zero_point) and fp32 bias -- 4-bit codes stay packed, `zp_gemm` = zero_point - 8 -- against the
    block's 16-bit activations, through qgemm.wq16_linear (csrc/gemm_wq16.hip): the codes become MFMA fragments in registers,
    exactly, and delta is applied in the fp32 epilogue.  No activation transform and no activation quantiser.
    With a `group_size` (the config's `weight.group_size`, a multiple of 64 that divides in_features) the three parameter buffers are
    [K / group_size, N] and the product is qgemm.wq16_grouped_linear: one fp32 fma per group and element instead of one in all.
    With a `low_rank` (the config's `weight.low_rank`) the optional buffers `lr_a` [Rp, K] / `lr_b` [N, Rp] hold the LoRC factors
    in the activation dtype (qdiff/base/low_rank.py; Rp = low_rank rounded up to 64, zero padded), `set_low_rank` attaches a user
    adapter behind them, and forward computes t = qgemm.fp_linear(x, A16) and calls qgemm.wq16_lowrank_linear: the branch is added
    inside the GEMM, GELU and gate + residual stay fused.  Under --dit_fsdp `sharded` stays ("weight",): the factors are replicated,
    (N + K) R 2 bytes against the N K / 2 of a 4-bit weight (R = 64 of a 1536 x 1536 layer: a third of it; of 8960 x 1536: a fifth).
    Counterpart of QuantizedLinear.forward with a_quantizer None (ViDiT-Q/quant_utils/qdiff/base/quant_layer.py:68-72)."""
    weight_only = True   # (its input is not quantised: the block's int8 producers and their prefetch skip it)
    act_premul = None

    def __init__(self, in_features, out_features, bias=True, sym=False, w_bits=8, name="linear", group_size=None, low_rank=None,
                 act_dtype=torch.bfloat16):
        self.name = name
        if group_size is not None and (group_size < 64 or group_size % 64):
            raise NotImplementedError(f"{name}: weight.group_size={group_size} has no kernel-mode form: the group-wise weight-only GEMM "
                                      "takes groups that are multiples of 64 input channels (simulation mode runs any group size)")
        why = qgemm.wq16_linear_refusal(1, out_features, in_features, group_size)
        super().__init__(in_features, out_features, bias, sym, w_bits, None if why is not None else group_size)
        if why is not None:
            raise ValueError(f"{name}: the weight-only GEMM cannot take this layer ({out_features}, {in_features}): {why}")
        self.low_rank = low_rank
        rp = padded_rank(low_rank) if low_rank else 0
        self.register_buffer("lr_a", torch.zeros(rp, in_features, dtype=act_dtype) if low_rank else None)
        self.register_buffer("lr_b", torch.zeros(out_features, rp, dtype=act_dtype) if low_rank else None)

    @classmethod
    def from_quantized(cls, ql, name="linear", act_dtype=torch.bfloat16):
        """From a plain qdiff QuantizedLinear without an activation quantiser: same integer codes, same parameters, and the same
        low-rank factors (the LoRC buffers cast once to `act_dtype`, the adapter as attached)."""
        if ql.uses_mask or ql.uses_rotation:
            raise NotImplementedError(
                f"{name}: a {type(ql).__name__} without an `act:` section has no kernel-mode form (its transform exists to "
                "condition the activation quantiser, and the reference's forward calls that quantiser unconditionally); give the "
                "config an `act:` section or leave the layer to the plain QuantizedLinear")
        wq = ql.w_quantizer
        if wq.n_bits not in (4, 8):
            raise NotImplementedError(f"{name}: weight-only kernel mode stores 8-bit and packed 4-bit codes (n_bits={wq.n_bits})")
        m = cls(ql.in_features, ql.out_features, ql.bias is not None, wq.sym, wq.n_bits, name, ql.group_size, ql.low_rank,
                act_dtype).to(ql.fp_module.weight.device)
        if ql.low_rank is not None:
            m.lr_a.copy_(ql.lr_a)
            m.lr_b.copy_(ql.lr_b)
        m._adapter = ql._adapter
        codes, sw, _, _ = ql.weight_only_operands()
        if tuple(codes.shape) != tuple(m.weight.shape) or codes.dtype != m.weight.dtype:
            raise ValueError(f"{name}: codes {tuple(codes.shape)} {codes.dtype} do not fit {tuple(m.weight.shape)} {m.weight.dtype}")
        m.weight.copy_(codes)
        m.scale_weight.copy_(sw)
        if m.zp_weight is not None:
            m.zp_weight.copy_(wq.zero_point.float().reshape(ql.out_features, -1).t() if m.group_size is not None
                              else wq.zero_point.reshape(-1).float().expand(ql.out_features))
        m.refresh_zp_gemm()
        if ql.bias is not None:
            m.bias.copy_(ql.bias.detach().float())
        return m

    def forward(self, x, out_dtype=None, gelu=False, gate=None, residual=None, out=None):
        """Reads `weight` as it is now (--dit_fsdp re-points it at views of the gathered buffer)."""
        if self.low_rank is not None or self._adapter is not None:
            a16, b16 = self.low_rank_operands(x.dtype, x.device)
            return qgemm.wq16_lowrank_linear(x, self.weight, self.scale_weight, self.zp, self.group_size, qgemm.fp_linear(x, a16), b16,
                                             self.bias, out_dtype, gelu=gelu, gate=gate, residual=residual, out=out,
                                             w4=self.w_bits == 4)
        if self.group_size is not None:
            return qgemm.wq16_grouped_linear(x, self.weight, self.scale_weight, self.zp, self.group_size, self.bias, out_dtype,
                                             gelu=gelu, gate=gate, residual=residual, out=out, w4=self.w_bits == 4)
        return qgemm.wq16_linear(x, self.weight, self.scale_weight, self.zp, self.bias, out_dtype, gelu=gelu, gate=gate,
                                 residual=residual, out=out, w4=self.w_bits == 4)


class _HipLinearCodes(_HipLinear):
    """What HipLinearFp8 and HipLinearMx share: uint8 `weight` codes and their `scale_weight` as the format's row quantiser wrote
    them for the simulation-mode layer, an fp32 `bias`, and an input that the same quantiser makes from the source's plain row
    (_LnSrc.rows / _FpSrc.rows, one copy for every consumer of that form).  No zero point, no activation transform; the int8
    producers and their prefetch skip it.  A subclass says what its scales are, where they come from, and calls its GEMM."""
    plain_rows = True
    act_premul = zp_weight = None

    def __init__(self, in_features, out_features, bias, fmt, why, weight_cols, scale_shape, scale_dtype, name):
        super().__init__()
        if why is not None:
            raise NotImplementedError(f"{name}: format: {fmt} has no kernel-mode form for this layer ({out_features}, "
                                      f"{in_features}): {why}")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.empty(out_features, weight_cols, dtype=torch.uint8))
        self.register_buffer("scale_weight", torch.empty(scale_shape, dtype=scale_dtype))
        self.register_buffer("bias", torch.empty(out_features, dtype=torch.float32) if bias else None)

    def _take(self, ql, scale, name):
        """The codes, `scale` and the bias of the qdiff layer `ql`."""
        if tuple(ql._codes.shape) != tuple(self.weight.shape) or ql._codes.dtype != torch.uint8:
            raise ValueError(f"{name}: codes {tuple(ql._codes.shape)} {ql._codes.dtype} do not fit {tuple(self.weight.shape)} uint8")
        self.weight.copy_(ql._codes)
        self.scale_weight.copy_(scale)
        if ql.bias is not None:
            self.bias.copy_(ql.bias.detach().float())
        return self

    def operands(self, src):
        return src.rows(self.act_form)


class HipLinearFp8(_HipLinearCodes):
    """An fp8 W8A8 Linear (`format: fp8_e4m3` in the config's `weight:` and `act:` sections): `weight` uint8 [N, K], OCP e4m3fn codes
    of the weight quantised per output channel by wanq_quant_rows_fp8; `scale_weight` fp32 [N], absmax / 448; `bias` fp32.  Its input
    is the block's activation quantised per token by the same entry (codes + fp32 scale), and the product is qgemm.fp8_linear
    (csrc/gemm_fp8.hip) with GELU and gate + residual in its epilogue."""
    fp8 = True
    act_form = act_key = "fp8"

    def __init__(self, in_features, out_features, bias=True, name="linear"):
        super().__init__(in_features, out_features, bias, "fp8_e4m3", qgemm.fp8_linear_refusal(1, out_features, in_features),
                         in_features, (out_features,), torch.float32, name)

    @classmethod
    def from_quantized(cls, ql, name="linear"):
        """From a plain qdiff QuantizedLinear built with `format: fp8_e4m3`: the same codes and scales."""
        m = cls(ql.in_features, ql.out_features, ql.bias is not None, name).to(ql.fp_module.weight.device)
        return m._take(ql, ql.w_quantizer.delta.reshape(-1).float(), name)

    def forward(self, a_q, a_scale, out_dtype=torch.bfloat16, gelu=False, gate=None, residual=None, out=None):
        """Reads `weight` as it is now (--dit_fsdp re-points it at views of the gathered buffer)."""
        return qgemm.fp8_linear(a_q, self.weight, a_scale, self.scale_weight, self.bias, out_dtype, gelu=gelu, gate=gate,
                                residual=residual, out=out)


class HipLinearMx(_HipLinearCodes):
    """An OCP MX Linear (`format: mxfp8_e4m3` activations against `mxfp8_e4m3` / `mxfp4_e2m1` weights, or with `a_fmt` "mxfp4_e2m1"
    the W4A4 pair): `weight` uint8 [N, K] e4m3 bytes or [N, K / 2] packed e2m1 nibbles, `scale_weight` uint8 [N, K / 32] E8M0 bytes,
    both from wanq_quant_rows_mx; `bias` fp32.  Its input is the block's activation quantised per block of 32 channels by the same
    entry (codes + scale bytes), and the product is qgemm.mx_linear, or qgemm.mx4_linear for e2m1 activations (csrc/gemm_mx.hip),
    with GELU and gate + residual in its epilogue.  `had32` (W4A4 only, the config's `mx.block_hadamard`): the weight codes were
    made behind the block Hadamard rotation and the input is quantised behind it too (activation form "mxfp4_h32"); the layer then
    holds the one-element uint8 buffer `mx_had32`, which travels with its codes in the integer checkpoint.  `a_fmt` "mxfp6_e2m3fn"
    (W6A6 / W4A6): `weight` uint8 [N, 3 K / 4] packed e2m3 codes (w_fmt "mxfp6_e2m3fn", from wanq_quant_rows_mx6) or the packed e2m1
    nibbles, the input quantised to e2m3 (activation form "mxfp6"), the product qgemm.mx6_linear; the layer then holds the uint8
    buffer `mx_fmt` = (w_fmt code, a_fmt code), which records the formats in the integer checkpoint."""
    act_form = act_key = "mxfp8"
    sharded = ("weight", "scale_weight")   # the scale bytes are a thirty-second or a sixteenth of the weight's

    def __init__(self, in_features, out_features, bias=True, w_fmt="mxfp8_e4m3", name="linear", a_fmt="mxfp8_e4m3", had32=False):
        a4, a6, w6 = a_fmt == "mxfp4_e2m1", a_fmt == "mxfp6_e2m3fn", w_fmt == "mxfp6_e2m3fn"
        if a_fmt not in ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3fn") or (a4 and w_fmt != "mxfp4_e2m1") or (had32 and not a4) or \
                (a6 and w_fmt not in ("mxfp6_e2m3fn", "mxfp4_e2m1")) or (w6 and not a6):
            raise NotImplementedError(f"{name}: no MX GEMM takes weight {w_fmt} against act {a_fmt}" + (" behind the block rotation" if had32 else ""))
        why = qgemm.mx6_linear_refusal(1, out_features, in_features, w_fmt) if a6 else \
            qgemm.mx4_linear_refusal(1, out_features, in_features) if a4 else qgemm.mx_linear_refusal(1, out_features, in_features, w_fmt)
        super().__init__(in_features, out_features, bias, w_fmt, why,
                         in_features // 2 if w_fmt == "mxfp4_e2m1" else in_features // 4 * 3 if w6 else in_features,
                         (out_features, in_features // 32), torch.uint8, name)
        self.mx, self.a_fmt, self.had32 = w_fmt, a_fmt, bool(had32)
        if a4:
            self.act_form = self.act_key = "mxfp4_h32" if had32 else "mxfp4"
        if a6:
            self.act_form = self.act_key = "mxfp6"
            self.register_buffer("mx_fmt", torch.tensor([_C.MX6_FMT[w_fmt], _C.MX6_FMT[a_fmt]], dtype=torch.uint8))
        if had32:
            self.register_buffer("mx_had32", torch.ones(1, dtype=torch.uint8))

    @classmethod
    def from_quantized(cls, ql, name="linear"):
        """From a plain qdiff QuantizedLinear built with an MX format: the same codes and scale bytes."""
        m = cls(ql.in_features, ql.out_features, ql.bias is not None, ql.mx, name, ql.mx_act, ql.mx_had32).to(ql.fp_module.weight.device)
        return m._take(ql, ql.w_quantizer.scale_u8, name)

    def forward(self, a_q, a_scale, out_dtype=torch.bfloat16, gelu=False, gate=None, residual=None, out=None):
        """Reads `weight` and `scale_weight` as they are now (--dit_fsdp re-points them at views of the gathered buffer)."""
        if self.a_fmt == "mxfp6_e2m3fn":
            return qgemm.mx6_linear(a_q, self.weight, a_scale, self.scale_weight, self.mx, self.bias, out_dtype, gelu=gelu, gate=gate,
                                    residual=residual, out=out)
        if self.a_fmt == "mxfp4_e2m1":
            return qgemm.mx4_linear(a_q, self.weight, a_scale, self.scale_weight, self.bias, out_dtype, gelu=gelu, gate=gate,
                                    residual=residual, out=out)
        return qgemm.mx_linear(a_q, self.weight, a_scale, self.scale_weight, self.mx, self.bias, out_dtype, gelu=gelu, gate=gate,
                               residual=residual, out=out)


# QuantizedLinear.kind -> the layer class that takes it over ("fp": the layer's FP module, below)
_HIP_LINEAR_OF = {"int8": HipLinearW8A8, "int8_grouped": HipLinearW8A8, "weight_only": HipLinearWq16, "fp8": HipLinearFp8,
                  "mx": HipLinearMx}


def _to_hip_linear(lin, n_bits, sym, act_dtype, fp_gemm="torch", name="linear"):
    from qdiff.base.quant_layer import QuantizedLinear

    if isinstance(lin, QuantizedLinear):
        cls = _HIP_LINEAR_OF.get(lin.kind)
        if cls is HipLinearWq16 and act_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"{name}: the weight-only GEMM takes bf16 or fp16 activations (act_dtype {act_dtype})")
        if cls is HipLinearWq16:
            return cls.from_quantized(lin, name, act_dtype)
        if cls is not None:
            return cls.from_quantized(lin, name)
        lin = lin.fp_module
    if n_bits is None:
        return HipLinearFp(lin.weight.data, lin.bias.data if lin.bias is not None else None, act_dtype, fp_gemm, name)
    return HipLinearW8A8.from_float(lin.weight.data, lin.bias.data if lin.bias is not None else None, n_bits, sym)


# activation form -> the fused row quantiser that makes it, (codes, scales) = f(rows, gelu=); a new form adds its entry here
_ROW_QUANTISERS = {"fp8": "quant_rows_fp8", "mxfp8": "quant_rows_mx", "mxfp4": "quant_rows_mxfp4", "mxfp4_h32": "quant_rows_mxfp4_h32",
                   "mxfp6": "quant_rows_mxfp6"}


class _Src:
    """What _LnSrc and _FpSrc share: the forms a row quantiser without a transform makes, one cached copy per form."""

    def rows(self, form):
        """(codes, scales) of this activation in `form` for every consumer of it (HipLinearFp8: e4m3 codes + fp32 scale;
        HipLinearMx: e4m3, packed e2m3 or packed e2m1 codes + E8M0 scale bytes), quantised from what `_plain_row` hands over."""
        if form not in self.cache:
            x, gelu = self._plain_row()
            self.cache[form] = getattr(fused, _ROW_QUANTISERS[form])(x, gelu=gelu)
        return self.cache[form]


class _LnSrc(_Src):
    """Lazy activation = LayerNorm(x) (* gamma) * (1 + scale) + shift, materialised per consumer format."""

    def __init__(self, blk, x, gamma, shift, scale):
        self.blk, self.x, self.gamma, self.shift, self.scale, self.cache = blk, x, gamma, shift, scale, {}

    def int8(self, lin):
        key = lin.act_key
        if key not in self.cache:
            x, rows, C = self.x, self.x.shape[0], self.x.shape[1]
            q = torch.empty(rows, C, dtype=torch.int8, device=x.device)
            qs = torch.empty(2, rows, dtype=torch.float32, device=x.device)
            if key is None:
                fused.layernorm_nobias_t2i_quant_sum_fuse(q, x, self.gamma, self.shift, self.scale, qs[1], qs[0], self.blk.eps)
            else:
                fused.layernorm_rotate_quant(q, x, self.gamma, self.shift, self.scale, lin.act_premul, lin.rot, qs[1], qs[0], self.blk.eps)
            self.cache[key] = (q, qs[0], qs[1])
        return self.cache[key]

    def _same_rotation(self, a, b):
        """Same Hadamard order and the same K' x K' sign matrix (a fixed function of the order: compared once, cached)."""
        key = (id(a), id(b))
        memo = self.blk.__dict__.setdefault("_rot_memo", {})
        if key not in memo:
            (ka, ha), (kb, hb) = a.rot, b.rot
            memo[key] = ka == kb and ((ha is None and hb is None) or
                                      (ha is not None and hb is not None and ha.shape == hb.shape and bool(torch.equal(ha, hb))))
        return memo[key]

    def prefetch(self, lins):
        """Materialise the int8 form for several quantized consumers in ONE pass over x (q / k / v of a block share
        this LayerNorm but carry their own ViDiT mask and rotation signs).  Falls back to the lazy per-consumer path
        whenever the consumers do not all rotate with the same Hadamard parameters."""
        todo = []
        for lin in lins:
            if not lin.quantized or lin.act_key is None or lin.act_key in self.cache or lin.rot is None or \
                    lin.act_quantizer is not None:
                continue
            if lin.act_key not in [l.act_key for l in todo]:
                todo.append(lin)
        if len(todo) < 2 or not all(self._same_rotation(todo[0], l) for l in todo[1:]):
            return
        todo = todo[:3]
        x, rows, C = self.x, self.x.shape[0], self.x.shape[1]
        qs = [torch.empty(rows, C, dtype=torch.int8, device=x.device) for _ in todo]
        vec = torch.empty(len(todo), 2, rows, dtype=torch.float32, device=x.device)
        fused.layernorm_rotate_quant_multi(qs, x, self.gamma, self.shift, self.scale, [l.act_premul for l in todo], todo[0].rot,
                                           [vec[i, 1] for i in range(len(todo))], [vec[i, 0] for i in range(len(todo))], self.blk.eps)
        for i, lin in enumerate(todo):
            self.cache[lin.act_key] = (qs[i], vec[i, 0], vec[i, 1])

    def _plain_row(self):
        """The fp32 row, what a simulation-mode quantiser sees.  (A fused LayerNorm + modulate + fp8 / MX producer would save the
        fp32 round trip.)"""
        return self.fp32(), False

    def fp(self):
        if "fp" not in self.cache:
            out = torch.empty(self.x.shape, dtype=self.blk.act_dtype, device=self.x.device)
            fused.layernorm_nobias_t2i_fuse(out, self.x, self.gamma, self.shift, self.scale, self.blk.eps)
            self.cache["fp"] = out
        return self.cache["fp"]

    def fp32(self):
        """The normalised, modulated row in fp32 (what a simulation-mode quantiser sees: model.py:327)."""
        if "fp32" not in self.cache:
            out = torch.empty(self.x.shape, dtype=torch.float32, device=self.x.device)
            fused.layernorm_nobias_t2i_fuse(out, self.x, self.gamma, self.shift, self.scale, self.blk.eps)
            self.cache["fp32"] = out
        return self.cache["fp32"]


class _FpSrc(_Src):
    """An activation that already exists in bf16 (attention output, FFN hidden, text context).  `gelu`: the tensor is the FFN's
    PRE-activation and the quantiser applies the tanh-GELU itself (gelu_quant_sum -- the reference's own split,
    K/csrc/fused/fused.cu gelu_quant_sum behind a 16-bit GEMM output, W/models/quant_opensora_cuda.py:402); only offered to a
    consumer that quantises without a rotation."""

    def __init__(self, t, fp_dtype=None, gelu=False):
        self.t, self.cache, self.fp_dtype, self.gelu = t, {}, fp_dtype, gelu
        # `derived`: what consumers computed from this source and may reuse while the source lives (the text context is the same
        # tensor in every denoising step: a block's cross-attention k / v of it are kept here, keyed by the block)
        self.derived = None

    def int8(self, lin):
        key = lin.act_key
        if key not in self.cache:
            qs = torch.empty(2, self.t.shape[0], dtype=torch.float32, device=self.t.device)
            if key is None:
                q = (fused.gelu_quant_sum if self.gelu else fused.quant_sum)(self.t, qs[1], qs[0])
            else:
                q = fused.rotate_quant(self.t, lin.act_premul, lin.rot, qs[1], qs[0])
            self.cache[key] = (q, qs[0], qs[1])
        return self.cache[key]

    def _plain_row(self):
        """The 16-bit tensor; `gelu`: the quantiser applies the tanh-GELU itself (its act = 1), as gelu_quant_sum does for the int8
        consumers."""
        return self.t, self.gelu

    def fp32(self):
        if "fp32" not in self.cache:
            t = self.t.float()
            self.cache["fp32"] = torch.nn.functional.gelu(t, approximate="tanh") if self.gelu else t
        return self.cache["fp32"]

    def fp(self):
        assert not self.gelu, "a pre-activation source has no floating-point view"
        if self.fp_dtype is not None and self.t.dtype != self.fp_dtype:
            if "fp" not in self.cache:
                self.cache["fp"] = self.t.to(self.fp_dtype)
            return self.cache["fp"]
        return self.t


_FORCE_CHUNK_UNIT = None  # tests: pipeline the exchange even when a tiny model's heads do not fill a GPU round


def _head_chunks(heads, seq_len, device, max_chunks=4):
    """Split a rank's `heads` for the pipelined Ulysses exchange.  The attention kernel launches ceil(L/256) workgroups per
    head, one per CU at a time, so a chunk should fill whole rounds of the GPU: with L = 32760 (128 workgroups per head,
    256 CUs) chunks are multiples of 2 heads -- 6 heads -> (2, 2, 2), never (3, 3), which would run 4 half-empty rounds
    instead of 3 full ones.  Small chunks first and last: those are the exchanges nothing hides."""
    per_head = -(-seq_len // 256)
    unit = _FORCE_CHUNK_UNIT or max(1, ops.cu_count(device) // per_head)   # heads per full round of the GPU (>= 1)
    units, rem = divmod(heads, unit)
    n = min(max_chunks - (1 if rem else 0), units)
    if n <= 0:
        return [(0, heads)]
    sizes = [units // n * unit] * n
    for i in range(units % n):               # spare whole units go to the middle chunks
        sizes[(n // 2 + i) % n] += unit
    if rem:
        sizes.append(rem)                    # a last, smaller chunk: its partial round exists either way
    out, a = [], 0
    for sz in sizes:
        out.append((a, a + sz))
        a += sz
    return out if len(out) > 1 else [(0, heads)]


def _late_gelu(ffn0, ffn2):
    """ffn.2's quantiser applies the FFN's GELU (int8: gelu_quant_sum; fp8 / MX: the row quantiser's act = 1) instead of ffn.0's
    epilogue: when it quantises the plain row, and that row is ffn.0's output in the form ffn.0 itself consumes."""
    return ffn2.plain_rows and ffn0.act_form == ffn2.act_form


class _Attn(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.q = self.k = self.v = self.o = None
        self.register_buffer("norm_q_weight", torch.ones(dim))
        self.register_buffer("norm_k_weight", torch.ones(dim))


class WanAttentionBlockWithHipKernel(nn.Module):
    def __init__(self, dim, ffn_dim, num_heads, eps=1e-6, act_dtype=torch.bfloat16, attn_qk8=False, cross_attn_qk8=False,
                 attn_v_bits=None, cross_attn_v_bits=None, attn_map=None, cross_attn_map=None, fp_gemm="torch", attn_smooth_k=False,
                 cross_attn_smooth_k=False):
        super().__init__()
        if fp_gemm not in FP_GEMMS:
            raise ValueError(f"fp_gemm={fp_gemm!r}: expected one of {FP_GEMMS}")
        # which GEMM runs the Linears kept in floating point (HipLinearFp); from_float hands it to each of them
        self.fp_gemm = fp_gemm
        self.dim, self.ffn_dim, self.num_heads, self.head_dim, self.eps = dim, ffn_dim, num_heads, dim // num_heads, eps
        self.act_dtype = act_dtype
        # quant_config.attn.qk / cross_attn.qk (8-bit symmetric): q and k of that attention leave RMSNorm + RoPE as
        # per-(token, head) int8 codes and Q.K^T runs on the int8 matrix cores (Q/base/quant_attn.py:168-174)
        self.attn_qk8, self.cross_attn_qk8 = bool(attn_qk8), bool(cross_attn_qk8)
        # quant_config.attn.qk.smooth_k / cross_attn.qk.smooth_k: k is quantised as k - mean over tokens (SageAttention's K smoothing;
        # exact: a vector shared by all keys shifts every score of a query row alike, and softmax drops it).  q is never centred.
        for key, on, qk8 in (("attn", attn_smooth_k, attn_qk8), ("cross_attn", cross_attn_smooth_k, cross_attn_qk8)):
            if on and not qk8:
                raise ValueError(f"{key}.qk.smooth_k without {key}.qk: K smoothing centres the int8 codes of k and has nothing to act on "
                                 "when q / k stay 16-bit")
        self.attn_smooth_k, self.cross_attn_smooth_k = bool(attn_smooth_k), bool(cross_attn_smooth_k)
        # quant_config.attn.v / cross_attn.v: v fake-quantised per (head, channel) over all tokens before the attention
        # (W/models/quant_opensora.py:438-440); P.V itself stays bf16 -- the reference's recipe has no integer P either
        self.attn_v_bits, self.cross_attn_v_bits = attn_v_bits, cross_attn_v_bits
        self.attn_map, self.cross_attn_map = attn_map, cross_attn_map  # (n_bits, sym) of the attention-map quantiser, or None
        # the source block's self_attn.window_size (from_float): sliding-window self-attention on the plain 16-bit kernel
        self.window_size = (-1, -1)
        self.self_attn, self.cross_attn = _Attn(dim), _Attn(dim)
        self.ffn0 = self.ffn2 = None
        self.register_buffer("modulation", torch.zeros(1, 6, dim))
        self.register_buffer("norm3_weight", torch.ones(dim))
        self.register_buffer("norm3_bias", torch.zeros(dim))
        self.register_buffer("ones_gate", torch.ones(dim))

    @classmethod
    def from_float(cls, blk, n_bits=8, sym=False, act_dtype=torch.bfloat16, attn_qk8=False, cross_attn_qk8=False,
                   attn_v_bits=None, cross_attn_v_bits=None, attn_map=None, cross_attn_map=None, fp_gemm="torch", name="block",
                   attn_smooth_k=False, cross_attn_smooth_k=False):
        """Build from a WanAttentionBlock (wan/modules/model.py) whose Linears are either plain nn.Linear
        (quantized here with plain per-channel W8 when n_bits is given, kept FP when n_bits is None) or qdiff
        QuantizedLinear variants (their codes / parameters / ViDiT transform are taken over as they are).
        fp_gemm: "torch" or "hip", the GEMM of the Linears kept FP (HipLinearFp); a layer "hip" cannot take is refused here, by name."""
        window = tuple(int(w) for w in getattr(blk.self_attn, "window_size", (-1, -1)))
        if ops.window_bounded(window) and (attn_qk8 or attn_map is not None):
            keys = [k for k, on in (("attn.qk", attn_qk8), ("attn.attn_map", attn_map is not None),
                                    ("attn.v", attn_map is not None and attn_v_bits is not None)) if on]
            raise NotImplementedError(
                f"{name}.self_attn: window_size={window} with {' + '.join(keys)} configured: sliding-window attention exists for the "
                "plain 16-bit kernel only (csrc/attention.hip, WIN); the int8 Q.K^T form and the attention-map quantiser have no banded "
                "form, and running them dense would ignore the window.  Drop those keys from the quant config or build the model with "
                "window_size=(-1, -1)")
        m = cls(blk.dim, blk.ffn_dim, blk.num_heads, blk.eps, act_dtype, attn_qk8, cross_attn_qk8, attn_v_bits,
                cross_attn_v_bits, attn_map, cross_attn_map, fp_gemm, attn_smooth_k, cross_attn_smooth_k).to(blk.modulation.device)
        m.window_size = window
        for name_ in ("self_attn", "cross_attn"):
            src, dst = getattr(blk, name_), getattr(m, name_)
            for l in "qkvo":
                setattr(dst, l, _to_hip_linear(getattr(src, l), n_bits, sym, act_dtype, fp_gemm, f"{name}.{name_}.{l}"))
            dst.norm_q_weight.copy_(src.norm_q.weight.data.float())
            dst.norm_k_weight.copy_(src.norm_k.weight.data.float())
        m.ffn0 = _to_hip_linear(blk.ffn[0], n_bits, sym, act_dtype, fp_gemm, f"{name}.ffn.0")
        m.ffn2 = _to_hip_linear(blk.ffn[2], n_bits, sym, act_dtype, fp_gemm, f"{name}.ffn.2")
        m.modulation.copy_(blk.modulation.data.float())
        if isinstance(blk.norm3, nn.LayerNorm) and blk.norm3.weight is not None:
            m.norm3_weight.copy_(blk.norm3.weight.data.float())
            m.norm3_bias.copy_(blk.norm3.bias.data.float())
        return m

    @staticmethod
    def _quant(x):
        qs = torch.empty(2, x.shape[0], dtype=torch.float32, device=x.device)
        q = fused.quant_sum(x, qs[1], qs[0])
        return q, qs[0], qs[1]

    def _linear(self, lin, src, out_dtype=None, gelu=False, gate=None, residual=None):
        """y = lin(src) with the producer / epilogue fusion the layer's kind allows.  With `residual` (the fp32
        stream) the result is residual + y*gate written in place."""
        out_dtype = out_dtype or self.act_dtype
        if lin.act_quantizer is not None:
            return self._linear_any_act(lin, src, out_dtype, gelu, gate, residual)
        a = lin.operands(src)
        if residual is not None:  # (the gate is a contiguous fp32 [C] at every call site: a modulation row, or `ones_gate`)
            return lin(*a, torch.float32, gate=gate, residual=residual, out=residual)
        return lin(*a, out_dtype, gelu=gelu)

    def _linear_any_act(self, lin, src, out_dtype, gelu, gate, residual):
        """A quantised Linear whose activation quantiser is not the fused producers' (asymmetric, below 8 bits, the mixed-precision
        class: Q/base/base_quantizer.py:130-149, mixed_precision_quantizer.py:126-186 -- no Wan configuration, and the reference's
        kernel mode has no such path at all): the layer's own qdiff quantiser on the fp32 activation (its HIP kernels: row statistics
        + quantise, the ViDiT transform written out in fp32 first), the int8 GEMM with its plain fp32 epilogue, the asymmetric zero
        point's rank-one term (zp_a s_a)[token] x rowsum(w_dq)[channel], then GELU / gate + residual unfused."""
        aq = lin.act_quantizer
        q, s, ssum = aq.quantize_int8(src.fp32(), lin.act_premul, lin.rot)
        y = lin(q, s, ssum, torch.float32)
        if not aq.sym:
            y = torch.addcmul(y, (aq.zero_point.reshape(-1).float() * s).unsqueeze(1), lin.w_rowsum().unsqueeze(0))
        y = _gelu_gate_residual(y, gelu, gate, residual)
        return y if residual is not None else y.to(out_dtype)

    @staticmethod
    def _vq(v, n_bits, k_len):
        """attn.v / cross_attn.v of the quant config: v fake-quantised in place, per column over the first k_len rows."""
        if n_bits:
            fused.fake_quant_cols_(v if k_len is None or k_len >= v.shape[0] else v[:k_len], n_bits)
        return v

    def _context_kv(self, ctx):
        """Cross-attention k (after its RMSNorm; Q8Rows under cross_attn.qk) and v (after cross_attn.v's fake-quant) of the text
        context.  Neither depends on the timestep or on the latent (W/wan/modules/model.py:178-200: k = norm_k(k(context)),
        v = v(context)), and the sampling loop hands every step the same context tensor (W/wan/text2video.py:248-269), so a
        source that carries a `derived` dict (QuantWanModel.forward keeps one per live context tensor) gets them computed once
        per block and reused: 2 GEMMs + 1-2 rowwise launches per block and pass leave the step, bit-identical results."""
        memo = ctx.derived
        if memo is not None and id(self) in memo:
            return memo[id(self)]
        ca = self.cross_attn
        k = self._linear(ca.k, ctx)
        v = self._vq(self._linear(ca.v, ctx), self.cross_attn_v_bits, None)
        k = self._prep_qk(k, ca.norm_k_weight, None, self.cross_attn_qk8, True, smooth=self.cross_attn_smooth_k)
        if memo is not None:
            memo[id(self)] = (k, v)
        return k, v

    def _prep_qk(self, x, weight, rope, int8, for_keys, smooth=False, sp=None):
        """q or k behind its projection: RMSNorm + RoPE in place, or -- int8: attn.qk / cross_attn.qk -- the Q8Rows of that row.
        smooth (keys only, qk.smooth_k): the codes are those of k - centre, the centre being k's mean over the tokens -- column sums
        first (a second read of x), under sequence parallelism all-reduced over the group (sp), then the centred quantiser."""
        if int8:
            center = None
            if smooth and for_keys:
                colsum = ops.rmsnorm_rope_colsum(x, weight, rope, self.head_dim, eps=self.eps)
                center = ops.center_of(colsum, x.shape[0]) if sp is None else sp.mean_rows(colsum, x.shape[0])
            return ops.rmsnorm_rope_q8(x, weight, rope, self.head_dim, for_keys, eps=self.eps, center=center)
        return ops.rmsnorm_rope_(x, weight, rope, self.head_dim, eps=self.eps)

    def _attend(self, q, k, v, heads, k_len, q_len, map_cfg, window=(-1, -1)):
        """The one place that picks the attention kernel: the attention-map quantiser (16-bit or Q8Rows q / k alike: with attn.qk
        and attn.v the reference's whole recipe), the int8 Q.K^T kernel for Q8Rows, else the plain 16-bit kernel, banded where
        `window` is bounded.  k_len None (cross-attention: the text context carries no padding): the call names no key length."""
        k_len = () if k_len is None else (k_len,)
        if map_cfg is not None:
            return ops.attention_map_quant(q, k, v, heads, map_cfg[0], map_cfg[1], *k_len, q_len=q_len)
        if isinstance(q, ops.Q8Rows):
            return ops.attention_qk8(q, k, v, heads, *k_len)
        return ops.attention(q, k, v, heads, *k_len, **ops.window_kwargs(window))

    def _self_attention_ulysses(self, q, h, rope, seq_len, sp):
        """Self-attention under Ulysses, pipelined over head chunks (_head_chunks): chunk 0 of q is exchanged under the k GEMM and
        chunk 0 of k under the v GEMM; the exchange of every further chunk, and the way back of the previous one, flies under the
        attention of another chunk, so about half of the all-to-all time of a block hides behind its 2-6 ms of attention.  The
        collectives run in issue order on the group's own stream.  Only the wire format of q and k varies:
          * 16 bits: RMSNorm + RoPE writes q and k straight into the send images of the chunks ([P, Lp, w] each): no pack pass;
          * int8 (attn.qk): the q / k quantiser works on (token, head) rows (Q/base/quant_attn.py:168-174 on the reshape of
            W/models/quant_opensora.py:431-436), and a rank holds whole (token, head) rows on BOTH sides of the head exchange -- so
            the rows are quantised where RMSNorm + RoPE produces them (same kernel, same codes as on one GPU) and the all-to-all
            moves the int8 codes and the two fp32 scale planes: half the xGMI bytes of the 16-bit exchange, bit-equal to the
            single-rank result."""
        sa, d = self.self_attn, self.head_dim
        lp, C = q.shape
        chunks = [(a * d, b * d) for a, b in _head_chunks(C // d // sp.size, lp * sp.size, q.device)]
        if self.attn_qk8:
            def pack(x, weight, for_keys):
                # (smooth_k: a rank holds a token shard of k, so the column sums are all-reduced before the centred quantiser)
                x8 = self._prep_qk(x, weight, rope, True, for_keys, smooth=self.attn_smooth_k, sp=sp)
                # scale planes [2, H, stride] -> [lp, H * 2]: a head's (delta, constant) pair travels with its codes
                return x8.codes, x8.scales[:, :, :lp].permute(2, 1, 0).reshape(lp, 2 * (C // d))

            def send(packed, i):
                c0, c1 = chunks[i]
                return (sp.scatter_heads(packed[0], async_op=True, cols=(c0, c1)),
                        sp.scatter_heads(packed[1], async_op=True, cols=(2 * c0 // d, 2 * c1 // d)))

            def receive(pending, for_keys):
                return ops.Q8Rows.from_exchange(pending[0].wait(), pending[1].wait(), d, for_keys)
        else:
            _, hmap, where = sp.packed_layout(lp, C, d, chunks, q.device)

            def pack(x, weight, for_keys):
                return ops.rmsnorm_rope_scatter(x, weight, rope, d, torch.empty(lp * C, dtype=x.dtype, device=x.device), hmap, eps=self.eps)

            def send(packed, i):
                return sp.scatter_packed(packed, lp, *where[i], async_op=True)

            def receive(pending, for_keys):
                return pending.wait()

        qs = pack(q, sa.norm_q_weight, False)
        pend = [[send(qs, 0)]]                                    # chunk 0 of q flies under the k GEMM
        ks = pack(self._linear(sa.k, h), sa.norm_k_weight, True)
        pend[0].append(send(ks, 0))                               # ... of k under the v GEMM
        v = self._linear(sa.v, h)
        pend[0].append(sp.scatter_heads(v, async_op=True, cols=chunks[0]))
        for i in range(1, len(chunks)):
            pend.append([send(qs, i), send(ks, i), sp.scatter_heads(v, async_op=True, cols=chunks[i])])
        o = torch.empty(lp, C, dtype=self.act_dtype, device=q.device) if self.attn_qk8 else torch.empty_like(q)
        back = []
        for (c0, c1), (wq, wk, wv) in zip(chunks, pend):
            # after the exchange a rank holds ALL tokens of its heads: v's per-(head, channel) statistics, the attention-map
            # quantiser's per-key-column statistics over all queries and the window's band are all local
            qc, kc, vc = receive(wq, False), receive(wk, True), self._vq(wv.wait(), self.attn_v_bits, seq_len)
            oc = self._attend(qc, kc, vc, (c1 - c0) // d, seq_len, seq_len, self.attn_map, self.window_size)
            back.append(sp.gather_heads(oc, async_op=True, out=o, cols=(c0, c1)))
        for b in back:
            b.wait()
        return o

    def forward(self, x, e0, rope, seq_len, ctx, sp=None, e=None):
        """x: fp32 [L, C] residual stream (this rank's token shard under sequence parallelism), updated IN PLACE.
        e0: fp32 [1, 6, C].  rope: fp32 [pos, d/2, 2] for the local tokens.  seq_len: number of real (unpadded)
        tokens of the WHOLE sequence.  ctx: _FpSrc of the bf16 text context [Lc, C] (shared by all blocks so that
        its plain int8 copy is made once per pass).  sp: wan.distributed.SeqParallel or None.  e: this block's
        `modulation + e0` when the caller has it already (the model adds all blocks' modulations in one launch per pass)."""
        H = self.num_heads
        if e is None:
            e = self.modulation + e0  # [1, 6, C] fp32
        sa, ca = self.self_attn, self.cross_attn

        # ---- self attention: LN*(1+e1)+e0 -> q,k,v -> RMSNorm+RoPE -> attention -> o (+gate, +residual)
        h = _LnSrc(self, x, None, e[:, 0], e[:, 1])
        h.prefetch([sa.q, sa.k, sa.v])  # one pass over x for the three ViDiT-transformed int8 inputs
        q = self._linear(sa.q, h)
        if sp is not None and sp.size > 1:
            o = self._self_attention_ulysses(q, h, rope, seq_len, sp)
        else:
            q = self._prep_qk(q, sa.norm_q_weight, rope, self.attn_qk8, False)
            k = self._prep_qk(self._linear(sa.k, h), sa.norm_k_weight, rope, self.attn_qk8, True, smooth=self.attn_smooth_k)
            v = self._vq(self._linear(sa.v, h), self.attn_v_bits, seq_len)
            o = self._attend(q, k, v, H, seq_len, seq_len, self.attn_map, self.window_size)
        self._linear(sa.o, _FpSrc(o), gate=e[0, 2].contiguous(), residual=x)

        # ---- cross attention: LN_affine -> q; k,v from the text context
        h = _LnSrc(self, x, self.norm3_weight, self.norm3_bias.view(1, -1), None)
        q = self._linear(ca.q, h)
        k, v = self._context_kv(ctx)
        # cross_attn.attn_map under sequence parallelism: a rank's queries are a token shard here (the cross-attention is not
        # exchanged), but a key column's quantisation step is a maximum over ALL queries.  The queries of all ranks are gathered
        # (rank order == sequence order), every rank evaluates the whole map's statistics on the 512 keys and keeps its own rows:
        # the numerics of N = 1 bit for bit, for one all-gather of q per block -- an optional recipe, not the headline path.
        gather_q = self.cross_attn_map is not None and sp is not None and sp.size > 1
        if gather_q:
            q = sp.all_gather_rows(q)
        q = self._prep_qk(q, ca.norm_q_weight, None, self.cross_attn_qk8, False)
        o = self._attend(q, k, v, H, None, seq_len, self.cross_attn_map)
        if gather_q:
            o = sp.shard_rows(o).contiguous()
        self._linear(ca.o, _FpSrc(o), gate=self.ones_gate, residual=x)

        # ---- FFN: LN*(1+e4)+e3 -> GEMM -> GELU + quantise -> GEMM (+gate, +residual).  The GELU runs in ffn.2's quantiser when
        # that is a plain per-token quantiser (the memory-bound pass has the vector slack: 439 + 218 us against 494 + 199 us with
        # the GELU in the GEMM epilogue, whose store loop is vector-bound; cfg-B, tools/probes/ffn_gelu_placement.py); with a
        # rotation in front of ffn.2, or a floating-point ffn.2, it stays in ffn.0's epilogue.
        h = _LnSrc(self, x, None, e[:, 3], e[:, 4])
        late_gelu = _late_gelu(self.ffn0, self.ffn2)
        hid = self._linear(self.ffn0, h, gelu=not late_gelu)
        self._linear(self.ffn2, _FpSrc(hid, gelu=late_gelu), gate=e[0, 5].contiguous(), residual=x)
        return x
