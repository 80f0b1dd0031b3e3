"""Quantizers with the reference's interface (ViDiT-Q/quant_utils/qdiff/base/base_quantizer.py:13-162): modules
with `delta` / `zero_point` buffers ([G,1]) and an `init_done` flag.  All heavy lifting is HIP
(viditq_extension.fused): row statistics, static quantisation and the per-token dynamic quantiser; the [G]-sized
parameter arithmetic is plain fp32 torch (IEEE, bit-identical to the reference's CPU result).
Tensors must live on the GPU: there is no CPU path."""
import torch
import torch.nn as nn

from viditq_extension import fused

from ..config import ListConfig


class BaseQuantizer(nn.Module):
    def __init__(self, quant_config):
        super().__init__()
        self.n_bits = quant_config["n_bits"]
        self.sym = quant_config.get("sym", False)
        if isinstance(self.n_bits, list):
            raise AssertionError("when multiple n_bits are adopted, use the MixedPrecisionBaseQuantizer")
        self.register_buffer("delta", None)
        self.register_buffer("zero_point", None)
        if not isinstance(self.n_bits, ListConfig):
            self.n_levels = self.levels(self.n_bits, self.sym)
        self.init_done = False
        self.module_name = None

    @staticmethod
    def levels(n_bits, sym):
        return 2 ** (n_bits - 1) - 1 if sym else 2 ** n_bits  # base_quantizer.py:32


def _full(t, v):
    return torch.full_like(t, float(v))  # divide by a TENSOR: torch-GPU turns `/ python_scalar` into a reciprocal multiply


def static_params(x, n_bits, sym):
    """(delta [G], zero_point [G]) of StaticQuantizer.init_quant_params (base_quantizer.py:70-90)."""
    assert x.dim() == 2
    lo, hi, am = fused.row_minmax(x.contiguous())
    if sym:
        return am / _full(am, 2 ** (n_bits - 1) - 1), torch.zeros_like(am)
    n_levels = 2 ** n_bits
    hi, lo = hi.clamp_min(0.0), lo.clamp_max(0.0)
    delta = (hi - lo) / _full(hi, n_levels - 1)
    return delta, torch.round(lo / delta) + n_levels / 2


class StaticQuantizer(BaseQuantizer):
    """Per-row (output channel) static quantizer for weights.
    `group_size` g (the `weight.group_size` key): one (delta, zero_point) per row and per group of g input channels -- this same
    quantiser on w.view(N K / g, g), the [N_group, -1] input the reference's quantisers are written for (base_quantizer.py:72).
    `delta` / `zero_point` are then [N, K / g]; codes and the dequantised weight keep w's shape."""

    def __init__(self, quant_config):
        super().__init__(quant_config)
        self.group_size = quant_config.get("group_size", None)

    def _group_rows(self, x):
        """x [N, K] as the quantiser's rows: itself, or [N K / g, g]"""
        x = x.contiguous()
        g = getattr(self, "group_size", None)
        if g is None:
            return x
        if x.dim() != 2 or x.shape[1] % g:
            raise ValueError(f"{self.module_name or 'StaticQuantizer'}: weight.group_size={g} does not divide the row length of {tuple(x.shape)}")
        return x.view(-1, g)

    def init_quant_params(self, x):
        delta, zp = static_params(self._group_rows(x), self.n_bits, self.sym)
        if not torch.all(delta > 1e-6):
            raise AssertionError("unexpected small delta exists")  # the reference drops into ipdb here (:94-97)
        self.delta, self.zero_point = delta.view(x.shape[0], -1), zp.view(x.shape[0], -1)  # [N, 1], or [N, K / g]

    def codes_and_dequant(self, x, want_codes=True, want_dequant=True):
        if self.init_done is not True:
            self.init_quant_params(x)
        n = self.n_levels
        codes, deq = fused.weight_quant(self._group_rows(x), self.delta.reshape(-1).float().contiguous(),
                                        self.zero_point.reshape(-1).float().contiguous(), -n - 1, n, want_codes, want_dequant)
        codes, deq = (None if t is None else t.view(x.shape) for t in (codes, deq))
        if codes is not None and self.n_bits < 8:
            # The reference's clamp is one level looser than the bit-width: a row whose extremes tie exactly at a
            # .5 boundary (lo = -hi, e.g. lattice-valued rotated weights) produces a 17th level.  Integer STORAGE has 2^b
            # levels, so the codes saturate; the fake-quant `weight.data` keeps the reference's value.
            codes.clamp_(-(2 ** (self.n_bits - 1)), 2 ** (self.n_bits - 1) - 1)
        return codes, deq

    def quantize(self, x):
        return self.codes_and_dequant(x, True, False)[0].float()

    def forward(self, x):
        return self.codes_and_dequant(x, False, True)[1]


class DynamicQuantizer(BaseQuantizer):
    """Per-group (per-token) dynamic quantizer (base_quantizer.py:101-162).  Symmetric (:116-128; every Wan configuration): one
    fused HIP pass gives int8 codes, scale and sum.  Asymmetric (:130-149; selected by no Wan configuration, pinned by
    tests/golden/a2_dynamic_asym.npz): the row minimum / maximum, delta and zero point are those of the static asymmetric
    quantiser evaluated per call (same equations, eps floor 1e-8), on the same HIP kernels (row_minmax + weight_quant)."""

    # eps floors of delta: symmetric (:122-127) / asymmetric (:139-146).  MixedPrecisionDynamicQuantizer overrides both.
    _sym_floor, _asym_floor = 1e-6, 1e-8

    # ---- asymmetric branch ------------------------------------------------------------------------
    def _asym_params(self, x):
        lo, hi, _ = fused.row_minmax(x)
        hi, lo = hi.clamp_min(0.0), lo.clamp_max(0.0)
        delta = (hi - lo) / _full(hi, self.n_levels - 1)
        delta = torch.where(delta < self._asym_floor, _full(delta, self._asym_floor), delta)  # (the reference drops into ipdb first, then floors: :139-146)
        zp = torch.round(lo / delta) + self.n_levels / 2
        self.delta, self.zero_point = delta.unsqueeze(-1), zp.unsqueeze(-1)
        return delta.contiguous(), zp.contiguous()

    def _asym(self, x, want_codes, want_dequant, lo=None, hi=None):
        x = x.contiguous().float()
        delta, zp = self._asym_params(x)
        n = self.n_levels
        return fused.weight_quant(x, delta, zp, -n - 1 if lo is None else lo, n if hi is None else hi, want_codes, want_dequant)

    def quantize_int8(self, x, premul=None, rotation=None, want_sum=True):
        """int8 codes + fp32 (scale [T], sum [T]).  premul / rotation = (had_k, hadk): the ViDiT transform fused in.
        Asymmetric: the per-token zero point is left in `self.zero_point`; the caller adds its rank-one term
        (QuantizedLinear.forward).  int8 storage saturates the code 128 the reference's loose clamp admits at an exact tie (D9)."""
        x = x.contiguous()
        rows = x.shape[0]
        if not self.sym:
            if premul is not None or rotation is not None:
                # (x * mask) @ R first, in fp32, then the asymmetric quantiser on the transformed row, as the reference's
                # ViDiTQuantizedLinear.forward orders it (viditq_quant_layer.py:60-73 with base_quantizer.py:130-149)
                y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
                fused.rotate_quant(x, premul, rotation, None, None, out_fp=y, quantize=False)
                x = y
            codes, _ = self._asym(x, True, False, -128, 127)
            scale = self.delta.reshape(-1).float().contiguous()
            return codes, scale, (codes.float().sum(dim=1) * scale) if want_sum else None
        qs = torch.empty(2, rows, dtype=torch.float32, device=x.device)
        if self.n_bits != 8 or self._sym_floor != 1e-6:
            # any other range (n_bits < 8; the mixed-precision class has no floor): codes still fit int8 and the GEMM is unchanged.
            # Under a transform the transformed row is written out in fp32 first and quantised by the plain kernel (simulation
            # mode only: kernel-mode activations are always 8-bit)
            if not 2 <= self.n_bits <= 8:
                raise NotImplementedError(f"int8 activation codes hold 2..8 bits, not {self.n_bits}")
            if premul is not None or rotation is not None:
                y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
                fused.rotate_quant(x, premul, rotation, None, None, out_fp=y, quantize=False)
                x = y
            q = fused.quant_sum_levels(x, qs[1] if want_sum else None, qs[0], 2 ** (self.n_bits - 1) - 1, self._sym_floor)
        elif premul is None and rotation is None:
            q = fused.quant_sum(x, qs[1] if want_sum else None, qs[0])
        else:
            q = fused.rotate_quant(x, premul, rotation, qs[1] if want_sum else None, qs[0])
        self.delta, self.zero_point = qs[0].unsqueeze(-1), torch.zeros(rows, 1, device=x.device)
        return q, qs[0], qs[1]

    def forward_with_quant_params(self, x, delta, mixed_precision=None):
        """base_quantizer.py:164-206: fake-quant with a PRECOMPUTED delta of x's shape (the reference's block-wise attention-map and
        pre-softmax quantisers), optionally with a per-element bit-width tensor (0 bits = masked to zero).  Symmetric quantisers only,
        as the reference asserts; like the reference, `delta` is floored at 1e-6 IN PLACE.  One HIP launch (wanq_fake_quant_with_delta)."""
        assert self.sym
        if delta.shape != x.shape:
            delta = delta.expand_as(x)
        d32 = delta if (delta.dtype == torch.float32 and delta.is_contiguous()) else delta.float().contiguous()
        d32.clamp_min_(1e-6)
        bits = None if mixed_precision is None else mixed_precision.to(device=x.device, dtype=torch.int32).expand_as(x).contiguous()
        return fused.fake_quant_with_delta(x.contiguous(), d32, self.n_bits, bits)

    def quantize(self, x):
        assert x.dim() == 2
        if not self.sym:  # (8 bits: codes live in int8 storage, which saturates the 2^b-th level of the reference's loose clamp, D9)
            return self._asym(x, True, False, *((-128, 127) if self.n_bits == 8 else (None, None)))[0].float()
        return self.quantize_int8(x, want_sum=False)[0].float()

    def forward(self, x):
        if not self.sym:
            return self._asym(x, False, True)[1]
        q, scale, _ = self.quantize_int8(x, want_sum=False)
        return q.float() * scale.unsqueeze(-1)


# ---- OCP fp8 (e4m3fn): `format: fp8_e4m3` ---------------------------------------------------------------------------------
FP8_FORMAT = "fp8_e4m3"
FP8_MAX = 448.0
_FP8_LUT = {}


def fp8_decode(codes):
    """fp32 values of uint8 e4m3fn bit patterns (exact; a 256-entry table on the codes' device)."""
    lut = _FP8_LUT.get(codes.device)
    if lut is None:
        lut = _FP8_LUT[codes.device] = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(codes.device)
    return lut[codes.long()]


def fp8_quant_rows(x, gelu=False):
    """(codes uint8, scale fp32 [rows]) of the per-row dynamic e4m3 quantiser: scale = max(absmax / 448, 1e-6), codes =
    e4m3fn_rne(clamp(x / scale, -448, 448)).  On the GPU wanq_quant_rows_fp8; in host memory the torch expression it is bit-equal to
    (this torch build casts fp32 -> float8_e4m3fn on the CPU to nearest even and keeps subnormals)."""
    if x.is_cuda:
        return fused.quant_rows_fp8(x.contiguous(), gelu)
    x = x.float()
    if gelu:
        x = torch.nn.functional.gelu(x, approximate="tanh")
    am = x.abs().amax(dim=-1, keepdim=True)
    s = (am / _full(am, FP8_MAX)).clamp_min(1e-6)
    codes = (x / s).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, s.reshape(-1)


class Fp8Quantizer(BaseQuantizer):
    """`format: fp8_e4m3` of a `weight:` or `act:` section (n_bits 8, sym True): one fp32 scale per row -- per output channel for a
    weight, per token for an activation -- and OCP e4m3fn codes.  `delta` [rows, 1] is the scale, `zero_point` zeros, as the integer
    quantisers keep them (save / load_quant_param_dict).  The scale is a function of the tensor alone (absmax / 448, floored at
    1e-6): nothing is fitted or calibrated, so it is derived again at every call, for a weight too."""

    def __init__(self, quant_config):
        super().__init__(quant_config)
        self.format = FP8_FORMAT

    def codes_and_scale(self, x, gelu=False):
        codes, scale = fp8_quant_rows(x, gelu)
        self.delta, self.zero_point = scale.unsqueeze(-1), torch.zeros(scale.shape[0], 1, device=scale.device)
        return codes, scale

    def codes_and_dequant(self, x, want_codes=True, want_dequant=True):
        codes, scale = self.codes_and_scale(x)
        return codes, (fp8_decode(codes) * scale.unsqueeze(-1)) if want_dequant else None

    def quantize(self, x):
        return fp8_decode(self.codes_and_scale(x)[0])

    def forward(self, x):
        return self.codes_and_dequant(x, False, True)[1]


# ---- OCP Microscaling (MX): `format: mxfp8_e4m3` / `format: mxfp4_e2m1` -------------------------------------------------------
# One E8M0 power-of-two scale per block of 32 consecutive input channels (include/wanq_hip.h, wanq_quant_rows_mx).  Repository-
# defined; the reference has no counterpart.  What follows is the host expression of the format: what simulation mode runs in host
# memory and what the GPU entry is bit-equal to.
MXFP8_FORMAT, MXFP4_FORMAT, MXFP6_FORMAT = "mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3fn"
MX_FORMATS = (MXFP8_FORMAT, MXFP4_FORMAT, MXFP6_FORMAT)
MX_BLOCK = 32
# emax, largest magnitude, the `fmt` code of the C ABI (WANQ_MX_E2M3 = 2 is wanq_quant_rows_mx6's and wanq_gemm_mx6's alone)
_MX_SPEC = {MXFP8_FORMAT: (8, 448.0, 0), MXFP4_FORMAT: (2, 6.0, 1), MXFP6_FORMAT: (2, 7.5, 2)}
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# the 32 e2m3 magnitudes by code: E in bits 3-4 (bias 1), M in bits 0-2; E = 0: M / 8, else 2^(E - 1) (1 + M / 8)
E2M3_VALUES = tuple((c & 7) / 8 if c < 8 else 2.0 ** ((c >> 3) - 1) * (1 + (c & 7) / 8) for c in range(32))


def mx_fmt_code(fmt):
    return _MX_SPEC[fmt][2]


def _pow2_f64(e):
    """2.0 ** e for an integer tensor e in [-1022, 1023], exactly, as float64 (the exponent field written directly)"""
    return ((e.long() + 1023) << 52).view(torch.float64)


def mx_pack_e2m1(codes):
    """[rows, cols] 4-bit codes -> [rows, cols / 2] bytes: element k in byte k / 2, even k in the low nibble"""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).contiguous()


def mx_unpack_e2m1(packed):
    """[rows, cols / 2] bytes -> [rows, cols] 4-bit codes"""
    return torch.stack((packed & 0xf, packed >> 4), dim=-1).reshape(*packed.shape[:-1], packed.shape[-1] * 2)


def mx_pack_e2m3(codes):
    """[rows, cols] 6-bit codes -> [rows, 3 cols / 4] bytes: block b of 32 codes is bytes 24 b .. 24 b + 23, element j of the block in bits
    6 j .. 6 j + 5 of that 192-bit little-endian string.  Four codes make three bytes and 32 is a multiple of 4, so this is the
    little-endian packing of the whole row."""
    c = codes.to(torch.int32).reshape(*codes.shape[:-1], codes.shape[-1] // 4, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack((w & 0xff, (w >> 8) & 0xff, w >> 16), dim=-1).to(torch.uint8).reshape(*codes.shape[:-1], codes.shape[-1] // 4 * 3)


def mx_unpack_e2m3(packed):
    """[rows, 3 cols / 4] bytes -> [rows, cols] 6-bit codes"""
    b = packed.to(torch.int32).reshape(*packed.shape[:-1], packed.shape[-1] // 3, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack((w & 63, (w >> 6) & 63, (w >> 12) & 63, w >> 18), dim=-1).to(torch.uint8).reshape(
        *packed.shape[:-1], packed.shape[-1] // 3 * 4)


def mx_hadamard32_host(x):
    """x [..., cols] fp32 with every block of 32 columns replaced by its unnormalised Sylvester-Hadamard transform, x_block H with
    H[i][j] = (-1)^popcount(i & j): five butterfly stages in fp32, in the order h = 1, 2, 4, 8, 16, each (x_i, x_{i+h}) <- (x_i +
    x_{i+h}, x_i - x_{i+h}) for bit h of i clear.  Only additions and subtractions, one rounding each, in the order
    wanq_quant_rows_mx_had32 performs them: this is the definition that entry is bit-equal to.  H is symmetric and H H = 32 I."""
    x = x.float()
    if x.shape[-1] % MX_BLOCK:
        raise ValueError(f"mx_hadamard32: cols={x.shape[-1]} must be a multiple of {MX_BLOCK}")
    v = x.reshape(-1, MX_BLOCK)
    h = 1
    while h < MX_BLOCK:
        v = v.reshape(-1, MX_BLOCK // (2 * h), 2, h)
        a, b = v[:, :, 0, :], v[:, :, 1, :]
        v = torch.stack((a + b, a - b), dim=2)
        h *= 2
    return v.reshape(x.shape)


def mx_quant_rows_host(x, fmt, gelu=False, had32=False):
    """(codes uint8, scale bytes uint8 [rows, cols / 32]) of the block quantiser, in torch on x's device.  Per block: amax, E = its
    biased fp32 exponent field, s = clamp(E - emax, 0, 254), c = rne(clamp(x 2^(127 - s), -max, max)).  The scaling is done in
    float64, where it is exact; the one rounding is the cast to e4m3fn (this torch build rounds to nearest even and keeps subnormals)
    or, for e2m1, the comparison against the seven midpoints with ties to the even code, or, for e2m3 (`mxfp6_e2m3fn`, include/wanq_hip.h:
    wanq_quant_rows_mx6), rne(|t| / q) with the binade's quantum q = 1/8 for |t| < 2, 1/4 for |t| < 4, else 1/2 -- the magnitude codes
    ascend with the value, so the code is that integer plus 0, 8 or 16 and the tie goes to the even code.  `had32`: the blocks go
    through mx_hadamard32_host behind the GELU and in front of the block maximum (wanq_quant_rows_mx_had32; not for e2m3)."""
    emax, vmax, _ = _MX_SPEC[fmt]
    if had32 and fmt == MXFP6_FORMAT:
        raise ValueError(f"mx_quant_rows: {MXFP6_FORMAT} has no had32 form")
    x = x.float()
    if gelu:
        x = torch.nn.functional.gelu(x, approximate="tanh")
    rows, cols = x.shape
    if cols % MX_BLOCK:
        raise ValueError(f"mx_quant_rows: cols={cols} must be a multiple of {MX_BLOCK}")
    if had32:
        x = mx_hadamard32_host(x)
    xb = x.reshape(rows, cols // MX_BLOCK, MX_BLOCK)
    amax = xb.abs().amax(dim=-1).contiguous()
    s = (((amax.view(torch.int32) >> 23) & 0xff) - emax).clamp(0, 254)
    t = (xb.double() * _pow2_f64(127 - s).unsqueeze(-1)).clamp(-vmax, vmax).reshape(rows, cols)
    if fmt == MXFP8_FORMAT:
        codes = t.float().to(torch.float8_e4m3fn).view(torch.uint8)
    elif fmt == MXFP6_FORMAT:
        a = t.abs()
        mag = torch.where(a < 2, torch.round(a * 8), torch.where(a < 4, torch.round(a * 4) + 8, torch.round(a * 2) + 16))
        codes = mx_pack_e2m3(mag.to(torch.uint8) | (torch.signbit(t).to(torch.uint8) << 5))
    else:
        a = t.abs()
        mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)).to(torch.uint8)
        codes = mx_pack_e2m1(mag | (torch.signbit(t).to(torch.uint8) << 3))
    return codes, s.to(torch.uint8)


def mx_quant_rows(x, fmt, gelu=False, had32=False):
    """The block quantiser: on the GPU wanq_quant_rows_mx (`had32`: wanq_quant_rows_mx_had32), in host memory the host expression it is
    bit-equal to."""
    if x.is_cuda:
        return fused.quant_rows_mx(x.contiguous(), fmt, gelu, had32)
    return mx_quant_rows_host(x, fmt, gelu, had32)


def mx_decode(codes, scale_u8, fmt, dtype=torch.float32):
    """Dequantised values [rows, cols] of codes + scale bytes: value(code) 2^(s - 127), exact in float64 (and in fp32 wherever the
    result is a normal fp32 number, as for anything the quantiser wrote)."""
    if fmt == MXFP8_FORMAT:
        v = fp8_decode(codes).double()
    elif fmt == MXFP6_FORMAT:
        c = mx_unpack_e2m3(codes).long()
        lut = torch.tensor(E2M3_VALUES, dtype=torch.float64, device=codes.device)
        v = lut[c & 31] * (1 - 2 * (c >> 5)).double()
    else:
        c = mx_unpack_e2m1(codes).long()
        lut = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=codes.device)
        v = lut[c & 7] * (1 - 2 * (c >> 3)).double()
    rows, cols = v.shape
    v = v.reshape(rows, cols // MX_BLOCK, MX_BLOCK) * _pow2_f64(scale_u8.long() - 127).unsqueeze(-1)
    return v.reshape(rows, cols).to(dtype)


class MxQuantizer(BaseQuantizer):
    """`format: mxfp8_e4m3` / `mxfp6_e2m3fn` / `mxfp4_e2m1` of a `weight:` or `act:` section (n_bits 8 / 6 / 4, sym True): one E8M0 scale
    byte per row and block of 32 input channels, e4m3 bytes, packed e2m3 codes (three bytes per four) or packed e2m1 nibbles.  `scale_u8` [rows, cols / 32] holds the bytes as the GEMM reads
    them; `delta` = 2^(scale_u8 - 127) and `zero_point` zeros keep the integer quantisers' names (save / load_quant_param_dict).
    Nothing is fitted or calibrated: the scales are a function of the tensor alone and are derived again at every call.
    `had32` (the config's `mx: {block_hadamard: True}`): every block is quantised behind its unnormalised 32-point Hadamard
    transform, and the codes, the scales and `dequantize` all live in that rotated domain.  A `weight_side` quantiser then takes
    w / 32 (an exact power of two), so that (x H)(w H / 32)^T = x w^T: rotated activations against the rotated weight need no inverse."""

    def __init__(self, quant_config, had32=False, weight_side=False):
        super().__init__(quant_config)
        self.format = quant_config["format"]
        self.had32, self.weight_side = bool(had32), bool(weight_side)
        self.register_buffer("scale_u8", None, persistent=False)

    def codes_and_scale(self, x, gelu=False):
        if self.had32 and self.weight_side:
            x = x.float() * 0.03125
        codes, s = mx_quant_rows(x, self.format, gelu, self.had32)
        self.scale_u8 = s
        self.delta = _pow2_f64(s.long() - 127).float()
        self.zero_point = torch.zeros_like(self.delta)
        return codes, s

    def dequantize(self, codes, scale_u8):
        return mx_decode(codes, scale_u8, self.format)

    def codes_and_dequant(self, x, want_codes=True, want_dequant=True):
        codes, s = self.codes_and_scale(x)
        return codes, self.dequantize(codes, s) if want_dequant else None

    def quantize(self, x):
        return self.codes_and_scale(x)[0]

    def forward(self, x):
        return self.codes_and_dequant(x, False, True)[1]
