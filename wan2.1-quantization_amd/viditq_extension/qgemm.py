"""`viditq_extension.qgemm` -- same functions as the reference pybind module
(ViDiT-Q/kernels/csrc/qgemm/pybind.cpp:5-12), executed by the int8-MFMA kernel in csrc/gemm_w8a8.hip.

Widenings: any M (ragged last tile in-kernel), N % 8 == 0, K % 16 == 0 (reference: M,N % 128, K % 64, and a
C assert that aborts the process otherwise); per-token / per-channel vectors fp16 or fp32; zero point
int16 or fp32; output fp16 (reference), bf16 or fp32; launched on the CURRENT stream (reference: legacy
default stream).
"""
import contextlib
import os

import torch

from . import _C

_VEC = (torch.float16, torch.float32)

_timer = None


def set_timer(t):
    """bench.py hook: when set to a list, every GEMM launch appends (start_event, end_event, int8 ops), the
    events bracketing exactly that launch on the current stream."""
    global _timer
    _timer = t


@contextlib.contextmanager
def _timed(ops):
    """The int8 timer's bracket (`set_timer`) around what the body launches on the current stream: `ops` int8 operations."""
    if _timer is None:
        yield
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    yield
    ev1.record()
    _timer.append((ev0, ev1, ops))


def _check_mat(name, t, dtype, *shape):
    """A matrix operand: on the GPU, contiguous, of `dtype`, of rank 2 and, when given, of `shape`."""
    _C.check_gpu(name, t)
    _C.check_contig(name, t)
    _C.check_dtype(name, t, dtype)
    if t.dim() != 2:
        raise RuntimeError(f"Tensor {name} must have dimension number (2)")
    if shape:
        _C.check_shape(name, t, *shape)


def _check_i8(name, t, rows=None, cols=None):
    _check_mat(name, t, torch.int8, *(() if rows is None else (rows, cols)))


def _check_vec(name, t, n, dtypes=_VEC):
    if t is None:
        return
    _C.check_gpu(name, t)
    _C.check_contig(name, t)
    _C.check_dtype(name, t, *dtypes)
    _C.check_shape(name, t, n)


def _epi_flags(gelu, gate, residual, M, N, out_dtype):
    """The epilogue flags of a launch, after the checks on gate (fp32 [N]) and residual ([M, N] of the out dtype): both or neither."""
    epi = _C.EPI_GELU if gelu else 0
    if gate is not None or residual is not None:
        if gate is None or residual is None:
            raise RuntimeError("gate and residual must be given together")
        _check_vec("gate", gate, N, (torch.float32,))
        _C.check_gpu("residual", residual)
        _C.check_contig("residual", residual)
        _C.check_dtype("residual", residual, out_dtype)
        _C.check_shape("residual", residual, M, N)
        epi |= _C.EPI_GATE_RES
    return epi


def _out_for(out, M, N, out_dtype, device):
    """`out` checked against [M, N] of out_dtype, or a fresh tensor when None."""
    if out is None:
        return torch.empty((M, N), dtype=out_dtype, device=device)
    _C.check_gpu("out", out)
    _C.check_contig("out", out)
    _C.check_dtype("out", out, out_dtype)
    _C.check_shape("out", out, M, N)
    return out


# Packed 4-bit weights at large M: the int8 matrix cores are the bound, not the weight bytes, so the fastest W4A8 product on this
# machine is the W8 ping-pong kernel on codes expanded ONCE per launch (wanq_unpack_w4: 1.5 N K bytes of traffic, 1-6 % of the
# product's time from 32760 down to 9450 rows) instead of once per tile inside the kernel (wanq_gemm_w4a8's in-register expansion
# costs ~20 % there).  The nibbles u = q + 8 go in as they are: the 8 rides in the zero point both ways (include/wanq_hip.h), the
# int32 accumulators and the epilogue are the same, outputs bit-equal (tests/test_gpu_gemm.py).  Weights stay packed at rest; the
# expanded copy lives for the launch.  WANQ_W4_UNPACK_ROWS: minimum M (0 = never).
_W4_UNPACK_ROWS = int(os.environ.get("WANQ_W4_UNPACK_ROWS", "2048"))


def w8a8_linear(input, weight, scale_input, scale_weight, bias=None, input_sum=None, zp_weight=None,
                out_dtype=torch.float16, gelu=False, gate=None, residual=None, out=None, w4=False):
    """General entry: y = epilogue(int8 input[M,K] @ int8 weight[N,K]^T); see include/wanq_hip.h.

    gate (fp32 [N]) + residual ([M,N], out dtype): y = residual + y * gate (may alias `out`).
    w4=True: `weight` is uint8 [N, K/2], unsigned 4-bit codes in the pack_w4 layout (wanq_gemm_w4a8; at M >= WANQ_W4_UNPACK_ROWS and
    K % 128 == 0 expanded once and multiplied by the W8 ping-pong kernel, see _W4_UNPACK_ROWS)."""
    _check_i8("input", input)
    M, K = input.shape
    if w4:
        _C.check_gpu("weight", weight)
        _C.check_contig("weight", weight)
        _C.check_dtype("weight", weight, torch.uint8)
        N = weight.shape[0]
        _C.check_shape("weight", weight, N, K // 2)
        if K % 32:
            raise RuntimeError(f"w4a8: K={K} must be a multiple of 32")
    else:
        _check_i8("weight", weight)
        N = weight.shape[0]
        _C.check_shape("weight", weight, N, K)
    _check_vec("scale_input", scale_input, M)
    _check_vec("scale_weight", scale_weight, N)
    _check_vec("bias", bias, N)
    _check_vec("input_sum", input_sum, M)
    _check_vec("zp_weight", zp_weight, N, (torch.int16, torch.float32))
    if input_sum is not None and input_sum.dtype != scale_input.dtype:
        raise RuntimeError("input_sum and scale_input must share a dtype")
    if bias is not None and bias.dtype != scale_weight.dtype:
        raise RuntimeError("bias and scale_weight must share a dtype")
    if zp_weight is not None and input_sum is None:
        raise RuntimeError("asymmetric weights (zp_weight) need input_sum")
    epi = _epi_flags(gelu, gate, residual, M, N, out_dtype)
    out = _out_for(out, M, N, out_dtype, input.device)
    _C.check_same_device(input, weight, scale_input, scale_weight, bias, input_sum, zp_weight, gate, residual, out)
    with torch.cuda.device(input.device), _timed(2 * M * N * K):
        if w4 and _W4_UNPACK_ROWS and M >= _W4_UNPACK_ROWS and K % 128 == 0 and K >= 256:
            weight, w4 = unpack_w4(weight, bias=0, out=_w4_scratch_for(weight)), False  # inside the timed region: part of this product's cost
        _C.call("wanq_gemm_w4a8" if w4 else "wanq_gemm_w8a8", _C.ptr(input), _C.ptr(weight), _C.ptr(out), _C.dt(out_dtype), _C.ptr(scale_input),
                _C.ptr(input_sum), _C.dt(scale_input), _C.ptr(scale_weight), _C.ptr(bias), _C.dt(scale_weight),
                _C.ptr(zp_weight), _C.dt(zp_weight) if zp_weight is not None else _C.F32, _C.ptr(gate),
                _C.ptr(residual), epi, M, N, K, _C.stream())
    return out


def w8a8_of16_bias_weight_asym(input, weight, bias, scale_input, scale_weight, input_sum, zp_weight):
    """fp16( acc*sA*sB + sumA*zp*sB + bias )."""
    return w8a8_linear(input, weight, scale_input, scale_weight, bias, input_sum, zp_weight)


def w8a8_of16_bias_weight_sym(input, weight, bias, scale_input, scale_weight):
    """fp16( acc*sA*sB + bias )."""
    return w8a8_linear(input, weight, scale_input, scale_weight, bias)


def w8a8_of16_nobias_weight_sym_qserve(input, weight, scale_input, scale_weight):
    """fp16( acc*sW*sA ), no bias."""
    return w8a8_linear(input, weight, scale_input, scale_weight)


def w8a8_o32(input, weight):
    """Raw int32 accumulators."""
    _check_i8("input", input)
    M, K = input.shape
    _check_i8("weight", weight)
    N = weight.shape[0]
    _C.check_shape("weight", weight, N, K)
    _C.check_same_device(input, weight)
    out = torch.empty((M, N), dtype=torch.int32, device=input.device)
    with torch.cuda.device(input.device):
        _C.call("wanq_gemm_w8a8", _C.ptr(input), _C.ptr(weight), _C.ptr(out), _C.I32, None, None, _C.F32, None, None,
                _C.F32, None, _C.F32, None, None, 0, M, N, K, _C.stream())
    return out


# ---- W4 -----------------------------------------------------------------------------------------------------------
def pack_w4(codes, bias=8):
    """int8 codes [N, K] (signed [-8,7] with bias 8, or unsigned 0..15 with bias 0) -> uint8 [N, K/2] in the library's
    packed layout (include/wanq_hip.h: 32 codes -> 16 bytes arranged as int8-MFMA operand nibbles)."""
    _check_i8("codes", codes)
    N, K = codes.shape
    out = torch.empty((N, K // 2), dtype=torch.uint8, device=codes.device)
    with torch.cuda.device(codes.device):
        _C.call("wanq_pack_w4", _C.ptr(codes), _C.ptr(out), int(bias), N, K, _C.stream())
    return out


_w4_scratch = {}


def _w4_scratch_for(packed):
    """ONE int8 [N, K] buffer per (device, stream, N, K) for the large-M W4A8 path (a fresh 70-MB tensor per launch at the
    14B FFN shapes was twice the packed weights' footprint and invisible to the memory accounting).  Launches on one stream are
    ordered, so the GEMM that reads the expansion is enqueued before the next expansion that overwrites it."""
    N, K2 = packed.shape
    key = (packed.device, torch.cuda.current_stream(packed.device).cuda_stream, N, K2 * 2)
    buf = _w4_scratch.get(key)
    if buf is None:
        buf = _w4_scratch[key] = torch.empty((N, K2 * 2), dtype=torch.int8, device=packed.device)
    return buf


def w4_scratch_bytes(device=None):
    """Bytes held by the large-M W4A8 path's expansion buffers (reported beside the sharded weights by bench.py / --dit_fsdp)."""
    return sum(b.numel() for k, b in _w4_scratch.items() if device is None or k[0] == torch.device(device))


def unpack_w4(packed, bias=8, out=None):
    """uint8 [N, K/2] -> int8 codes [N, K] (into `out` when given)."""
    _C.check_gpu("packed", packed)
    _C.check_contig("packed", packed)
    _C.check_dtype("packed", packed, torch.uint8)
    N, K2 = packed.shape
    if out is None:
        out = torch.empty((N, K2 * 2), dtype=torch.int8, device=packed.device)
    else:
        _check_i8("out", out, N, K2 * 2)
    with torch.cuda.device(packed.device):
        _C.call("wanq_unpack_w4", _C.ptr(packed), _C.ptr(out), int(bias), N, K2 * 2, _C.stream())
    return out


def w4a8_o32(input, kernel):
    """Raw int32 accumulators of int8 input [M, K] x unsigned 4-bit codes (packed uint8 [N, K/2])."""
    _check_i8("input", input)
    M, K = input.shape
    N = kernel.shape[0]
    _C.check_dtype("kernel", kernel, torch.uint8)
    _C.check_shape("kernel", kernel, N, K // 2)
    out = torch.empty((M, N), dtype=torch.int32, device=input.device)
    with torch.cuda.device(input.device):
        _C.call("wanq_gemm_w4a8", _C.ptr(input), _C.ptr(kernel), _C.ptr(out), _C.I32, None, None, _C.F32, None, None,
                _C.F32, None, _C.F32, None, None, 0, M, N, K, _C.stream())
    return out


def w4a8_of16_nobias_weight_asym_qserve(in_feats, kernel, wscales, ascales, w_szs, a_ssums, out_feats):
    """Reference signature (ViDiT-Q/kernels/csrc/qgemm/pybind.cpp:12): writes out_feats (fp16 [M, N]).
    kernel: UNSIGNED 4-bit codes packed two per byte, uint8 [N, K/2] in THIS library's layout (pack_w4(..., bias=0));
    y = acc * wscales[n] * ascales[m] - w_szs[n] * a_ssums[m]  with w_szs = scale*zero
    (w4a8_per_channel_gemm_cuda_qserve.cu:580-587).  The nibbles are expanded in registers inside the GEMM."""
    vec = ascales.dtype
    zp = (-(w_szs.float() / wscales.float())).contiguous()  # asym epilogue: + a_ssum * zp * wscale
    w8a8_linear(in_feats, kernel, ascales, wscales.to(vec), None, a_ssums, zp.float(), out_dtype=out_feats.dtype, out=out_feats,
                w4=True)


# ---- 16-bit floating point ----------------------------------------------------------------------------------------
_BIAS16 = (torch.bfloat16, torch.float16, torch.float32)


def _check_operands16(input, wname, weight, wdtype):
    """The operand checks fp_linear and wq16_linear share: `input` bf16 / fp16 [M, K], `weight` (named `wname` in messages) a matrix
    of `wdtype` (None: the input's dtype).  -> M, N, K"""
    _C.check_gpu("input", input)
    _C.check_gpu(wname, weight)
    _C.check_contig("input", input)
    _C.check_contig(wname, weight)
    _C.check_dtype("input", input, torch.bfloat16, torch.float16)
    _C.check_dtype(wname, weight, wdtype or input.dtype)
    if input.dim() != 2 or weight.dim() != 2:
        raise RuntimeError(f"Tensors input and {wname} must have dimension number (2)")
    M, K = input.shape
    return M, weight.shape[0], K


def _shape_refusal(M, N, K, k_step, bounded=False):
    """The shape rules the entries share, in the order they check them: N a positive multiple of 8, K one of `k_step` (None: the
    entry has a K rule of its own) and, for a `bounded` entry, M's range before and the tile count after."""
    if bounded and (M < 0 or M >= (1 << 31) - 128):
        return f"M={M} out of range"
    if N < 8 or N % 8:
        return f"N={N} must be a positive multiple of 8"
    if k_step is not None and (K < k_step or K % k_step):
        return f"K={K} must be a positive multiple of {k_step}"
    if bounded and ((M + 127) // 128) * ((N + 127) // 128) >= (1 << 31):
        return "too many tiles"
    return None


def _check_group_params(K, N, group_size, scale_weight, zp):
    """scale_weight and zp of a group-wise entry: fp32 [K / group_size, N] (zp may be None)."""
    for name, t in (("scale_weight", scale_weight), ("zp", zp)):
        if t is not None:
            _C.check_gpu(name, t)
            _C.check_contig(name, t)
            _C.check_dtype(name, t, torch.float32)
            _C.check_shape(name, t, K // group_size, N)


def _launch16(entry, lead, operands, bias, out_dtype, gelu, gate, residual, out, M, N, K):
    """What the entries with the 16-bit GEMMs' epilogue share behind their operand checks: bias, epilogue flags, `out`, one device,
    then `entry`(*lead, out, out dtype, bias, bias dtype, gate, residual, epi, M, N, K, stream).  -> out"""
    _check_vec("bias", bias, N, _BIAS16)
    epi = _epi_flags(gelu, gate, residual, M, N, out_dtype)
    out = _out_for(out, M, N, out_dtype, operands[0].device)
    _C.check_same_device(*operands, bias, gate, residual, out)
    with torch.cuda.device(operands[0].device):
        _C.call(entry, *lead, _C.ptr(out), _C.dt(out_dtype), _C.ptr(bias), _C.dt(bias) if bias is not None else _C.F32, _C.ptr(gate),
                _C.ptr(residual), epi, M, N, K, _C.stream())
    return out


def fp_linear(input, weight, bias=None, out_dtype=None, gelu=False, gate=None, residual=None, out=None):
    """y = epilogue(input[M,K] @ weight[N,K]^T) on the bf16 / fp16 matrix cores (wanq_gemm_bf16, csrc/gemm_bf16.hip); input and
    weight share a dtype (bf16 or fp16).  Epilogue in fp32: + bias, tanh-GELU (`gelu`), residual + y * gate (gate fp32 [N], residual
    [M,N] of out_dtype, may alias `out`), one rounding to out_dtype (default: the input's dtype).  A row's bits do not depend on M
    or on where the row sits in the launch.  Not counted by the int8 timer (`set_timer`)."""
    M, N, K = _check_operands16(input, "weight", weight, None)
    _C.check_shape("weight", weight, N, K)
    return _launch16("wanq_gemm_bf16", (_C.ptr(input), _C.ptr(weight), _C.dt(input)), (input, weight), bias,
                     out_dtype or input.dtype, gelu, gate, residual, out, M, N, K)


def fp_linear_refusal(M, N, K):
    """Why wanq_gemm_bf16 would refuse an [M, K] x [N, K] product (None = accepted): the shape rules of include/wanq_hip.h, checked on
    the host so that a model can name a layer the kernel cannot take when it is built, not in its first forward."""
    return _shape_refusal(M, N, K, 32)


# ---- weight-only quantisation: 16-bit activations x integer weight codes --------------------------------------------
def wq16_linear(input, codes, scale_weight, zp=None, bias=None, out_dtype=None, gelu=False, gate=None, residual=None, out=None,
                w4=False):
    """y = epilogue(scale_weight[n] * input[M,K] @ (codes[N,K] + zp[n])^T) on the bf16 / fp16 matrix cores (wanq_gemm_wq16,
    csrc/gemm_wq16.hip): `input` bf16 or fp16, `codes` int8 [N, K] or, with w4=True, uint8 [N, K/2] unsigned nibbles in the pack_w4
    layout (zp = zero_point - 8 then); scale_weight and zp fp32 [N].  The codes become MFMA fragments in registers, exactly (c + zp
    is an integer of at most 8 bits); epilogue as `fp_linear`.  Not counted by the int8 timer (`set_timer`).
    `zp` must be integer valued, as StaticQuantizer's rounded zero point is: the kernel cuts the 16-bit operand from the fp32 sum
    c + zp (bf16: truncation, fp16: round toward zero), so a fractional zp would be quantised silently, and differently for the two
    activation types."""
    M, N, K = _check_operands16(input, "codes", codes, torch.uint8 if w4 else torch.int8)
    _C.check_shape("codes", codes, N, K // 2 if w4 else K)
    _check_vec("scale_weight", scale_weight, N, (torch.float32,))
    _check_vec("zp", zp, N, (torch.float32,))
    return _launch16("wanq_gemm_wq16", (_C.ptr(input), _C.ptr(codes), _C.dt(input), 4 if w4 else 8, _C.ptr(scale_weight), _C.ptr(zp)),
                     (input, codes, scale_weight, zp), bias, out_dtype or input.dtype, gelu, gate, residual, out, M, N, K)


def wq16_grouped_linear(input, codes, scale_weight, zp=None, group_size=None, bias=None, out_dtype=None, gelu=False, gate=None,
                        residual=None, out=None, w4=False):
    """`wq16_linear` with one scale and one zero point per output channel and per group of `group_size` input channels
    (wanq_gemm_wq16_grouped): scale_weight and zp fp32 [K / group_size, N] (group-major).  Each group's partial sum is accumulated on
    the matrix cores from the exact operand c + zp[g, n] and folded into the result by one fp32 fma with scale_weight[g, n], groups
    ascending; then + bias and the epilogue of `fp_linear`.  group_size % 64 == 0 and K % group_size == 0."""
    M, N, K = _check_operands16(input, "codes", codes, torch.uint8 if w4 else torch.int8)
    _C.check_shape("codes", codes, N, K // 2 if w4 else K)
    why = wq16_linear_refusal(M, N, K, group_size)
    if why is not None:
        raise RuntimeError(f"wq16_grouped_linear: {why}")
    _check_group_params(K, N, group_size, scale_weight, zp)
    return _launch16("wanq_gemm_wq16_grouped", (_C.ptr(input), _C.ptr(codes), _C.dt(input), 4 if w4 else 8, _C.ptr(scale_weight),
                                                _C.ptr(zp), int(group_size)),
                     (input, codes, scale_weight, zp), bias, out_dtype or input.dtype, gelu, gate, residual, out, M, N, K)


def wq16_linear_refusal(M, N, K, group_size=None):
    """Why wanq_gemm_wq16 -- with a `group_size`, wanq_gemm_wq16_grouped -- would refuse an [M, K] x [N, K] product (None =
    accepted); see `fp_linear_refusal`."""
    why = _shape_refusal(M, N, K, 64)
    if why is not None or group_size is None:
        return why
    if not isinstance(group_size, int) or group_size < 64 or group_size % 64:
        return f"group_size={group_size} must be a positive multiple of 64"
    if K % group_size:
        return f"K={K} must be a multiple of group_size={group_size}"
    return None


LOWRANK_MAX = 256  # the largest (padded) rank wanq_gemm_wq16_lowrank takes; ranks are padded to multiples of 64


def wq16_lowrank_linear(input, codes, scale_weight, zp, group_size, t, b, bias=None, out_dtype=None, gelu=False, gate=None,
                        residual=None, out=None, w4=False):
    """`wq16_linear` (group_size None or 0) or `wq16_grouped_linear` with a 16-bit low-rank side branch added inside the GEMM
    (wanq_gemm_wq16_lowrank): y = epilogue(y0 + t[M,R] @ b[N,R]^T), y0 what that entry has before its GELU.  `t` and `b` have the
    input's dtype; `t` is `fp_linear(input, A)` for the [R, K] factor A, rounded once to that dtype -- the rounding is part of the
    definition.  R % 64 == 0, 64 <= R <= 256 (zero pad a smaller rank: a zero column contributes exactly 0).  The branch is summed in
    fp32 in an accumulator set of its own and added once, behind the bias and before GELU and gate + residual."""
    M, N, K = _check_operands16(input, "codes", codes, torch.uint8 if w4 else torch.int8)
    _C.check_shape("codes", codes, N, K // 2 if w4 else K)
    group_size = group_size or None
    for name, x in (("t", t), ("b", b)):
        _C.check_gpu(name, x)
        _C.check_contig(name, x)
        _C.check_dtype(name, x, input.dtype)
        if x.dim() != 2:
            raise RuntimeError(f"Tensor {name} must have dimension number (2)")
    R = t.shape[1]
    why = wq16_lowrank_refusal(M, N, K, group_size, R)
    if why is not None:
        raise RuntimeError(f"wq16_lowrank_linear: {why}")
    _C.check_shape("t", t, M, R)
    _C.check_shape("b", b, N, R)
    if group_size is None:
        _check_vec("scale_weight", scale_weight, N, (torch.float32,))
        _check_vec("zp", zp, N, (torch.float32,))
    else:
        _check_group_params(K, N, group_size, scale_weight, zp)
    return _launch16("wanq_gemm_wq16_lowrank", (_C.ptr(input), _C.ptr(codes), _C.dt(input), 4 if w4 else 8, _C.ptr(scale_weight),
                                                _C.ptr(zp), int(group_size or 0), _C.ptr(t), _C.ptr(b), int(R)),
                     (input, codes, scale_weight, zp, t, b), bias, out_dtype or input.dtype, gelu, gate, residual, out, M, N, K)


def wq16_lowrank_refusal(M, N, K, group_size, R):
    """Why wanq_gemm_wq16_lowrank would refuse an [M, K] x [N, K] product with a rank-R branch (None = accepted): the rules of
    `wq16_linear_refusal` (group_size None or 0: the per-channel form), then R; see `fp_linear_refusal`."""
    why = wq16_linear_refusal(M, N, K, group_size or None)
    if why is not None:
        return why
    if not isinstance(R, int) or R < 64 or R > LOWRANK_MAX or R % 64:
        return f"R={R} must be 64, 128, 192 or 256"
    return None


# ---- group-wise weight scales on the int8 matrix cores ---------------------------------------------------------------
def w8a8_grouped_linear(input_i8, codes, scale_input, scale_weight, zp, group_size, bias=None, out_dtype=None, gelu=False, gate=None,
                        residual=None, out=None, w4=False):
    """y = epilogue(scale_input[m] * sum_g scale_weight[g, n] * input_i8[M, K_g] @ (codes[N, K_g] + zp[g, n])^T) on the int8 matrix
    cores (wanq_gemm_w8a8_grouped, csrc/gemm_i8_grouped.hip): `codes` int8 [N, K] (symmetric weights: zp must be None) or, with
    w4=True, uint8 [N, K/2] unsigned nibbles in the pack_w4 layout (zp = zero_point - 8, integer valued, codes + zp an int8);
    scale_weight and zp fp32 [K / group_size, N] (group-major).  Each group's int32 partial sum is folded into the result by one fp32
    fma with scale_weight[g, n], groups ascending; then y = fma(acc, scale_input[m], bias[n]) and the epilogue of `w8a8_linear`
    (`gelu`; gate fp32 [N] + residual [M, N] of the out dtype, which may alias `out`), one rounding to out_dtype (default fp16).
    group_size % 128 == 0 and K % group_size == 0.  Counted by the int8 timer (`set_timer`)."""
    _check_i8("input", input_i8)
    M, K = input_i8.shape
    _check_mat("codes", codes, torch.uint8 if w4 else torch.int8)
    N = codes.shape[0]
    _C.check_shape("codes", codes, N, K // 2 if w4 else K)
    why = w8a8_grouped_linear_refusal(M, N, K, group_size, 4 if w4 else 8, zp is None)
    if why is not None:
        raise RuntimeError(f"w8a8_grouped_linear: {why}")
    _check_group_params(K, N, group_size, scale_weight, zp)
    _check_vec("scale_input", scale_input, M)
    _check_vec("bias", bias, N)
    out_dtype = out_dtype or torch.float16
    epi = _epi_flags(gelu, gate, residual, M, N, out_dtype)
    out = _out_for(out, M, N, out_dtype, input_i8.device)
    _C.check_same_device(input_i8, codes, scale_input, scale_weight, zp, bias, gate, residual, out)
    with torch.cuda.device(input_i8.device), _timed(2 * M * N * K):
        _C.call("wanq_gemm_w8a8_grouped", _C.ptr(input_i8), _C.ptr(codes), 4 if w4 else 8, _C.ptr(scale_weight), _C.ptr(zp),
                int(group_size), _C.ptr(out), _C.dt(out_dtype), _C.ptr(scale_input), _C.dt(scale_input), _C.ptr(bias),
                _C.dt(bias) if bias is not None else _C.F32, _C.ptr(gate), _C.ptr(residual), epi, M, N, K, _C.stream())
    return out


def w8a8_grouped_linear_refusal(M, N, K, group_size, w_bits, sym):
    """Why wanq_gemm_w8a8_grouped would refuse an [M, K] x [N, K] product of `w_bits`-bit weights, symmetric (`sym`: no zero point) or
    not (None = accepted); see `fp_linear_refusal`."""
    if w_bits not in (4, 8):
        return f"w_bits={w_bits} must be 4 or 8"
    if w_bits == 8 and not sym:
        return "w_bits=8 takes symmetric weights only, zp must be None (c + zp does not fit int8)"
    why = _shape_refusal(M, N, K, None)
    if why is not None:
        return why
    if not isinstance(group_size, int) or group_size < 128 or group_size % 128:
        return f"group_size={group_size} must be a positive multiple of 128"
    if K < group_size or K % group_size:
        return f"K={K} must be a positive multiple of group_size={group_size}"
    return None


# ---- fp8 (OCP e4m3fn) activations x fp8 weights ------------------------------------------------------------------------
FP8_K_STEP = 64  # wanq_gemm_fp8's K multiple: one 16-byte fragment read per lane, half of the 128-deep fp8 MFMA


def fp8_linear(a_q, w_q, a_scale, w_scale, bias=None, out_dtype=None, gelu=False, gate=None, residual=None, out=None):
    """y = epilogue(a_scale[m] * w_scale[n] * a_q[M, K] @ w_q[N, K]^T) on the fp8 matrix cores (wanq_gemm_fp8, csrc/gemm_fp8.hip):
    a_q and w_q uint8, OCP e4m3fn bit patterns as `fused.quant_rows_fp8` writes them; a_scale fp32 [M], w_scale fp32 [N].  fp32
    accumulation, then y = fma(acc * a_scale[m], w_scale[n], bias[n]) and the epilogue of `fp_linear` (`gelu`; gate fp32 [N] +
    residual [M, N] of out_dtype, which may alias `out`), one rounding to out_dtype (default bf16).  K % 64 == 0, N % 8 == 0.  A
    row's bits do not depend on M or on where the row sits in the launch.  Not counted by the int8 timer (`set_timer`)."""
    for name, t in (("a_q", a_q), ("w_q", w_q)):
        _check_mat(name, t, torch.uint8)
    M, K = a_q.shape
    N = w_q.shape[0]
    _C.check_shape("w_q", w_q, N, K)
    why = fp8_linear_refusal(M, N, K)
    if why is not None:
        raise RuntimeError(f"fp8_linear: {why}")
    _check_vec("a_scale", a_scale, M, (torch.float32,))
    _check_vec("w_scale", w_scale, N, (torch.float32,))
    if a_scale is None or w_scale is None:
        raise RuntimeError("fp8_linear: a_scale and w_scale must be given")
    return _launch16("wanq_gemm_fp8", (_C.ptr(a_q), _C.ptr(w_q), _C.ptr(a_scale), _C.ptr(w_scale)), (a_q, w_q, a_scale, w_scale), bias,
                     out_dtype or torch.bfloat16, gelu, gate, residual, out, M, N, K)


def fp8_linear_refusal(M, N, K):
    """Why wanq_gemm_fp8 would refuse an [M, K] x [N, K] product (None = accepted): the shape rules of include/wanq_hip.h in the
    order the entry checks them; see `fp_linear_refusal`."""
    return _shape_refusal(M, N, K, FP8_K_STEP, bounded=True)


# ---- OCP MX: MXFP8 (e4m3) activations x MXFP8 / MXFP4 weights, E8M0 block scales ---------------------------------------------------
MX_K_STEP = 128  # wanq_gemm_mx's K multiple: one K-tile = one 128-deep MFMA = four blocks of 32


def mx_linear(a_q, w_q, a_scale, w_scale, w_fmt="mxfp8_e4m3", bias=None, out_dtype=None, gelu=False, gate=None, residual=None,
              out=None):
    """y = epilogue(sum over blocks of 2^(a_scale - 127) 2^(w_scale - 127) a_q @ w_q^T) on the block-scaled matrix cores (wanq_gemm_mx,
    csrc/gemm_mx.hip): a_q uint8 [M, K] e4m3 bytes; w_q uint8 [N, K] e4m3 bytes (w_fmt "mxfp8_e4m3") or [N, K / 2] packed e2m1 nibbles
    ("mxfp4_e2m1"); a_scale uint8 [M, K / 32], w_scale uint8 [N, K / 32], E8M0 bytes, all as `fused.quant_rows_mx` writes them.  fp32
    accumulation, y = acc + bias and the epilogue of `fp_linear` (`gelu`; gate fp32 [N] + residual [M, N] of out_dtype, which may alias
    `out`), one rounding to out_dtype (default bf16).  K % 128 == 0, N % 8 == 0.  A row's bits do not depend on M or on where the row
    sits in the launch.  Not counted by the int8 timer (`set_timer`)."""
    if w_fmt not in _C.MX_FMT:
        raise RuntimeError(f"mx_linear: w_fmt={w_fmt!r} must be one of {tuple(_C.MX_FMT)}")
    fp4 = _C.MX_FMT[w_fmt] == 1
    for name, t in (("a_q", a_q), ("w_q", w_q), ("a_scale", a_scale), ("w_scale", w_scale)):
        if t is None:
            raise RuntimeError(f"mx_linear: {name} must be given")
        _check_mat(name, t, torch.uint8)
    M, K = a_q.shape
    N = w_q.shape[0]
    why = mx_linear_refusal(M, N, K, w_fmt)
    if why is not None:
        raise RuntimeError(f"mx_linear: {why}")
    _C.check_shape("w_q", w_q, N, K // 2 if fp4 else K)
    _C.check_shape("a_scale", a_scale, M, K // 32)
    _C.check_shape("w_scale", w_scale, N, K // 32)
    return _launch16("wanq_gemm_mx", (_C.ptr(a_q), _C.ptr(w_q), _C.ptr(a_scale), _C.ptr(w_scale), _C.MX_FMT[w_fmt]),
                     (a_q, w_q, a_scale, w_scale), bias, out_dtype or torch.bfloat16, gelu, gate, residual, out, M, N, K)


def mx_linear_refusal(M, N, K, w_fmt="mxfp8_e4m3"):
    """Why wanq_gemm_mx would refuse an [M, K] x [N, K] product (None = accepted): the shape rules of include/wanq_hip.h in the order
    the entry checks them; see `fp_linear_refusal`."""
    if w_fmt not in _C.MX_FMT:
        return f"w_fmt={w_fmt!r} must be one of {tuple(_C.MX_FMT)}"
    return _shape_refusal(M, N, K, MX_K_STEP, bounded=True)


# ---- OCP MX W4A4: MXFP4 (e2m1) activations x MXFP4 weights, E8M0 block scales ---------------------------------------------------------
def mx4_linear(a_q, w_q, a_scale, w_scale, bias=None, out_dtype=None, gelu=False, gate=None, residual=None, out=None):
    """`mx_linear` with both operands 4 bits wide (wanq_gemm_mx4, csrc/gemm_mx.hip): a_q uint8 [M, K / 2] and w_q uint8 [N, K / 2], packed
    e2m1 nibbles, a_scale uint8 [M, K / 32], w_scale uint8 [N, K / 32], all as `fused.quant_rows_mx(fmt="mxfp4_e2m1")` writes them (both
    sides with `had32`, or neither).  The accumulation, epilogue, shape rules (K % 128 == 0, N % 8 == 0) and determinism are
    `mx_linear`'s.  Not counted by the int8 timer (`set_timer`)."""
    for name, t in (("a_q", a_q), ("w_q", w_q), ("a_scale", a_scale), ("w_scale", w_scale)):
        if t is None:
            raise RuntimeError(f"mx4_linear: {name} must be given")
        _check_mat(name, t, torch.uint8)
    M, K = a_q.shape[0], a_q.shape[1] * 2
    N = w_q.shape[0]
    why = mx4_linear_refusal(M, N, K)
    if why is not None:
        raise RuntimeError(f"mx4_linear: {why}")
    _C.check_shape("w_q", w_q, N, K // 2)
    _C.check_shape("a_scale", a_scale, M, K // 32)
    _C.check_shape("w_scale", w_scale, N, K // 32)
    return _launch16("wanq_gemm_mx4", (_C.ptr(a_q), _C.ptr(w_q), _C.ptr(a_scale), _C.ptr(w_scale)), (a_q, w_q, a_scale, w_scale), bias,
                     out_dtype or torch.bfloat16, gelu, gate, residual, out, M, N, K)


def mx4_linear_refusal(M, N, K):
    """Why wanq_gemm_mx4 would refuse an [M, K] x [N, K] product (None = accepted): the shape rules of include/wanq_hip.h in the order
    the entry checks them; see `fp_linear_refusal`."""
    return _shape_refusal(M, N, K, MX_K_STEP, bounded=True)


# ---- OCP MX W6A6 / W4A6: MXFP6 (e2m3) activations x MXFP6 / MXFP4 weights, E8M0 block scales ------------------------------------------
def mx6_linear(a_q, w_q, a_scale, w_scale, w_fmt="mxfp6_e2m3fn", bias=None, out_dtype=None, gelu=False, gate=None, residual=None,
               out=None):
    """`mx_linear` with e2m3 activations and no operand 8 bits wide (wanq_gemm_mx6, csrc/gemm_mx.hip): a_q uint8 [M, 3 K / 4] packed
    e2m3 codes; w_q uint8 [N, 3 K / 4] packed e2m3 codes (w_fmt "mxfp6_e2m3fn") or [N, K / 2] packed e2m1 nibbles ("mxfp4_e2m1");
    a_scale uint8 [M, K / 32], w_scale uint8 [N, K / 32], all as `fused.quant_rows_mx` writes them.  The accumulation, epilogue, shape
    rules (K % 128 == 0, N % 8 == 0) and determinism are `mx_linear`'s.  Not counted by the int8 timer (`set_timer`)."""
    if w_fmt not in _C.MX6_FMT:
        raise RuntimeError(f"mx6_linear: w_fmt={w_fmt!r} must be one of {tuple(_C.MX6_FMT)}")
    for name, t in (("a_q", a_q), ("w_q", w_q), ("a_scale", a_scale), ("w_scale", w_scale)):
        if t is None:
            raise RuntimeError(f"mx6_linear: {name} must be given")
        _check_mat(name, t, torch.uint8)
    if a_q.shape[1] % 3:
        raise RuntimeError(f"mx6_linear: a_q has {a_q.shape[1]} bytes per row, not 3 K / 4 of any K")
    M, K = a_q.shape[0], a_q.shape[1] // 3 * 4
    N = w_q.shape[0]
    why = mx6_linear_refusal(M, N, K, w_fmt)
    if why is not None:
        raise RuntimeError(f"mx6_linear: {why}")
    _C.check_shape("w_q", w_q, N, K // 2 if _C.MX6_FMT[w_fmt] == 1 else K // 4 * 3)
    _C.check_shape("a_scale", a_scale, M, K // 32)
    _C.check_shape("w_scale", w_scale, N, K // 32)
    return _launch16("wanq_gemm_mx6", (_C.ptr(a_q), _C.ptr(w_q), _C.ptr(a_scale), _C.ptr(w_scale), _C.MX6_FMT[w_fmt]),
                     (a_q, w_q, a_scale, w_scale), bias, out_dtype or torch.bfloat16, gelu, gate, residual, out, M, N, K)


def mx6_linear_refusal(M, N, K, w_fmt="mxfp6_e2m3fn"):
    """Why wanq_gemm_mx6 would refuse an [M, K] x [N, K] product (None = accepted): the shape rules of include/wanq_hip.h in the order
    the entry checks them; see `fp_linear_refusal`."""
    if w_fmt not in _C.MX6_FMT:
        return f"w_fmt={w_fmt!r} must be one of {tuple(_C.MX6_FMT)}"
    return _shape_refusal(M, N, K, MX_K_STEP, bounded=True)
