/*
 * wanq_hip.h -- C ABI of libwanq_hip.so: the MI355X (gfx950) hot path of the quantized Wan2.1 DiT.
 *
 * This is the drop-in boundary.  The reference has no C ABI: its "ABI" is two pybind11 modules
 * taking torch::Tensor (ViDiT-Q/kernels/csrc/{fused,qgemm}/pybind.cpp).  Every entry point below
 * names the reference function(s) it replaces; the Python package
 * wan2.1-quantization_amd/viditq_extension re-exports them under the reference's own names and
 * argument order through ctypes.
 *
 * Conventions
 *   - plain device pointers + sizes, no torch types; `stream` is a hipStream_t passed as void*
 *     (NULL = the legacy default stream).  Calls only enqueue work; nothing synchronises.
 *   - return value 0 = enqueued; non-zero = refused (WANQ_E_*), nothing enqueued, message from
 *     wanq_last_error().  Shape/dtype errors are reported, never asserted (the reference aborts the
 *     process on tile-divisibility violations: w8a8_gemm_cuda.cu:678-680).
 *   - row-major contiguous tensors; activations [rows, cols], weights [N, K] (nn.Linear layout).
 *   - dtype codes WANQ_F16/BF16/F32 for floating tensors; per-token / per-channel vectors
 *     (scale, sum, bias ...) carry their own dtype code so both the reference's fp16 buffers
 *     (K/viditq_extension/nn/base.py:12-26) and fp32 buffers (simulation-path accuracy) work.
 *   - integer results (int8 codes, int32 accumulators) are bit-exact w.r.t. oracle/; see DESIGN.md.
 */
#ifndef WANQ_HIP_H
#define WANQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { WANQ_F16 = 0, WANQ_BF16 = 1, WANQ_F32 = 2, WANQ_I32 = 3, WANQ_I16 = 4 };

enum {
  WANQ_OK = 0,
  WANQ_E_ARG = 1,     /* bad pointer / dtype / flag combination */
  WANQ_E_SHAPE = 2,   /* unsupported shape (message says which rule) */
  WANQ_E_LAUNCH = 3   /* hipGetLastError() after launch was not hipSuccess */
};

/* Last refusal message of the calling thread ("" if none).  Never NULL. */
const char* wanq_last_error(void);
/* Version of this ABI (bumped on any signature change). */
int wanq_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Per-token dynamic int8 quantisation (+ dequantised row sum).
 *   q[r,c]   = clamp(rne(x[r,c] / scale_r), -128, 127),  scale_r = max(absmax_r / 127, 1e-6)
 *   sum[r]   = scale_r * sum_c q[r,c]                       (sum may be NULL)
 * act: 0 = identity, 1 = tanh-GELU applied to x first.
 * static_amax != 0: `scale` is an INPUT holding absmax_r (reference quant_sum_static reads it so).
 * Replaces fused.quant_sum / quant_sum_static / gelu_quant_sum
 *   (ViDiT-Q/kernels/csrc/fused/fused.cu:30-232, hosts :524-706) and is bit-identical to
 *   DynamicQuantizer.quantize (quant_utils/qdiff/base/base_quantizer.py:101-157) for any cols % 8 == 0
 *   (the reference needs cols % 128 == 0 and cols <= 8192). */
int wanq_quant_rows(const void* x, int x_dtype, int8_t* q, void* scale, void* sum, int vec_dtype,
                    int64_t rows, int cols, int act, int static_amax, void* stream);

/* The same per-token dynamic symmetric quantiser at a narrower range (codes still int8, the GEMMs are unchanged):
 *   q[r,c] = rne(x[r,c] / scale_r),  scale_r = max(absmax_r / n_levels, floor),  n_levels = 2^(b-1) - 1 in [1, 127]
 * floor = 0: no floor -- a row of zeros gets scale 0 and codes 0 (the reference divides 0 by 0 there and returns NaN).
 * Replaces MixedPrecisionDynamicQuantizer.quantize, symmetric branch, at the active entry of its bit-width list
 *   (quant_utils/qdiff/base/mixed_precision_quantizer.py:135-146,171-175: no eps floor) and DynamicQuantizer.quantize for
 *   n_bits < 8 (base/base_quantizer.py:116-128,154-157: floor 1e-6).  Bit-identical codes and scales. */
int wanq_quant_rows_levels(const void* x, int x_dtype, int8_t* q, void* scale, void* sum, int vec_dtype,
                           int64_t rows, int cols, int n_levels, float floor, void* stream);

/* Per-row dynamic OCP fp8 (e4m3fn) quantisation: the activation quantiser (one row = one token) and, once at conversion time, the
 * weight quantiser (a weight [N, K] goes through it as rows = N: one row = one output channel) of wanq_gemm_fp8.
 *   scale_r = max(absmax_r / 448, 1e-6)                          (448: the largest e4m3fn value; the floor of wanq_quant_rows)
 *   q[r,c]  = e4m3fn_rne(clamp(x[r,c] / scale_r, -448, 448))     (true fp32 division; ONE rounding, fp32 -> e4m3fn, to nearest even,
 *                                                                 subnormal codes kept, made by v_cvt_pk_fp8_f32 behind the clamp)
 * x: F16 | BF16 | F32 [rows, cols], cols % 8 == 0, cols <= 16384.  q: one byte per element, OCP e4m3fn bit patterns (S.EEEE.MMM, bias
 * 7, no infinities, 0x7f / 0xff NaN) -- NOT the e4m3fnuz format of gfx942.  scale: fp32 [rows].  There is no `sum` output: symmetric
 * weights need none.  act: 0 = identity, 1 = tanh-GELU applied to x first (the gelu_tanh_fast_f32 of wanq_quant_rows).
 * A row of zeros gets scale 1e-6 and codes 0.  -0 and negative values that round to zero give the code 0x80.
 * Non-finite inputs: fmax drops NaN, so a NaN element does not enter absmax_r and its own code is unspecified (the clamp's result
 * for a NaN); a row holding +-inf gets scale inf, codes 0 for its finite elements and unspecified codes for the infinite ones
 * (inf / inf).  Nothing is trapped; no test pins these.
 * Bit-identical to the torch expression (x / s).clamp(-448, 448).to(torch.float8_e4m3fn) with s = (x.abs().amax(-1) / 448).clamp(1e-6).
 * No reference counterpart: the reference's Linear formats are integer ones. */
int wanq_quant_rows_fp8(const void* x, int x_dtype, uint8_t* q, float* scale, int64_t rows, int cols, int act, void* stream);

/* OCP Microscaling (MX) block quantisation: one E8M0 power-of-two scale per block of 32 consecutive columns.  The activation
 * quantiser (fmt e4m3) and, once at conversion time, the weight quantiser (a weight [N, K] goes through it as rows = N, either
 * format) of wanq_gemm_mx.  For row r and block b (columns 32 b .. 32 b + 31):
 *   amax = max |x| over the block;  E = the biased fp32 exponent field of amax, (bits >> 23) & 0xff (0 for amax = 0 and for fp32
 *          subnormals)
 *   s    = clamp(E - emax, 0, 254)          scale byte; the block scale is 2^(s - 127); emax = 8 (e4m3), 2 (e2m1); 255, the E8M0
 *                                           NaN, is never written
 *   c    = rne_fmt(clamp(ldexp(x, 127 - s), -max, max))     max = 448 (e4m3), 6 (e2m1); ONE rounding, to nearest even, subnormal
 *                                           codes kept
 * fmt: WANQ_MX_E4M3 -- q [rows, cols] bytes, the OCP e4m3fn bit patterns of wanq_quant_rows_fp8;  WANQ_MX_E2M1 -- q [rows, cols / 2]
 * bytes, two 4-bit codes per byte, element k in byte k / 2 with even k in the low nibble; a code is the sign in bit 3 and the
 * magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6} in bits 0-2.  scale_u8: uint8 [rows, cols / 32], row-major.
 * x: F16 | BF16 | F32 [rows, cols], cols % 32 == 0, cols <= 16384.  act: 0 = identity, 1 = tanh-GELU applied to x first (the
 * gelu_tanh_fast_f32 of wanq_quant_rows).  -0 and negative values that round to zero keep their sign bit.
 * Non-finite inputs: fmax drops NaN, so a NaN element does not enter amax and its own code is unspecified; a block holding +-inf
 * gets s = 255 - emax and unspecified codes for the infinite elements.  Nothing is trapped; no test pins these.
 * Bit-identical to the host expression mx_quant_rows of qdiff/base/base_quantizer.py.
 * No reference counterpart: the reference's Linear formats are integer ones. */
enum { WANQ_MX_E4M3 = 0, WANQ_MX_E2M1 = 1, WANQ_MX_E2M3 = 2 };   /* E2M3: wanq_quant_rows_mx6 / wanq_gemm_mx6 only */
int wanq_quant_rows_mx(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int fmt, int act,
                       void* stream);

/* wanq_quant_rows_mx behind a block Hadamard rotation: the same arguments and rules (both fmt values), and after the optional GELU and
 * before the block maximum every block of 32 columns is replaced by its UNNORMALISED Sylvester-Hadamard transform x H, H[i][j] =
 * (-1)^popcount(i & j).  Computed in fp32 by five butterfly stages in the order h = 1, 2, 4, 8, 16: for every pair (i, i + h) with bit
 * h of i clear, (x_i, x_{i+h}) <- (x_i + x_{i+h}, x_i - x_{i+h}).  Additions and subtractions only, one rounding each, so the host
 * restatement in the same order (mx_hadamard32_host, and mx_quant_rows_host(had32=True), qdiff/base/base_quantizer.py) is bit-equal.
 * H is symmetric and H H = 32 I: a layer whose activations go through this entry quantises its weight as w / 32 through it too,
 * (x H)(w H / 32)^T = x w^T, and the GEMM needs no inverse rotation (config `mx: {block_hadamard: True}`).
 * No reference counterpart. */
int wanq_quant_rows_mx_had32(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int fmt, int act,
                             void* stream);

/* OCP MXFP6 (e2m3) block quantisation: wanq_quant_rows_mx's row frame, GELU option, block maximum and argument rules, to 6-bit codes.
 * The format (WANQ_MX_E2M3; config name mxfp6_e2m3fn: finite only), defined here and as a host expression in
 * qdiff/base/base_quantizer.py:
 *   code  6 bits: sign in bit 5, E in bits 3-4 (bias 1), M in bits 0-2.  E = 0: M / 8;  E > 0: 2^(E - 1) (1 + M / 8).  Largest
 *         magnitude 7.5; no inf, no NaN; the magnitude codes 0-31 ascend with the value.
 *   s     = clamp(E(amax) - 2, 0, 254): emax 2 as for e2m1, so a row's scale bytes are those wanq_quant_rows_mx(fmt E2M1) writes.
 *   c     : t = clamp(ldexp(x, 127 - s), -7.5, 7.5);  quantum q = 1/8 for |t| < 2, 1/4 for |t| < 4, else 1/2;  |c| = rne(|t| / q) q,
 *           ONE rounding, ties to the even code.  -0 and negative values that round to zero keep their sign bit.
 *   q     [rows, 3 cols / 4] bytes: block b of a row is bytes 24 b .. 24 b + 23, element j of the block bits 6 j .. 6 j + 5 of that
 *         192-bit little-endian string.  This is the order in which v_mfma_scale_f32_16x16x128_f8f6f4 takes a 6-bit operand's six
 *         registers (one block per lane group; probes A of tests/test_gpu_mx6.py), so wanq_gemm_mx6 never re-packs anything.
 * scale_u8: uint8 [rows, cols / 32].  x, cols, act, alignment of q (16 bytes) and the non-finite behaviour: wanq_quant_rows_mx's.
 * Bit-identical to the host expression mx_quant_rows_host(fmt "mxfp6_e2m3fn").  No reference counterpart. */
int wanq_quant_rows_mx6(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int act, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (no bias, optional gamma) -> optional adaLN modulate -> fp output OR int8 quant (+sum).
 *   y = (x - mean) * rstd * gamma;  y = y * (1 + mscale[b]) + mshift[b]   (b = row / rows_per_batch)
 *   out_fp != NULL : write y in out_dtype.      q != NULL : quantise y like wanq_quant_rows.
 * gamma / mshift / mscale may be NULL (identity).  mod_stride = elements between batches.
 * Statistics and modulation are fp32 (simulation-path semantics, Wan model.py:327), not half2.
 * Replaces fused.layernorm_nobias, layernorm_nobias_quant_nosum_fuse, layernorm_nobias_quant_sum_fuse,
 *   layernorm_nobias_t2i_fuse, layernorm_nobias_t2i_quant_sum_fuse
 *   (ViDiT-Q/kernels/csrc/fused/fused.cu:234-380, hosts :485-522,:708-915).  Any cols % 8 == 0 up to
 *   16384 (the reference: cols/4 <= 1024 threads). */
int wanq_layernorm_rows(const void* x, int x_dtype, const void* gamma, const void* mshift,
                        const void* mscale, int mod_dtype, int64_t mod_stride, int64_t rows_per_batch,
                        float eps, void* out_fp, int out_dtype, int8_t* q, void* scale, void* sum,
                        int vec_dtype, int64_t rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * out = y * gate[b] + residual   (fp32 arithmetic; each tensor has its own dtype).
 * Replaces fused.gate_residual_fuse (fused.cu:382-483, host :917-961). */
int wanq_gate_residual(const void* y, int y_dtype, const void* gate, int gate_dtype, int64_t gate_stride,
                       const void* residual, int res_dtype, void* out, int out_dtype, int64_t rows,
                       int cols, int64_t rows_per_batch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * W8A8 GEMM on int8 MFMA with fused dequant epilogue:
 *   acc[m,n] = sum_k a[m,k] * w[n,k]                                  (int32, exact)
 *   y        = acc*sa[m]*sw[n] (+ asum[m]*zp[n]*sw[n]) (+ bias[n])     (fp32, this order)
 *   y        = gelu_tanh(y)                     if WANQ_EPI_GELU
 *   y        = residual[m,n] + y * gate[n]      if WANQ_EPI_GATE_RES  (gate fp32[N], residual/out same dtype)
 *   out      = cast(y)  to out_dtype;  out_dtype == WANQ_I32 stores acc (no scales read).
 * sa/asum: per-token, dtype tok_dtype (F16|F32).  sw/bias: per-channel, dtype ch_dtype (F16|F32).
 * zp: zp_dtype WANQ_I16 (reference buffer) or WANQ_F32; NULL = symmetric weights.  bias may be NULL.
 * Any M >= 1 (ragged last tile handled in-kernel, no host padding: replaces pad_to_multiple_2d,
 * wan/quant_wanx_cuda.py:313-328); N % 8 == 0; K % 16 == 0.
 * Replaces qgemm.w8a8_of16_bias_weight_asym / _sym / w8a8_o32 / w8a8_of16_nobias_weight_sym_qserve
 *   (ViDiT-Q/kernels/csrc/qgemm/w8a8/w8a8_gemm_cuda.cu:624-838,
 *    ViDiT-Q/kernels/csrc/qgemm/w8a8/w8a8_gemm_cuda_qserve.cu:527-611). */
enum { WANQ_EPI_GELU = 1, WANQ_EPI_GATE_RES = 2 };
int wanq_gemm_w8a8(const int8_t* a, const int8_t* w, void* out, int out_dtype, const void* sa,
                   const void* asum, int tok_dtype, const void* sw, const void* bias, int ch_dtype,
                   const void* zp, int zp_dtype, const float* gate, const void* residual, int epi_flags,
                   int64_t M, int N, int K, void* stream);

/* Diagnostic: which int8 GEMM kernel wanq_gemm_w8a8 / wanq_gemm_w4a8 launch.  0 = automatic (default: the ping-pong persistent
 * kernel where a problem is eligible, else the persistent kernel, else the 128 x 128 kernel), 1 = always the 128 x 128
 * kernel, 2 = never the ping-pong kernel.  Process-wide; returns the previous setting (or -1 for a bad value, nothing changed).
 * Accumulators are bit-identical across the three kernels and so are the outputs of the two persistent ones; the 128 x 128
 * kernel sums the epilogue terms in another order (one unit of the output type; tests/test_gpu_gemm.py).  No reference counterpart. */
int wanq_gemm_select_kernel(int which);

/* ------------------------------------------------------------------------------------------------
 * bf16 / fp16 GEMM on v_mfma_f32_16x16x32_{bf16,f16} with the epilogue of wanq_gemm_w8a8:
 *   y   = sum_k a[m,k] * w[n,k]                     (fp32 accumulation; a, w both of `dtype`: WANQ_BF16 or WANQ_F16)
 *   y   = y + bias[n]                               (bias may be NULL; bias_dtype F16 | BF16 | F32)
 *   y   = gelu_tanh(y)                              if WANQ_EPI_GELU
 *   y   = residual[m,n] + y * gate[n]               if WANQ_EPI_GATE_RES  (gate fp32[N], residual of out_dtype; out may alias it)
 *   out = cast(y) to out_dtype (F16 | BF16 | F32): one rounding, all arithmetic above in fp32.
 * Any M >= 1 (ragged last tile in-kernel, no host padding); N % 8 == 0; K % 32 == 0; a, w, out and residual 16-byte aligned,
 * gate and bias aligned to 4 elements.  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).
 * Determinism: the fp32 summation order of element (m, n) depends on K only -- not on M, on the row's position in the launch or
 * on the workgroup that ran it (one kernel form, no split-K), so a row gives the same bits in any launch, and repeated calls are
 * bit-identical.
 * Replaces the nn.Linear layers the reference's kernel-mode block keeps in floating point: the FFN with its separate GELU
 * (ViDiT-Q/examples/Wan2.1/wan/quant_wanx_cuda.py:162-164) and the attention output projection (:360), whose
 * gate + residual the reference applies in a separate pass. */
int wanq_gemm_bf16(const void* a, const void* w, int dtype, void* out, int out_dtype, const void* bias, int bias_dtype,
                   const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight-only quantised GEMM (W8A16 / W4A16): 16-bit activations against integer weight codes, on the matrix cores and with the
 * epilogue of wanq_gemm_bf16:
 *   acc = sum_k a[m,k] * (c[n,k] + zp[n])           (a of `dtype`: WANQ_BF16 or WANQ_F16; fp32 accumulation)
 *   y   = acc * sw[n] + bias[n]                     (one fp32 fma; sw fp32[N]; zp fp32[N] or NULL = 0; bias may be NULL)
 *   y   = gelu_tanh(y)                              if WANQ_EPI_GELU
 *   y   = residual[m,n] + y * gate[n]               if WANQ_EPI_GATE_RES
 *   out = cast(y) to out_dtype (F16 | BF16 | F32): one rounding.
 * w_bits = 8: c is int8 [N, K].  w_bits = 4: c is the unsigned nibbles of wanq_pack_w4's layout ([N, K/2] bytes) and zp follows
 * the W4A8 convention, zero_point - 8.  The codes become 16-bit MFMA fragments in registers; no dequantised weight is written.
 * Exactness: c + zp is an integer with |c + zp| <= 255 for every StaticQuantizer output (8-bit asymmetric: c in [-128, 127], zp in
 * [-127, 128]; 4-bit: 0..15), exact in bf16 (8 significant bits) and in fp16, so the weight reaches the matrix cores without any
 * rounding and each product a (c + zp) is exact in fp32; sw is applied once, in fp32.  zp must be integer valued.
 * Any M >= 1; N % 8 == 0; K % 64 == 0; a, w, out, residual, sw and zp 16-byte aligned, gate and bias aligned to 4 elements.
 * Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).
 * Determinism: wanq_gemm_bf16's summation order -- with sw = 1 the output is bit-equal to wanq_gemm_bf16 on (c + zp) cast to `dtype`;
 * a row gives the same bits in any launch.
 * Replaces QuantizedLinear.forward with a weight quantiser and a_quantizer = None, F.linear(x, (c + zp) * delta, bias)
 *   (ViDiT-Q/quant_utils/qdiff/base/quant_layer.py:68-72), which under autocast rounds (c + zp) * delta to bf16 first. */
int wanq_gemm_wq16(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp, void* out,
                   int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags,
                   int64_t M, int N, int K, void* stream);

/* Group-wise form of wanq_gemm_wq16 (the weight scales of AWQ / GPTQ-style W4A16): one scale and one zero point per output channel
 * and per group of `group_size` input channels, sw and zp fp32 [K / group_size][N] (group-major; zp may be NULL = 0):
 *   part_g = sum_{k in group g} a[m,k] * (c[n,k] + zp[g,n])     (fp32, on the matrix cores, wanq_gemm_wq16's order within a group)
 *   acc    = fma(part_g, sw[g,n], acc)                          (g ascending from acc = 0: one fp32 fma per group)
 *   y      = acc + bias[n];  GELU, gate + residual and the one rounding to out_dtype as above.
 * a, w (int8 [N, K] or packed nibbles [N, K/2], zp = zero_point - 8), out, bias, gate, residual and epi_flags as for wanq_gemm_wq16.
 * The weight operand c + zp reaches the matrix cores unrounded and the scale is applied in fp32 only; no dequantised weight is
 * written.  zp must be integer valued.  With group_size == K and bias NULL the output is bit-equal to wanq_gemm_wq16's.
 * group_size % 64 == 0, K % group_size == 0, N % 8 == 0, sw and zp 16-byte aligned; every other rule as for wanq_gemm_wq16.
 * Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).  A row gives the same bits in any launch.
 * Group-wise weight quantisation is the reference's StaticQuantizer applied to w.view(N K / g, g): its quantisers are written for
 * [N_group, -1] input (ViDiT-Q/quant_utils/qdiff/base/base_quantizer.py:72). */
int wanq_gemm_wq16_grouped(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp, int group_size,
                           void* out, int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual,
                           int epi_flags, int64_t M, int N, int K, void* stream);

/* wanq_gemm_wq16 / wanq_gemm_wq16_grouped with a 16-bit low-rank side branch, y = x W^T + (x A^T) B^T: the low-rank compensation of
 * the quantisation error (LoRC: B A the best rank-r approximation of W - W^) and LoRA adapters on a quantised Linear.  The caller
 * computes t = x A^T (wanq_gemm_bf16 with N = R, rounded once to `dtype`); this entry adds t B^T INSIDE the GEMM, before GELU and
 * gate + residual:
 *   y0[m,n] = exactly what wanq_gemm_wq16 (group_size == 0: sw, zp fp32 [N]; fma(acc, sw[n], bias[n])) or wanq_gemm_wq16_grouped
 *             (any other group_size: that entry's rules and [K / group_size][N] layouts; acc + bias[n]) computes before GELU
 *   lr[m,n] = sum_r t[m,r] * b[n,r]      (fp32, on the 16-bit matrix cores of `dtype`, 64-deep r-tiles ascending, in an accumulator
 *                                         set of its own: bit-equal to wanq_gemm_bf16(t, b) with an fp32 output)
 *   y       = y0 + lr                    (one fp32 add);  GELU, gate + residual and the one rounding to out_dtype as above.
 * t is [M, R] and b is [N, R], both of `dtype`, row-major and 16-byte aligned.  R % 64 == 0 and 64 <= R <= 256: a smaller rank is
 * zero padded by the caller, and a zero column of t or b contributes exactly 0.  With t = 0 or b = 0 and finite operands the output
 * is bit-equal to the entry without the branch (y0 + 0).  Every other argument and rule as for the two entries above; rows past M
 * and channels past N are clamped in-kernel as there.  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the
 * rule).  Determinism: the summation order of y0 is that of the entry without the branch and that of lr depends on R only, so a
 * row gives the same bits in any launch and repeated calls are bit-identical. */
int wanq_gemm_wq16_lowrank(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp, int group_size,
                           const void* t, const void* b, int R, void* out, int out_dtype, const void* bias, int bias_dtype,
                           const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PTQ calibration reduction: running per-channel absmax over tokens,
 *   colmax[c] = max(colmax[c], max_r |x[r,c]|)        (colmax fp32[cols], caller zero-initialises)
 * Replaces SaveActivationHook.__call__ default branch
 *   (ViDiT-Q/examples/Wan2.1/get_calib_data_wanx.py:262-267) -- and, because ptq takes .max(dim=0)
 *   over the stacked calls (ptq_wanx.py:336), the stack itself. */
int wanq_col_absmax(const void* x, int x_dtype, float* colmax, int64_t rows, int cols, void* stream);

/* v fake-quantisation of the reference's quantized attention (ViDiT-Q/examples/Wan2.1/models/quant_opensora.py:438-440:
 * DynamicQuantizer over all tokens for every (head, channel)), on the token-major [rows, cols] tensor: per COLUMN c
 *   delta_c = max(colmax[c] / (2^(b-1) - 1), 1e-6),   out = clamp(rne(x / delta_c), -2^(b-1), 2^(b-1) - 1) * delta_c.
 * colmax: fp32 [cols] from wanq_col_absmax over the same rows.  In place (out == x) is allowed. */
int wanq_fake_quant_cols(const void* x, int x_dtype, const float* colmax, void* out, int out_dtype, int n_bits,
                         int64_t rows, int cols, void* stream);

/* Fake-quantisation with a PRECOMPUTED delta of x's own shape, elementwise over n values (n % 8 == 0):
 *   d = max(delta, 1e-6);  plain (bits == NULL): d' = d / (2^b - 1), out = clamp(rne(x / d'), 0, 2^b - 1) * d'
 *     (everything at or below zero, rne(x / d') = -0.0 included, gives +0.0: the clamp's lower bound is the result)
 *   bits != NULL (int32 per element): d' = d / (2^bits - 1), out = min(rne(x / d'), 2^bits - 1) * d', 0 bits -> 0.
 * Replaces DynamicQuantizer.forward_with_quant_params (quant_utils/qdiff/base/base_quantizer.py:164-206: the fake-quant step of
 *   the reference's block-wise attention-map quantisers, symmetric quantisers only).  Bit-identical for fp32 x.  In place allowed. */
int wanq_fake_quant_with_delta(const void* x, int x_dtype, const float* delta, const int32_t* bits, void* out, int out_dtype,
                               int n_bits, int64_t n, void* stream);

/* Per-row min / max / absmax of a weight matrix (StaticQuantizer.init_quant_params statistics,
 *   quant_utils/qdiff/base/base_quantizer.py:70-90).  Any of the outputs may be NULL. */
int wanq_row_minmax(const void* w, int w_dtype, float* row_min, float* row_max, float* row_absmax,
                    int64_t rows, int cols, void* stream);

/* Static per-output-channel weight quantisation with given params (fp32 [rows]):
 *   q = clamp(rne(w/delta) - zp, qmin, qmax)  -> fake-quant (q+zp)*delta -> fp32, and/or int8 codes (q saturated to
 *   [-128,127] on top of [qmin,qmax]: the reference's own clamp is looser than the bit-width).
 *   (base_quantizer.py:56-68; export: wan/quant_wanx_cuda.py:39-53).  q8 / deq may be NULL. */
int wanq_weight_quant(const void* w, int w_dtype, const float* delta, const float* zp, int qmin, int qmax,
                      int8_t* q8, float* deq, int64_t rows, int cols, void* stream);

/* The GPTQ weight solver (Frantar et al., 2022; qdiff/base/gptq.py drives it; csrc/gptq.hip): the grid of wanq_weight_quant is kept,
 * only the choice of each code changes, so that the layer's output error on the calibration activations is minimised.
 *   w      fp32 [N, K], row stride w_stride (elements): the working copy, updated in place
 *   u      fp32 [K, K], row stride u_stride: the UPPER Cholesky factor of H^-1 (H = X^T X of the layer's calibration inputs)
 *   delta, zp  fp32 [N, K / group_size] as StaticQuantizer holds them; group_size = 0: fp32 [N], one per row
 *   qmin, qmax the range of the STORED codes (the quantiser's [-n-1, n] intersected with the bit-width's [-2^(b-1), 2^(b-1)-1],
 *              SURVEY D9), so that the error pushed on is the error of what the checkpoint keeps
 *   codes  int8 [N, K] (row stride K);  err  fp32 [N, cols] (row stride cols)
 * wanq_gptq_block, for j = c0 .. c0+cols-1 in order (1 <= cols <= 128), every row on its own:
 *   q = clamp(rne(w[j] / delta) - zp, qmin, qmax);  w_hat = (q + zp) delta;  codes[j] = q;  e = (w[j] - w_hat) / u[j,j];
 *   err[n, j-c0] = e;  w[k] = w[k] - e u[j,k] for c0+cols > k > j;  w[j] = w_hat.
 * wanq_gptq_propagate:  w[n, k] -= sum_{i < cols} err[n, i] u[c0+i, k]  for k >= c0+cols, the sum over i ascending from 0.
 * Every operation is one fp32 IEEE operation, rounded once, never contracted into an fma (true divisions): a fixed function of
 * the operands, bit-equal to the host model gptq_solve_host.  Columns before c0 are not touched.
 * Refused before any launch (WANQ_E_ARG / WANQ_E_SHAPE, the message names the rule): NULL pointers, cols outside 1..128,
 * c0 + cols > K, strides below K, a range that is not an int8 range, a group_size that does not divide K, an odd group_size or c0
 * with a group_size (the kernel keeps two neighbouring columns per lane: a pair must lie in one group).  N = 0: WANQ_OK. */
int wanq_gptq_block(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* delta, const float* zp,
                    int group_size, int qmin, int qmax, int8_t* codes, float* err, int64_t N, int K, int c0, int cols, void* stream);
int wanq_gptq_propagate(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* err,
                        int64_t N, int K, int c0, int cols, void* stream);

/* wanq_gptq_block with a group per COLUMN (gptq.act_order: the solver visits the input channels in order of descending diag H, so
 * the columns of w / u are a permutation of the channels and neighbouring columns lie in arbitrary groups):
 *   delta, zp  fp32 [N, G] (row stride G);  g_idx  int32 [K] in device memory: column j is quantised on delta[n, g_idx[j]],
 *              zp[n, g_idx[j]].  The kernel clamps every index into 0 .. G-1, so a bad map never reads outside delta / zp.
 * Every other operand, the steps and their arithmetic are wanq_gptq_block's, operation for operation (one fp32 IEEE operation each,
 * no fma, true divisions, the error pushed on in ascending column order): with g_idx[j] = j / group_size the two entries agree bit
 * for bit, and both are bit-equal to the host model gptq_block_host on the same map.  There is no evenness rule on c0 or on the
 * groups.  wanq_gptq_propagate does not depend on groups and serves both.
 * Refused before any launch (WANQ_E_ARG / WANQ_E_SHAPE, the message names the rule): NULL pointers (g_idx among them), G < 1,
 * cols outside 1..128, c0 + cols > K, strides below K, a range that is not an int8 range.  N = 0: WANQ_OK. */
int wanq_gptq_block_gidx(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* delta, const float* zp,
                         const int32_t* g_idx, int G, int qmin, int qmax, int8_t* codes, float* err, int64_t N, int K, int c0,
                         int cols, void* stream);

/* H += x^T x in fp32, in place: the Hessian of a Linear's calibration inputs (csrc/gram.hip).
 *   x  row-major [rows, C], WANQ_BF16 or WANQ_F16, read as it lies (no transposed copy);  H  fp32 [C, C], row stride C.
 * The contraction runs over the rows on v_mfma_f32_16x16x32_{bf16,f16}, 32 rows a step from row 0 upwards; rows past `rows` in the
 * last step enter as exact zeros.  Only the 128 x 128 tile pairs (ti <= tj) are computed: an element's sum s is added to H[i, j]
 * and, off the diagonal, the same s to H[j, i] (inside a diagonal tile only i <= j is taken), so a symmetric H stays symmetric
 * bit for bit by construction.  The summation order of an element depends on `rows` alone: not on C, on the element's place or on
 * where x lies.
 * Refused before any launch: NULL x or H, x_dtype other than bf16 / fp16, rows < 0, C < 8 or C % 8 != 0, x or H not 16-byte
 * aligned.  rows == 0: WANQ_OK, H untouched. */
int wanq_gram_accumulate(const void* x, int x_dtype, float* H, int64_t rows, int C, void* stream);

/* Reference-format int8 export of a weight matrix, all arithmetic in HALF precision as the reference does it:
 *   q8 = clamp( round( f16(w) / delta ) - zp, -128, 127 )   delta, zp: fp16 [rows]
 * Replaces quantize_and_save_weight_ (ViDiT-Q/examples/Wan2.1/wan/quant_wanx_cuda.py:39-53); bit-identical to it
 * (tests/golden a12_*).  The codes feed `int_weight.pt` written with reference_format=True. */
int wanq_weight_export_f16(const void* w, int w_dtype, const void* delta_f16, const void* zp_f16, int8_t* q8,
                           int64_t rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention front-end for q / k:  y = x * rsqrt(mean(x^2) + eps) * weight   (RMSNorm over ALL cols),
 * then the 3-axis rotary embedding per head: pairs (2i, 2i+1) of every head are multiplied by
 * (cos + i sin) from rope[pos, i] with pos = row % rows_per_batch; rows with pos >= positions (sequence
 * padding) are left unrotated.  weight fp32[cols] or NULL (rope only); rope fp32[positions, head_dim/2, 2]
 * or NULL (norm only).  In place (out == x) is allowed.
 * Replaces WanRMSNorm.forward + rope_apply (ViDiT-Q/examples/Wan2.1/wan/modules/model.py:43-89), which the
 * reference evaluates with several torch passes and a float64 complex multiply. */
int wanq_rmsnorm_rope(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                      int out_dtype, int64_t rows, int cols, int head_dim, int64_t rows_per_batch,
                      int64_t positions, float eps, void* stream);

/* The same, additionally (or only: out may be NULL) emitting the row as per-(token, head) symmetric int8 codes for the int8
 * Q.K^T attention below: for every head slice of 128 columns  delta = max(absmax / 127, 1e-6),  q8 = clamp(rne(y / delta))
 * -- DynamicQuantizer on [tokens*heads, head_dim] rows, the q / k recipe of the reference's quantized attention
 * (ViDiT-Q/quant_utils/qdiff/base/quant_attn.py:168-174, examples/Wan2.1/models/quant_opensora.py:431-436).
 * q8: int8 [rows, cols].  qscale: fp32, two planes of [cols/128][scale_stride]: delta[h][row], then -12582912 * delta[h][row]
 * (the constant of the attention kernel's dequantising fma); scale_stride >= rows (for keys: rows rounded up to 64).
 * head_dim must be 128. */
int wanq_rmsnorm_rope_q8(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                         int out_dtype, int8_t* q8, float* qscale, int64_t scale_stride, int64_t rows, int cols,
                         int head_dim, int64_t rows_per_batch, int64_t positions, float eps, void* stream);

/* K smoothing for the int8 Q.K^T attention (SageAttention's remedy for a per-channel offset shared by all keys): subtracting one
 * vector c[cols] from every key changes all scores of a query row by the same q.c, which softmax does not see, so the keys may be
 * quantised as y - c with c = the mean of y over the tokens, and no attention kernel changes.  Two entries:
 *
 * wanq_rmsnorm_rope_colsum: colsum[c] = sum over all `rows` of y[r, c], y being the fp32 row wanq_rmsnorm_rope_q8 quantises (same
 * arguments, same bits; weight and rope may both be NULL: y = x).  Deterministic, a function of (rows, cols) only: rows are cut
 * into slabs of 64 rows (doubled until at most 1024 slabs remain), a slab is added in ascending row order per column, the slab
 * partials go to `workspace` and a second kernel adds them in ascending slab order; no floating-point atomics.  rows == 0 writes
 * zeros.  workspace: wanq_rmsnorm_rope_colsum_workspace(rows, cols) bytes of device memory, 16-byte aligned.  The centre of
 * `rows` tokens is colsum / rows (the caller's division; under sequence parallelism the sums of the ranks are added first). */
int64_t wanq_rmsnorm_rope_colsum_workspace(int64_t rows, int cols);
int wanq_rmsnorm_rope_colsum(const void* x, int x_dtype, const float* weight, const float* rope, int64_t rows, int cols,
                             int head_dim, int64_t rows_per_batch, int64_t positions, float eps, float* colsum,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* wanq_rmsnorm_rope_q8 with the codes taken of y - center (center: fp32 [cols], required; one fp32 subtraction per element):
 * delta, clamp, rounding and both scale planes as above, on the centred row.  `out`, when given, still receives the uncentred y.
 * center all zeros: bit-identical to wanq_rmsnorm_rope_q8. */
int wanq_rmsnorm_rope_q8_centered(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                                  int out_dtype, int8_t* q8, float* qscale, int64_t scale_stride, const float* center,
                                  int64_t rows, int cols, int head_dim, int64_t rows_per_batch, int64_t positions, float eps,
                                  void* stream);

/* The same as wanq_rmsnorm_rope with the store scattered per head: head h (head_dim columns) of row r lands at
 * out + head_map[2h] + r * head_map[2h+1] (elements of out_dtype).  head_map: DEVICE int64 [cols/head_dim][2].
 * Writes the Ulysses head-scatter all-to-all send buffers ([P][rows][w] per head chunk) directly, in place of the
 * permute + contiguous pack the reference's all_to_all_4D does around the collective
 * (ViDiT-Q/examples/Wan2.1/wan/distributed/xdit_context_parallel.py:147-192, yunchang SeqAllToAll4D). */
int wanq_rmsnorm_rope_scatter(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                              int out_dtype, const int64_t* head_map, int64_t rows, int cols, int head_dim,
                              int64_t rows_per_batch, int64_t positions, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flash-attention forward, non-causal:  o[q,h,:] = softmax_k(q[q,h,:].k[k,h,:] * scale) v[k,h,:] over the
 * first Lk keys.  Token-major tensors [tokens, heads*head_dim] with a token stride in ELEMENTS (so q/k/v may
 * be column slices of one packed buffer).  dtype: WANQ_BF16 or WANQ_F16, the one type of q, k, v and o (any other code is
 * refused with WANQ_E_ARG); head_dim: 128.  fp32 online softmax, S and P.V on v_mfma_f32_16x16x32_{bf16,f16}; the fp16 form keeps
 * P 2^8 above the bf16 form's so that it stays in fp16's normal range down to 22 log2 units below the row maximum.
 * Replaces flash_attention(q, k, v, k_lens) (ViDiT-Q/examples/Wan2.1/wan/modules/attention.py:24-130, which
 * calls the external flash_attn library) for batch size 1. */
int wanq_attention_fwd(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq,
                       int64_t Lk, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                       int64_t v_stride, int64_t o_stride, float scale, void* stream);

/* Sliding-window local attention: wanq_attention_fwd with every query restricted to a band of keys -- what the reference's
 * WanSelfAttention asks of flash_attn with window_size=(left, right) (ViDiT-Q/examples/Wan2.1/wan/modules/model.py:110-169,
 * attention.py:34,48,126).  With off = Lk - Lq, query i sees key j iff i + off - left <= j <= i + off + right and 0 <= j < Lk
 * (flash_attn's bottom-right alignment); a negative side is unbounded; a query that sees no key gets a row of exact zeros.
 * Arguments, refusals and the 8- / 4-wave choice (wanq_attention_select_form) as for wanq_attention_fwd, the choice made by the
 * keys a 256-query block walks (left + right + 256, at most Lk) in place of Lk.  Both sides negative: exactly the launch of
 * wanq_attention_fwd (bit-equal output).  A workgroup reads only the 64-key tiles its query block's band touches. */
int wanq_attention_window_fwd(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq, int64_t Lk,
                              int heads, int head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                              int64_t o_stride, float scale, int64_t window_left, int64_t window_right, void* stream);

/* The same with the keys split over `splits` workgroups per (query block, head) ("split-KV"): every share writes
 * unnormalised fp32 partials (O, reference maximum, row sum) into `workspace` and a second kernel merges them.  For launches
 * whose (query blocks x heads) grid leaves a large part of the last round of CUs idle -- 3 heads x 128 query blocks on 256
 * CUs under 4-way sequence parallelism: 1.5 rounds cost 2 -- halving the work unit restores the balance.
 * wanq_attention_split_workspace() gives the bytes `workspace` (16-byte aligned, device memory) must hold; splits <= 1 or
 * more splits than 64-key tiles fall back to fewer.  No counterpart in the reference (flash_attn picks its own splits). */
int64_t wanq_attention_split_workspace(int64_t Lq, int heads, int head_dim, int splits);

int wanq_attention_fwd_split(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq,
                             int64_t Lk, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                             int64_t v_stride, int64_t o_stride, float scale, int splits, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* Diagnostic: which form of the attention kernel wanq_attention_fwd launches (bf16 and fp16 alike).  The kernel exists with 8 waves per workgroup
 * (256 queries, three ring stages, one workgroup per CU) and with 4 (128 queries, two stages, two workgroups per CU); key sequences
 * up to `nw4_keys` run the 4-wave form (start-up default 1024 or WANQ_ATTN_NW4_KEYS: cross-attention), longer ones the 8-wave form.
 * 0 = always 8 waves, a large value = always 4, -1 = back to the start-up value.  Process-wide; returns the previous setting.
 * Outputs are bit-identical across the two forms (tests/test_gpu_block.py).  No reference counterpart. */
int64_t wanq_attention_select_form(int64_t nw4_keys);

/* Quantized Q.K^T (the reference's `attn.qk` fake-quant recipe, quant_attn.py:168-174, run on the integer matrix cores):
 *   o[q,h,:] = softmax_k( (q8[q,h,:] . k8[k,h,:]) * delta_q[h][q] * delta_k[h][k] * scale ) v[k,h,:]
 * q8 / k8: int8 [tokens, heads*128] with byte strides q8_stride / k8_stride; q_scale: fp32 [heads][qs_stride]; k_scale: fp32
 * two planes [heads][ks_stride] (delta_k, then -12582912*delta_k: the layout wanq_rmsnorm_rope_q8 writes), ks_stride >= Lk
 * rounded up to 64.  S = K8.Q8^T on v_mfma_i32_16x16x64_i8 (integer-exact), P.V in `dtype` as above; v / o of `dtype`
 * (WANQ_BF16 or WANQ_F16).
 * splits as in wanq_attention_fwd_split (1 = none; workspace from wanq_attention_split_workspace).
 * The reference wires this recipe for OpenSORA only (Q/base/quant_attn.py is imported, not used, by its Wan model). */
int wanq_attention_qk8_fwd(const int8_t* q8, const float* q_scale, int64_t qs_stride, const int8_t* k8,
                           const float* k_scale, int64_t ks_stride, const void* v, void* o, int dtype, int64_t Lq,
                           int64_t Lk, int heads, int head_dim, int64_t q8_stride, int64_t k8_stride,
                           int64_t v_stride, int64_t o_stride, float scale, int splits, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Attention with a QUANTISED ATTENTION MAP (the reference's `attn.attn_map` / `cross_attn.attn_map`, group 'row':
 * QuantizedAttentionMapOpenSORA, ViDiT-Q/quant_utils/qdiff/base/quant_attn.py:118-173, applied between softmax and `attn @ v`
 * at examples/Wan2.1/models/quant_opensora.py:459-476): every KEY column of the post-softmax map is one dynamic quantisation
 * group shared by all queries (DynamicQuantizer, base_quantizer.py:101-162), which on a map in [0, 1] is
 *   P~[q,k] = rne(P[q,k] / delta_k) * delta_k,  delta_k = max_q P[q,k] / L,  L = 2^(n_bits-1) - 1 (sym) or 2^n_bits - 1 (asym).
 * The reference materialises the N x N map (and asserts against flash attention); this entry point streams it in three passes
 * over the keys (row statistics, column maxima, quantised P.V), so it also runs at lengths where the map does not fit.  The map
 * is kept in fp32 (the reference rounds it to the model's 16-bit dtype first when it runs under autocast).
 * workspace: wanq_attention_map_workspace() bytes of device memory, 16-byte aligned.  q / k / v / o as in wanq_attention_fwd, but
 * dtype WANQ_BF16 only (both map entry points): P reaches the MFMA as a bf16 hi + lo pair, numerics that have no fp16 form yet. */
int64_t wanq_attention_map_workspace(int64_t Lq, int64_t Lk, int heads);
int wanq_attention_map_quant_fwd(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq, int64_t Lk,
                                 int heads, int head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                 int64_t o_stride, float scale, int n_bits, int sym, void* workspace,
                                 int64_t workspace_bytes, void* stream);
/* The reference's FULL quantised-attention recipe in one call (models/quant_opensora.py:431-476: the q / k / v quantisers AND the
 * attention-map quantiser): q and k as the per-(token, head) int8 codes and fp32 scale planes wanq_rmsnorm_rope_q8 writes
 * (q_scale / k_scale: plane [heads][stride] of delta; the key plane 16-byte aligned, its stride a multiple of 4 covering whole
 * 64-key tiles), S = K8 . Q8^T on the int8 matrix cores in all three passes; v is the caller's, already fake-quantised
 * (wanq_fake_quant_cols).  Same workspace, map quantiser and output as wanq_attention_map_quant_fwd. */
int wanq_attention_map_quant_qk8_fwd(const int8_t* q8, const float* q_scale, int64_t qs_stride, const int8_t* k8,
                                     const float* k_scale, int64_t ks_stride, const void* v, void* o, int dtype, int64_t Lq,
                                     int64_t Lk, int heads, int head_dim, int64_t q8_stride, int64_t k8_stride,
                                     int64_t v_stride, int64_t o_stride, float scale, int n_bits, int sym, void* workspace,
                                     int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ViDiT activation transform fused with the per-token quantiser:
 *   y = hadU(x * premul),   hadU = (H_K (x) H_128) / sqrt(cols)   (natural-order Walsh-Hadamard on each
 *   128-wide block, then the reference's +-1 table of order K across blocks)
 * premul fp32[cols] = channel_mask * rotation_signs (either may be all ones), or NULL.  had_k = 0: no rotation, y = x * premul
 * (SmoothQuant, any cols % 8 == 0); otherwise had_k must equal cols / 128
 * (the caller states the factorisation it expects); the table across blocks is the one get_hadK picks for this width
 * (ViDiT-Q/quant_utils/qdiff/quarot/quarot_utils.py:100-155), a fixed function of cols: Sylvester for 2^p (had_k <= 32),
 * Paley-I of order 12 for 1536, H_2 (x) Paley-I of order 20 for 5120 -- generated inside the library, not passed in.
 * Equals `x*channel_mask -> (x.double() @ rotation_matrix)` of ViDiTQuantizedLinear.forward
 * (ViDiT-Q/quant_utils/qdiff/viditq/viditq_quant_layer.py:62-63) because row i of the random Hadamard
 * matrix is sign_i * hadU(e_i) (quarot_utils.py:186-192); evaluated in fp32 registers with O(n log n + nK) adds instead
 * of a dense fp64 GEMM, no LDS.  Outputs: fp (out_fp) and/or int8 codes + scale (+sum), as wanq_quant_rows.  (No activation
 * option: tanh-GELU in front of a transformed layer is fused into the producing GEMM, WANQ_EPI_GELU.) */
int wanq_rotate_quant_rows(const void* x, int x_dtype, const float* premul, int had_k, void* out_fp, int out_dtype,
                           int8_t* q, void* scale, void* sum, int vec_dtype, int64_t rows, int cols, void* stream);

/* LayerNorm -> modulate (as wanq_layernorm_rows) -> ViDiT transform -> int8 quantise, one kernel. */
int wanq_layernorm_rotate_quant_rows(const void* x, int x_dtype, const void* gamma, const void* mshift,
                                     const void* mscale, int mod_dtype, int64_t mod_stride, int64_t rows_per_batch,
                                     float eps, const float* premul, int had_k, int8_t* q, void* scale, void* sum,
                                     int vec_dtype, int64_t rows, int cols, void* stream);

/* The same, for up to three consumers of ONE normalised row: self-attention q / k / v share norm1 and the modulation
 * (ViDiT-Q/examples/Wan2.1/wan/modules/model.py:327-331) but each ViDiTQuantizedLinear has its own channel mask and
 * rotation signs (viditq_quant_layer.py:30-38), so the reference normalises, scales, rotates (fp64 GEMM) and quantises
 * three times.  Here x is read and normalised once; set t gets hadU(LN(x) * premul[t]) quantised into q[t] / scale[t] /
 * sum[t].  premul / q / scale / sum are host arrays of nsets (1..3) device pointers. */
int wanq_layernorm_rotate_quant_rows_multi(const void* x, int x_dtype, const void* gamma, const void* mshift,
                                           const void* mscale, int mod_dtype, int64_t mod_stride, int64_t rows_per_batch,
                                           float eps, int nsets, const float* const* premul, int had_k,
                                           int8_t* const* q, void* const* scale, void* const* sum, int vec_dtype,
                                           int64_t rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 4-bit weights.  Storage: row-major [N, K/2] bytes, K % 32 == 0; each group of 32 consecutive codes takes 16 bytes = 4
 * dwords (P0a, P1a, P0b, P1b); for a 16-code half e[0..15] (a = codes 0-15, b = codes 16-31 of the group), as unsigned
 * nibbles u = e + bias:   P0 byte i = u[i] | u[4+i] << 4,   P1 byte i = u[8+i] | u[12+i] << 4   (i = 0..3),
 * so `P & 0x0f0f0f0f` and `(P >> 4) & 0x0f0f0f0f` are the dwords of an int8 MFMA operand.  bias 8 for signed codes in
 * [-8,7] (qdiff 4-bit asym, base_quantizer.py:32,89-90), bias 0 for unsigned codes 0..15 (QServe convention,
 * ViDiT-Q/kernels/csrc/qgemm/w4a8/w4a8_per_channel_gemm_cuda_qserve.cu:287-299).  The reference exports a W4A8 GEMM
 * (w4a8_of16_nobias_weight_asym_qserve) but ships neither a packer nor a module that calls it, and its layout is an NVIDIA
 * ldmatrix interleave; this layout is the CDNA4 counterpart. */
int wanq_pack_w4(const int8_t* q, uint8_t* packed, int bias, int64_t rows, int cols, void* stream);
int wanq_unpack_w4(const uint8_t* packed, int8_t* q, int bias, int64_t rows, int cols, void* stream);

/* W4A8 GEMM: as wanq_gemm_w8a8 with `w_packed` = UNSIGNED nibbles u in [0,15] in the layout above (N x K/2 bytes), expanded to
 * int8 in registers next to the MFMA (the weight panel's HBM / LDS bytes halve):
 *   acc[m,n] = sum_k a[m,k] * u[n,k];   y = acc*sa[m]*sw[n] (+ asum[m]*zp[n]*sw[n]) (+ bias[n]) ...   (same epilogue flags)
 * With zp = -zero this is y = acc*sW*sA - (sW*zW)*sumA (w4a8_per_channel_gemm_cuda_qserve.cu:580-587); signed qdiff codes q
 * stored with bias 8 use zp = zero_point - 8.  K % 32 == 0.
 * Replaces qgemm.w4a8_of16_nobias_weight_asym_qserve (ViDiT-Q/kernels/csrc/qgemm/w4a8/w4a8_per_channel_gemm_cuda_qserve.cu:304-656). */
int wanq_gemm_w4a8(const int8_t* a, const uint8_t* w_packed, void* out, int out_dtype, const void* sa,
                   const void* asum, int tok_dtype, const void* sw, const void* bias, int ch_dtype,
                   const void* zp, int zp_dtype, const float* gate, const void* residual, int epi_flags,
                   int64_t M, int N, int K, void* stream);

/* Group-wise W8A8 / W4A8 GEMM (the W4A8-g128 form of QServe-style checkpoints): int8 activations against integer weight codes with
 * one scale and one zero point per output channel and per group of `group_size` input channels.
 *   - sw and zp are fp32 [K / group_size][N], group-major: the layout wanq_gemm_wq16_grouped takes.  zp may be NULL, meaning 0.
 *   - w_bits = 4: w is the packed unsigned nibbles u of wanq_pack_w4 ([N, K/2] bytes) and zp = zero_point - 8, the W4A8 convention.
 *     The integer weight operand is u + zp[g,n]; the kernel forms it in registers while expanding the nibbles, before the MFMA.  For
 *     every StaticQuantizer output u + zp = q + zero_point lies in [-15, 15] (asymmetric: q + zero_point = round(w / delta) lies in
 *     [round(min- / delta), round(min- / delta) + 15] and min- / delta >= -15), so the operand is an exact int8 and no per-token,
 *     per-group activation sums are needed for the zero point.  Precondition: zp integer valued, u + zp in [-128, 127].
 *   - w_bits = 8: w is int8 [N, K] and zp must be NULL (symmetric weights); a non-NULL zp is refused with WANQ_E_ARG: c + zp does not
 *     fit int8, and the rank-one correction would need per-group token sums, which no producer writes.
 *   - part_g[m,n] = sum_{k in group g} a[m,k] * (u[n,k] + zp[g,n]): int32, exact, on v_mfma_i32_32x32x32_i8.  The conversion
 *     (float)part_g is exact while |part_g| < 2^24: for group_size <= 1024 at 8 bits, and always at 4 bits for group_size <= 8192.
 *     Beyond that it is round-to-nearest-even.
 *   - acc = fmaf((float)part_g, sw[g,n], acc), g ascending from acc = 0.
 *   - y = fmaf(acc, sa[m], bias[n]), bias 0 when NULL; sa is the per-token scale of wanq_quant_rows, dtype tok_dtype (F16 | F32);
 *     bias of ch_dtype (F16 | F32).
 *   - WANQ_EPI_GELU, WANQ_EPI_GATE_RES (y = fmaf(y, gate[n], residual[m,n])) and the single rounding to out_dtype (F16 | BF16 | F32)
 *     as wanq_gemm_w8a8 specifies them, with the same gelu_tanh_fast_f32.  out may alias residual.
 *   - Determinism: the bits of element (m, n) depend on K and group_size only -- not on M, on the row's place in the launch or on
 *     the workgroup.  No split-K.
 *   - Shapes: any M >= 1 (ragged last tile in-kernel, no host padding); N % 8 == 0; group_size % 128 == 0 and K % group_size == 0;
 *     a, w, out, residual, sw and zp 16-byte aligned; gate and bias aligned to 4 elements; out_dtype == WANQ_I32 is refused (there
 *     is no single integer accumulator to return).  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).
 * wanq_gemm_select_kernel does not apply: one kernel form.  The reference has per-channel int8 GEMMs only
 *   (ViDiT-Q/kernels/csrc/qgemm/w4a8/w4a8_per_channel_gemm_cuda_qserve.cu); group-wise weights are its StaticQuantizer applied to
 *   w.view(N K / g, g), as for wanq_gemm_wq16_grouped. */
int wanq_gemm_w8a8_grouped(const int8_t* a, const void* w, int w_bits, const float* sw, const float* zp, int group_size,
                           void* out, int out_dtype, const void* sa, int tok_dtype, const void* bias, int ch_dtype,
                           const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream);

/* fp8 W8A8 GEMM: per-token dynamic e4m3 activations against per-channel e4m3 weights (both from wanq_quant_rows_fp8), on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands, unit block scales: twice the rate of the unscaled fp8 instruction) with the epilogue of
 * wanq_gemm_bf16:
 *   acc[m,n] = sum_k a[m,k] * w[n,k]               (a, w: OCP e4m3fn bytes, row-major [M, K] and [N, K]; every product exact in fp32,
 *                                                   fp32 accumulation on the matrix cores)
 *   y   = fmaf(acc * sa[m], sw[n], bias[n])        (sa fp32 [M], sw fp32 [N]; bias F16 | BF16 | F32 or NULL = 0; this order, fp32)
 *   y   = gelu_tanh(y)                             if WANQ_EPI_GELU
 *   y   = residual[m,n] + y * gate[n]              if WANQ_EPI_GATE_RES  (gate fp32 [N], residual of out_dtype; out may alias it)
 *   out = cast(y) to out_dtype (F16 | BF16 | F32): one rounding.
 * Shapes: any M >= 1 (ragged last tile in-kernel, no host padding); N % 8 == 0; K % 64 == 0 -- the kernel's K step: one 16-byte
 * fragment read per lane, half of the 128-deep MFMA (K % 128 == 64 is a ragged last K-tile, handled in-kernel: the missing half of
 * both fragments is zeros).  a, w, out, residual and sw
 * 16-byte aligned, gate and bias aligned to 4 elements, sa to 4 bytes.  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the
 * message names the rule).
 * Determinism: one kernel form, no split-K; the fp32 summation order of element (m, n) depends on K only, so a row gives the same
 * bits at any m and in a launch of any M, and repeated calls are bit-identical.  With integer-valued operands whose partial sums
 * stay below 2^24 the accumulator is the exact integer product.
 * No reference counterpart (its 8-bit Linears are int8: ViDiT-Q/kernels/csrc/qgemm/w8a8/w8a8_gemm_cuda.cu). */
int wanq_gemm_fp8(const uint8_t* a, const uint8_t* w, const float* sa, const float* sw, void* out, int out_dtype, const void* bias,
                  int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream);

/* MX GEMM: MXFP8 (e4m3) activations against MXFP8 (e4m3) or MXFP4 (e2m1) weights, both from wanq_quant_rows_mx, on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with the E8M0 block scales applied by the matrix cores, and the epilogue of wanq_gemm_bf16:
 *   acc[m,n] = sum_b 2^(sa[m,b] - 127) 2^(sw[n,b] - 127) sum_{k in block b} a[m,k] * w[n,k]      (fp32 accumulation on the matrix cores;
 *                                                   every product is exact in fp32)
 *   y   = acc + bias[n]                            (bias F16 | BF16 | F32 or NULL = 0; no fp32 row or channel scale: the hardware has
 *                                                   applied every scale)
 *   y   = gelu_tanh(y)                             if WANQ_EPI_GELU
 *   y   = residual[m,n] + y * gate[n]              if WANQ_EPI_GATE_RES  (gate fp32 [N], residual of out_dtype; out may alias it)
 *   out = cast(y) to out_dtype (F16 | BF16 | F32): one rounding.
 * a: e4m3 bytes [M, K].  w_fmt WANQ_MX_E4M3: w e4m3 bytes [N, K];  WANQ_MX_E2M1: w packed nibbles [N, K / 2].  sa_u8 [M, K / 32],
 * sw_u8 [N, K / 32]: E8M0 bytes, 4-byte aligned (a K-tile's four bytes of a row are read as one dword).
 * Shapes: any M >= 1 (ragged last tile in-kernel); N % 8 == 0; K % 128 == 0 (one K-tile = one 128-deep MFMA = four blocks).  a, w, out
 * and residual 16-byte aligned, gate and bias aligned to 4 elements.  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the
 * message names the rule).
 * Determinism: one kernel form per weight format, no split-K; the summation order of element (m, n) depends on K only, so a row
 * gives the same bits at any m and in a launch of any M, and repeated calls are bit-identical.
 * No reference counterpart (its Linears are integer ones: ViDiT-Q/kernels/csrc/qgemm/w8a8/w8a8_gemm_cuda.cu). */
int wanq_gemm_mx(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, int w_fmt, void* out, int out_dtype,
                 const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K,
                 void* stream);

/* W4A4 MX GEMM: MXFP4 (e2m1) activations against MXFP4 (e2m1) weights, both from wanq_quant_rows_mx (fmt WANQ_MX_E2M1) or both from
 * wanq_quant_rows_mx_had32, on v_mfma_scale_f32_16x16x128_f8f6f4 with both operands 4 bits wide (the instruction's fp4 rate).
 * Semantics, epilogue, shape rules and determinism statement are wanq_gemm_mx's, word for word:
 *   acc[m,n] = sum_b 2^(sa[m,b] - 127) 2^(sw[n,b] - 127) sum_{k in block b} a[m,k] * w[n,k];  y = acc + bias[n];  GELU;
 *   residual + y * gate;  one rounding to out_dtype.
 * a: packed nibbles [M, K / 2], w: packed nibbles [N, K / 2], even k in the low nibble.  sa_u8 [M, K / 32], sw_u8 [N, K / 32]: E8M0
 * bytes, 4-byte aligned.  Any M >= 1 (M == 0 returns WANQ_OK); N % 8 == 0; K % 128 == 0.  a, w, out and residual 16-byte aligned, gate
 * and bias aligned to 4 elements.  Anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).
 * Determinism: one kernel form, no split-K; the summation order of element (m, n) depends on K only, so a row gives the same bits at
 * any m and in a launch of any M, and repeated calls are bit-identical.
 * No reference counterpart. */
int wanq_gemm_mx4(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, void* out, int out_dtype,
                  const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K,
                  void* stream);

/* MXFP6 GEMMs, W6A6 and W4A6: e2m3 activations (wanq_quant_rows_mx6) against e2m3 weights (w_fmt WANQ_MX_E2M3, the same entry once
 * at conversion) or packed e2m1 weights (w_fmt WANQ_MX_E2M1, wanq_quant_rows_mx), on v_mfma_scale_f32_16x16x128_f8f6f4 with no
 * operand 8 bits wide (the instruction's fp4 rate).  Semantics, epilogue, shape rules and determinism statement are wanq_gemm_mx4's:
 *   acc[m,n] = sum_b 2^(sa[m,b] - 127) 2^(sw[n,b] - 127) sum_{k in block b} a[m,k] * w[n,k];  y = acc + bias[n];  GELU;
 *   residual + y * gate;  one rounding to out_dtype.
 * a: packed e2m3 codes [M, 3 K / 4].  w: packed e2m3 codes [N, 3 K / 4] or packed e2m1 nibbles [N, K / 2].  sa_u8 [M, K / 32], sw_u8
 * [N, K / 32]: E8M0 bytes, 4-byte aligned.  Any M >= 1 (M == 0 returns WANQ_OK); N % 8 == 0; K % 128 == 0 (a row and a K-tile's 96
 * bytes are then 16-byte aligned).  a, w, out and residual 16-byte aligned, gate and bias aligned to 4 elements.  Any other w_fmt
 * and anything else is refused (WANQ_E_SHAPE / WANQ_E_ARG, the message names the rule).
 * Determinism: one kernel form per w_fmt, no split-K; the summation order of element (m, n) depends on K only.
 * No reference counterpart. */
int wanq_gemm_mx6(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, int w_fmt, void* out, int out_dtype,
                  const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Step-level elementwise work of the denoising loop in one kernel:  out[o] = sum_i coef[o][i] * in[i]  over fp32 tensors of
 * `numel` elements (n_out <= 4, n_in <= 8; `in` / `out` are HOST arrays of device pointers, 16-byte aligned, outputs may
 * alias inputs element for element).  Classifier-free guidance, the model-output conversion and the UniPC / DPM++ / Euler
 * predictor and corrector are all such combinations (ViDiT-Q/examples/Wan2.1/wan/text2video.py:260-269,
 * wan/utils/fm_solvers_unipc.py:303-307,354-630): one launch replaces the ~12 elementwise torch kernels of a step.
 * coef: HOST fp32 [n_out][n_in], copied into the kernel arguments by this call (the launch does not read it afterwards). */
int wanq_lincomb(int n_out, int n_in, const float* coef, const float* const* in, float* const* out, int64_t numel,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * The fp32 ends of a DiT pass (ViDiT-Q/examples/Wan2.1/wan/modules/model.py:580-610 embeddings, :372-400 Head, :633-656
 * unpatchify), one fp32 matrix-core tile kernel with the gather / LayerNorm / scatter folded into its loads and stores.
 * Activations: 0 none, 1 GELU (tanh form), 2 SiLU.  All tensors fp32, row-major, 16-byte aligned; K a multiple of 16.
 *
 * wanq_linear_f32:  out[M, N] = act_out(act_in(x)[M, K] . w[N, K]^T + bias)      (bias may be NULL)
 *   x holds x_rows <= M rows; the missing ones are zeros (text_embedding pads its input to text_len, model.py:600-605).
 *   replaces nn.Linear / nn.Sequential(Linear, act, Linear) of time_embedding, time_projection, text_embedding.
 * wanq_time_sinusoid: sinusoidal_embedding_1d (model.py:18-28) of n positions (t_kind: 0 fp32, 1 int64, 2 fp64, 3 int32), float64
 *   angles, cos half first; out fp32 [n, dim]. */
int wanq_linear_f32(const float* x, int64_t x_rows, const float* w, const float* bias, float* out, int64_t M, int N, int K,
                    int in_act, int out_act, void* stream);
int wanq_time_sinusoid(const void* t, int t_kind, float* out, int n, int dim, void* stream);
/* wanq_patch_embed: Conv3d(C -> N, kernel = stride = (pt, ph, pw)) on latent [C, F, H, W] (model.py:580-584), w = the
 *   convolution weight [N, C, pt, ph, pw]; out [out_rows, N], token (f, h, w) in row (f * H/ph + h) * W/pw + w, rows from the token
 *   count up to out_rows zero (the reference pads the sequence to seq_len, model.py:586-590). */
int wanq_patch_embed(const float* latent, const float* w, const float* bias, float* out, int C, int F, int H, int W, int pt,
                     int ph, int pw, int N, int64_t out_rows, void* stream);
/* wanq_head_fwd: Head.forward (model.py:391-399): LayerNorm(x[rows, K], eps, no affine) * (1 + modulation[1] + e) + modulation[0] + e,
 *   then Linear(K -> N).  modulation [2, K], e [K].  unpatchify == 0: out [rows, N].  unpatchify != 0: rows must be the token count
 *   of the latent [C, F, H, W] under patch (pt, ph, pw), N == C * pt * ph * pw <= 64, and out is that latent (model.py:633-656). */
int wanq_head_fwd(const float* x, const float* modulation, const float* e, const float* w, const float* bias, float* out,
                  int64_t rows, int K, int N, float eps, int unpatchify, int C, int F, int H, int W, int pt, int ph, int pw,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WANQ_HIP_H */
