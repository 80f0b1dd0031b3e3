// Kernels that run once per model or only in calibration: column absmax, weight row statistics, static weight quantisation,
// the reference-format int8 export, the fake-quantisers of the quantized-attention emulation, and the 4-bit weight packing.
// Layout and row frame as in row_frame.h.
#include "row_frame.h"

namespace wanq {

// ------------------------------------------------------------------------------ calibration: column absmax
// Each workgroup owns a 512-column panel (64 lanes x 8 columns) and a slab of rows; a lane keeps 8
// running maxima in registers, the 4 waves of a workgroup take rows round-robin, partials meet in LDS
// and one atomicMax per column per workgroup goes to HBM (non-negative floats order like uints).
template <typename T>
__global__ __launch_bounds__(256) void col_absmax_kernel(const void* x, float* colmax, int64_t rows, int cols,
                                                         int rows_per_block) {
  __shared__ float part[4][512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 512 + lane * 8;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < rows) ? r0 + rows_per_block : rows;
  float m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = 0.f;
  if (c0 < cols) {
    int64_t r = r0 + wave;
    for (; r + 12 < r1; r += 16) {  // 4 independent loads in flight per lane
      float a[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) Io<T>::load8(x, (r + 4 * u) * cols + c0, a[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], fabsf(a[u][j]));
    }
    for (; r < r1; r += 4) {
      float a[8];
      Io<T>::load8(x, r * cols + c0, a);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], fabsf(a[j]));
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[wave][lane * 8 + j] = m[j];
  __syncthreads();
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int col = blockIdx.x * 512 + c;
    if (col < cols) {
      const float v = fmaxf(fmaxf(part[0][c], part[1][c]), fmaxf(part[2][c], part[3][c]));
      atomicMax(reinterpret_cast<unsigned int*>(colmax + col), __float_as_uint(v));
    }
  }
}

// ------------------------------------------------------------------------------ weight row statistics
template <int WPR, int NCH>
__global__ __launch_bounds__(256) void row_minmax_kernel(const void* w, int dt, float* rmin, float* rmax,
                                                         float* rabs, int64_t rows, int cols) {
  __shared__ float slots[2 * WPR];
  RowFrame<WPR, NCH> f;
  if (f.surplus(rows)) return;
  const RowReduce<WPR> red{slots, f.wave};
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (f.col(i) < cols) {
      float v[8];
      load8_rt(w, dt, f.row * cols + f.col(i), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        lo = fminf(lo, v[j]);
        hi = fmaxf(hi, v[j]);
      }
    }
  }
  lo = red.template reduce<OpMin>(lo, 0);
  hi = red.template reduce<OpMax>(hi, 1);
  if (f.lane == 0 && f.sub == 0) {
    if (rmin) rmin[f.row] = lo;
    if (rmax) rmax[f.row] = hi;
    if (rabs) rabs[f.row] = fmaxf(fabsf(lo), fabsf(hi));
  }
}

// ------------------------------------------------------------------------------ static weight quantisation
__global__ __launch_bounds__(256) void weight_quant_kernel(const void* w, int dt, const float* delta, const float* zp,
                                                           int qmin, int qmax, int8_t* q8, float* deq, int64_t rows,
                                                           int cols) {
  const int cpr = cols / 8;
  const int64_t total = rows * (int64_t)cpr;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < total; ch += (int64_t)gridDim.x * 256) {
    const int64_t row = ch / cpr;
    const int c0 = (int)(ch - row * cpr) * 8;
    float v[8];
    load8_rt(w, dt, row * cols + c0, v);
    const float d = delta[row], z = zp[row];
    int qi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // rne(w/delta) - zp, clamp   (base_quantizer.py:64-67); true division: runs once per model
      float t = rintf(v[j] / d) - z;
      t = fminf(fmaxf(t, (float)qmin), (float)qmax);  // the reference's (loose) clamp for the fake-quant value
      qi[j] = (int)fminf(fmaxf(t, -128.f), 127.f);     // int8 storage saturates on top of it
      v[j] = (t + z) * d;
    }
    if (q8)
      *reinterpret_cast<uint2*>(q8 + row * cols + c0) =
          make_uint2(pack4_i8(qi[0], qi[1], qi[2], qi[3]), pack4_i8(qi[4], qi[5], qi[6], qi[7]));
    if (deq) Io<F32>::store8(deq, row * cols + c0, v);
  }
}

// ------------------------------------------------------------------------------ reference-format int8 export
// quantize_and_save_weight_ (W/wan/quant_wanx_cuda.py:39-53): everything in HALF precision --
//   int8 = clamp( round( f16(w) / f16(delta) ) - f16(zp), -128, 127 )
// torch evaluates the fp16 quotient as fl16(fl32(a / b)); round() and the subtraction are exact on these magnitudes.
__global__ __launch_bounds__(256) void weight_export_f16_kernel(const void* w, int dt, const __half* delta, const __half* zp,
                                                                int8_t* q8, int64_t rows, int cols) {
  const int cpr = cols / 8;
  const int64_t total = rows * (int64_t)cpr;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < total; ch += (int64_t)gridDim.x * 256) {
    const int64_t row = ch / cpr;
    const int c0 = (int)(ch - row * cpr) * 8;
    float v[8];
    load8_rt(w, dt, row * cols + c0, v);
    const float d = __half2float(delta[row]), z = __half2float(zp[row]);
    int qi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float w16 = __half2float(__float2half_rn(v[j]));        // fp_module.weight.to(torch.float16)
      const float quo = __half2float(__float2half_rn(w16 / d));     // fp16 division
      const float t = __half2float(__float2half_rn(rintf(quo) - z));
      qi[j] = (int)fminf(fmaxf(t, -128.f), 127.f);
    }
    *reinterpret_cast<uint2*>(q8 + row * cols + c0) =
        make_uint2(pack4_i8(qi[0], qi[1], qi[2], qi[3]), pack4_i8(qi[4], qi[5], qi[6], qi[7]));
  }
}

}  // namespace wanq

using namespace wanq;

extern "C" int wanq_weight_export_f16(const void* w, int w_dtype, const void* delta_f16, const void* zp_f16, int8_t* q8,
                                      int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(w && delta_f16 && zp_f16 && q8, WANQ_E_ARG, "wanq_weight_export_f16: NULL pointer");
  WANQ_REQUIRE(is_fp(w_dtype), WANQ_E_ARG, "wanq_weight_export_f16: bad dtype %d", w_dtype);
  if (int e = check_rows_cols("wanq_weight_export_f16", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  const int64_t total = rows * (cols / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(weight_export_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, w_dtype,
                     static_cast<const __half*>(delta_f16), static_cast<const __half*>(zp_f16), q8, rows, cols);
  return check_launch("wanq_weight_export_f16");
}

extern "C" int wanq_col_absmax(const void* x, int x_dtype, float* colmax, int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(x && colmax, WANQ_E_ARG, "wanq_col_absmax: NULL pointer");
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "wanq_col_absmax: bad dtype %d", x_dtype);
  WANQ_REQUIRE(cols >= 8 && cols % 8 == 0, WANQ_E_SHAPE, "wanq_col_absmax: cols=%d must be a multiple of 8", cols);
  WANQ_REQUIRE(rows >= 0 && rows < (1ll << 40), WANQ_E_SHAPE, "wanq_col_absmax: rows out of range");
  if (rows == 0) return WANQ_OK;
  const unsigned panels = (unsigned)((cols + 511) / 512);
  // ~2048 workgroups in total, at least 64 rows each
  int64_t slabs = 2048 / panels;
  if (slabs < 1) slabs = 1;
  int64_t rpb = (rows + slabs - 1) / slabs;
  if (rpb < 64) rpb = 64;
  slabs = (rows + rpb - 1) / rpb;
  WANQ_REQUIRE(slabs <= 65535, WANQ_E_SHAPE, "wanq_col_absmax: too many row slabs");
  dim3 grid(panels, (unsigned)slabs);
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == WANQ_F16) hipLaunchKernelGGL(col_absmax_kernel<F16>, grid, dim3(256), 0, st, x, colmax, rows, cols, (int)rpb);
  else if (x_dtype == WANQ_BF16) hipLaunchKernelGGL(col_absmax_kernel<BF16>, grid, dim3(256), 0, st, x, colmax, rows, cols, (int)rpb);
  else hipLaunchKernelGGL(col_absmax_kernel<F32>, grid, dim3(256), 0, st, x, colmax, rows, cols, (int)rpb);
  return check_launch("wanq_col_absmax");
}

// v fake-quantisation of the reference's quantized attention: DynamicQuantizer over ALL TOKENS for every (head, channel) --
// `self.v_quantizer(v.permute([0,1,3,2]).reshape([-1, N_token]))`, ViDiT-Q/examples/Wan2.1/models/quant_opensora.py:438-440 --
// i.e. per COLUMN of the token-major [tokens, heads*head_dim] tensor: delta_c = max(absmax_c / n, 1e-6), n = 2^(b-1) - 1,
// y = clamp(rne(x / delta_c), -n-1, n) * delta_c.  colmax comes from wanq_col_absmax over the same rows.
namespace wanq {
__global__ __launch_bounds__(256) void fake_quant_cols_kernel(const void* x, int x_dt, const float* colmax, void* out, int out_dt,
                                                              float nlev, int64_t rows, int cols) {
  const int cpr = cols / 8;
  const int64_t total = rows * (int64_t)cpr;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < total; ch += (int64_t)gridDim.x * 256) {
    const int64_t row = ch / cpr;
    const int c0 = (int)(ch - row * cpr) * 8;
    float v[8], m[8];
    load8_rt(x, x_dt, row * cols + c0, v);
    Io<F32>::load8(colmax, c0, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = m[j] / nlev;
      if (d < 1e-6f) d = 1e-6f;
      v[j] = __builtin_amdgcn_fmed3f(rintf(v[j] / d), -nlev - 1.f, nlev) * d;
    }
    store8_rt(out, out_dt, row * cols + c0, v);
  }
}
}  // namespace wanq

extern "C" int wanq_fake_quant_cols(const void* x, int x_dtype, const float* colmax, void* out, int out_dtype, int n_bits,
                                    int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(x && colmax && out, WANQ_E_ARG, "wanq_fake_quant_cols: NULL pointer");
  WANQ_REQUIRE(is_fp(x_dtype) && is_fp(out_dtype), WANQ_E_ARG, "wanq_fake_quant_cols: bad dtype code");
  WANQ_REQUIRE(n_bits >= 2 && n_bits <= 8, WANQ_E_ARG, "wanq_fake_quant_cols: n_bits=%d must be in [2, 8]", n_bits);
  WANQ_REQUIRE(cols >= 8 && cols % 8 == 0, WANQ_E_SHAPE, "wanq_fake_quant_cols: cols=%d must be a multiple of 8", cols);
  WANQ_REQUIRE(rows >= 0 && rows < (1ll << 40), WANQ_E_SHAPE, "wanq_fake_quant_cols: rows out of range");
  if (rows == 0) return WANQ_OK;
  const int64_t total = rows * (cols / 8);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(fake_quant_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_dtype, colmax, out,
                     out_dtype, (float)((1 << (n_bits - 1)) - 1), rows, cols);
  return check_launch("wanq_fake_quant_cols");
}

// ------------------------------------------------------------------------------ fake-quant with a precomputed delta
// DynamicQuantizer.forward_with_quant_params (Q/base/base_quantizer.py:164-206): elementwise, delta has x's shape; optional per-element
// bit-widths (`mixed_precision`).  IEEE divisions, as the reference's torch ops (an HBM-bound pass: 12-16 B per element).
namespace wanq {
__global__ __launch_bounds__(256) void fake_quant_delta_kernel(const void* x, int x_dt, const float* delta, const int32_t* bits, void* out,
                                                               int out_dt, float levels, int64_t chunks) {
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < chunks; ch += (int64_t)gridDim.x * 256) {
    float v[8], d[8];
    load8_rt(x, x_dt, ch * 8, v);
    Io<F32>::load8(delta, ch * 8, d);
    int b[8];
    if (bits) {
      const int4 b0 = *reinterpret_cast<const int4*>(bits + ch * 8), b1 = *reinterpret_cast<const int4*>(bits + ch * 8 + 4);
      b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float dj = d[j] < 1e-6f ? 1e-6f : d[j];  // :181-189
      if (bits) {  // levels 2^bits - 1; 0 bits: computed as 8 bits, then masked (:174-178, :203-204); clipped from above only (:194)
        const bool zero = b[j] == 0;
        const float nl = zero ? 255.f : (float)((1u << b[j]) - 1u);
        dj = dj / nl;
        const float xi = rintf(v[j] / dj);
        v[j] = zero ? 0.f : (xi > nl ? nl : xi) * dj;
      } else {     // :196-199
        dj = dj / levels;
        v[j] = __builtin_amdgcn_fmed3f(rintf(v[j] / dj), 0.f, levels) * dj;
      }
    }
    store8_rt(out, out_dt, ch * 8, v);
  }
}
}  // namespace wanq

extern "C" int wanq_fake_quant_with_delta(const void* x, int x_dtype, const float* delta, const int32_t* bits, void* out, int out_dtype,
                                          int n_bits, int64_t n, void* stream) {
  WANQ_REQUIRE(x && delta && out, WANQ_E_ARG, "wanq_fake_quant_with_delta: NULL pointer");
  WANQ_REQUIRE(is_fp(x_dtype) && is_fp(out_dtype), WANQ_E_ARG, "wanq_fake_quant_with_delta: bad dtype code");
  WANQ_REQUIRE(n_bits >= 2 && n_bits <= 16, WANQ_E_ARG, "wanq_fake_quant_with_delta: n_bits=%d must be in [2, 16]", n_bits);
  WANQ_REQUIRE(n >= 0 && n % 8 == 0 && n < (1ll << 40), WANQ_E_SHAPE, "wanq_fake_quant_with_delta: n=%lld must be a multiple of 8", (long long)n);
  if (n == 0) return WANQ_OK;
  int64_t blocks = (n / 8 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  // symmetric quantiser: n_levels = 2^(b-1) - 1, the unsigned range of this method is 2 n_levels + 1 = 2^b - 1
  hipLaunchKernelGGL(fake_quant_delta_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_dtype, delta, bits, out, out_dtype,
                     (float)((1u << n_bits) - 1u), n / 8);
  return check_launch("wanq_fake_quant_with_delta");
}

extern "C" int wanq_row_minmax(const void* w, int w_dtype, float* row_min, float* row_max, float* row_absmax,
                               int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(w && (row_min || row_max || row_absmax), WANQ_E_ARG, "wanq_row_minmax: NULL pointer");
  WANQ_REQUIRE(is_fp(w_dtype), WANQ_E_ARG, "wanq_row_minmax: bad dtype %d", w_dtype);
  if (int e = check_rows_cols("wanq_row_minmax", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = cols / 8;
  if (chunks <= 256)
    hipLaunchKernelGGL((row_minmax_kernel<1, 4>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, w, w_dtype, row_min, row_max, row_absmax, rows, cols);
  else
    hipLaunchKernelGGL((row_minmax_kernel<4, 8>), dim3((unsigned)rows), dim3(256), 0, st, w, w_dtype, row_min, row_max, row_absmax, rows, cols);
  return check_launch("wanq_row_minmax");
}

extern "C" int wanq_weight_quant(const void* w, int w_dtype, const float* delta, const float* zp, int qmin, int qmax,
                                 int8_t* q8, float* deq, int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(w && delta && zp && (q8 || deq), WANQ_E_ARG, "wanq_weight_quant: NULL pointer");
  WANQ_REQUIRE(is_fp(w_dtype), WANQ_E_ARG, "wanq_weight_quant: bad dtype %d", w_dtype);
  WANQ_REQUIRE(qmin < qmax, WANQ_E_ARG, "wanq_weight_quant: bad clamp range [%d,%d]", qmin, qmax);
  if (int e = check_rows_cols("wanq_weight_quant", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  const int64_t total = rows * (cols / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(weight_quant_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, w_dtype, delta, zp, qmin, qmax, q8, deq, rows, cols);
  return check_launch("wanq_weight_quant");
}

// ------------------------------------------------------------------------------ 4-bit weight storage
// Packed layout (ours; the reference ships no packer and its QServe layout is an NVIDIA ldmatrix interleave): row-major
// [N, K/2] bytes, K % 32 == 0.  Each group of 32 consecutive codes takes 16 bytes = 4 dwords (P0a, P1a, P0b, P1b); for a
// 16-code half e[0..15] (a = codes 0-15 of the group, b = codes 16-31), codes biased to unsigned nibbles u = e + bias:
//     P0 byte i = u[i] | u[4+i] << 4,    P1 byte i = u[8+i] | u[12+i] << 4        (i = 0..3)
// so that `P & 0x0f0f0f0f` and `(P >> 4) & 0x0f0f0f0f` ARE the four dwords of an int8 MFMA operand (16 consecutive k):
// wanq_gemm_w4a8 reads 16 packed bytes per lane from LDS and gets two MFMA operands for six VALU instructions.
__device__ __forceinline__ uint32_t w4_nibbles(uint32_t d, uint32_t flip) { return (d ^ flip) & 0x0f0f0f0fu; }

__global__ __launch_bounds__(256) void pack_w4_kernel(const int8_t* q, uint8_t* packed, int bias, int64_t total32) {
  const uint32_t flip = bias ? 0x08080808u : 0u;  // low nibble of (e + 8) = low nibble of e with bit 3 flipped
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total32; i += (int64_t)gridDim.x * 256) {
    const uint4 a = *reinterpret_cast<const uint4*>(q + i * 32), b = *reinterpret_cast<const uint4*>(q + i * 32 + 16);
    uint4 o;
    o.x = w4_nibbles(a.x, flip) | (w4_nibbles(a.y, flip) << 4);
    o.y = w4_nibbles(a.z, flip) | (w4_nibbles(a.w, flip) << 4);
    o.z = w4_nibbles(b.x, flip) | (w4_nibbles(b.y, flip) << 4);
    o.w = w4_nibbles(b.z, flip) | (w4_nibbles(b.w, flip) << 4);
    *reinterpret_cast<uint4*>(packed + i * 16) = o;
  }
}

__device__ __forceinline__ uint32_t w4_to_i8(uint32_t u4, int bias) {  // four unsigned nibbles (one per byte) -> int8 codes u - bias
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) r |= (uint32_t)(((int)((u4 >> (8 * b)) & 0xf) - bias) & 0xff) << (8 * b);
  return r;
}

__global__ __launch_bounds__(256) void unpack_w4_kernel(const uint8_t* packed, int8_t* q, int bias, int64_t total32) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total32; i += (int64_t)gridDim.x * 256) {
    const uint4 p = *reinterpret_cast<const uint4*>(packed + i * 16);
    const uint32_t m = 0x0f0f0f0fu;
    *reinterpret_cast<uint4*>(q + i * 32) =
        make_uint4(w4_to_i8(p.x & m, bias), w4_to_i8((p.x >> 4) & m, bias), w4_to_i8(p.y & m, bias), w4_to_i8((p.y >> 4) & m, bias));
    *reinterpret_cast<uint4*>(q + i * 32 + 16) =
        make_uint4(w4_to_i8(p.z & m, bias), w4_to_i8((p.z >> 4) & m, bias), w4_to_i8(p.w & m, bias), w4_to_i8((p.w >> 4) & m, bias));
  }
}

extern "C" int wanq_pack_w4(const int8_t* q, uint8_t* packed, int bias, int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(q && packed, WANQ_E_ARG, "wanq_pack_w4: NULL pointer");
  WANQ_REQUIRE(cols >= 32 && cols % 32 == 0, WANQ_E_SHAPE, "wanq_pack_w4: cols=%d must be a multiple of 32", cols);
  WANQ_REQUIRE(rows >= 0 && (bias == 0 || bias == 8), WANQ_E_ARG, "wanq_pack_w4: bias must be 0 (unsigned codes) or 8 (signed codes)");
  const int64_t total32 = rows * (cols / 32);
  if (total32 == 0) return WANQ_OK;
  const unsigned grid = (unsigned)((total32 + 255) / 256 < 4096 ? (total32 + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_w4_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, q, packed, bias, total32);
  return check_launch("wanq_pack_w4");
}

extern "C" int wanq_unpack_w4(const uint8_t* packed, int8_t* q, int bias, int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(q && packed, WANQ_E_ARG, "wanq_unpack_w4: NULL pointer");
  WANQ_REQUIRE(cols >= 32 && cols % 32 == 0, WANQ_E_SHAPE, "wanq_unpack_w4: cols=%d must be a multiple of 32", cols);
  WANQ_REQUIRE(rows >= 0 && (bias == 0 || bias == 8), WANQ_E_ARG, "wanq_unpack_w4: bias must be 0 (unsigned codes) or 8 (signed codes)");
  const int64_t total32 = rows * (cols / 32);
  if (total32 == 0) return WANQ_OK;
  const unsigned grid = (unsigned)((total32 + 255) / 256 < 4096 ? (total32 + 255) / 256 : 4096);
  hipLaunchKernelGGL(unpack_w4_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, packed, q, bias, total32);
  return check_launch("wanq_unpack_w4");
}