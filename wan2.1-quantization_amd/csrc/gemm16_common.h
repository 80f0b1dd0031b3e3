// What the two 16-bit GEMM kernels share (gemm_bf16.hip: floating-point weights; gemm_wq16.hip: integer weight codes): the tile
// geometry, the token half of a K-tile in LDS, the MFMA fragment addresses, the fp32 epilogue and the argument rules of the two
// extern "C" entries.  The fp8 GEMM (gemm_fp8.hip) is built on the same geometry, fragment addresses, epilogue and argument rules,
// with a K-tile of 128 one-byte elements in the same 128-byte LDS rows.
//
// Structure.  One 128(M) x 128(N) output tile per 256-thread workgroup (4 waves, 2 x 2, 64 x 64 each = 4 x 4 MFMA tiles), K in
// tiles of 64.  The token half of a K-tile (128 rows of 128 B) is copied global -> LDS by LDS-DMA (global_load_lds_dwordx4, 4 per
// wave) into one of two buffers; rows are 128 B with the 16-B chunk index XORed with (row >> 1) & 7, on the DMA source address and
// on the fragment reads (the LDS image of gemm_w8a8_pp.hip: a 16x16x32 bf16 fragment takes the same 16 bytes per lane as a
// 16x16x64 int8 one).  The MFMA takes the WEIGHT fragment as its A operand and the token fragment as B, so a lane's four
// accumulators are four consecutive channels of one token: bias / gate loads and the stores are 4-wide vectors.
//
// Determinism.  Every output element is summed by one lane, over k in K-tile order and within a tile in two 32-deep MFMA steps
// with the same k -> fragment-slot assignment in both kernels: its fp32 summation order depends on K only -- not on M, on the
// row's place in the launch or on which workgroup ran it.  No split-K, one kernel form each.  Rows past M are read from row M - 1
// (computed, never stored); channels past N likewise.
#pragma once
#include "gemm_params.h"

namespace wanq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

constexpr int TM = 128, TN = 128, TK = 64;
constexpr int TROW = TK * 2;  // bytes of one LDS row

template <int OFF>
__device__ __forceinline__ void dsr(v4i& d, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

template <bool F16IN>
__device__ __forceinline__ v4f mfma(const v4i& a, const v4i& b, const v4f& c) {
  if constexpr (F16IN) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
  }
}

// four consecutive per-channel values of dtype F16 / BF16 / F32
__device__ __forceinline__ void load4_any(const void* p, int dt, int idx, float (&o)[4]) {
  if (dt == WANQ_BF16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + idx);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
    load4_ch(p, dt, idx, o);
  }
}

template <int OUT>
__device__ __forceinline__ void load4_out(const void* p, int64_t idx, float (&o)[4]) {
  if constexpr (OUT == WANQ_F32) {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + idx);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    load4_any(static_cast<const uint16_t*>(p) + idx, OUT, 0, o);
  }
}

template <int OUT>
__device__ __forceinline__ void store4_out(void* p, int64_t idx, const float (&y)[4]) {
  if constexpr (OUT == WANQ_F32) {
    *reinterpret_cast<float4*>(static_cast<float*>(p) + idx) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
    *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p) + idx) = pack16x4<OUT>(y);
  }
}

// LDS-DMA sources of the token rows: instruction q (0-3) of this wave fills LDS rows 8 g .. 8 g + 7, g = 4 q + wave; lane l writes
// row 8 g + (l >> 3), physical chunk l & 7 = logical chunk c ^ ((row >> 1) & 7).  src[q] points at k = 0 of that chunk.
__device__ __forceinline__ void token_dma_sources(const uint16_t* a, int m0, int M, int K, int wave, int lane,
                                                  const uint16_t* (&src)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + wave) + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int m = m0 + r < M ? m0 + r : M - 1;
    src[q] = a + (int64_t)m * K + c * 8;
  }
}

// fragment reads: lane l reads row (16-row block) + fr, fr = l & 15, logical chunk 4 kk + fq, fq = l >> 4, of the 32-deep step kk
__device__ __forceinline__ uint32_t frag_addr(uint32_t lds0, int fr, int fq, int kk) {
  return lds0 + fr * TROW + (((4 * kk + fq) ^ ((fr >> 1) & 7)) << 4);
}

// acc[token block i][channel block j]: channel (lane >> 4) * 4 + e, token lane & 15
__device__ __forceinline__ void zero_acc(v4f (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
}

// epilogue, fp32: acc + bias, or with SCALED acc * sw + bias in one fma, or with TOKEN (gemm_fp8.hip) (acc * sa[m]) * sw + bias, the
// per-token factor first and then one fma; GELU; residual + y * gate; one rounding to OUT
template <int OUT, bool SCALED, bool TOKEN = false>
__device__ __forceinline__ void epilogue16(const v4f (&acc)[4][4], int m0, int n0, int wm, int wn, int fr, int fq, int M, int N,
                                           const float* sw, const void* bias, int bias_dtype, const float* gate,
                                           const void* residual, void* out, int epi, const float* sa = nullptr) {
  static_assert(!TOKEN || SCALED, "the per-token factor comes with the per-channel one");
  const bool gelu = epi & WANQ_EPI_GELU, gres = epi & WANQ_EPI_GATE_RES;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + fq * 4;
    if (n >= N) continue;
    float s4[4], b4[4] = {0.f, 0.f, 0.f, 0.f}, g4[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SCALED) load4_ch(sw, WANQ_F32, n, s4);
    if (bias) load4_any(bias, bias_dtype, n, b4);
    if (gres) load4_ch(gate, WANQ_F32, n, g4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      if (m >= M) continue;
      const int64_t o = (int64_t)m * N + n;
      float y[4];
      float sm = 1.f;
      if constexpr (TOKEN) sm = sa[m];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (TOKEN) y[e] = __fmaf_rn(acc[i][j][e] * sm, s4[e], b4[e]);
        else if constexpr (SCALED) y[e] = __fmaf_rn(acc[i][j][e], s4[e], b4[e]);
        else y[e] = acc[i][j][e] + b4[e];
      }
      if (gelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = gelu_tanh_fast_f32(y[e]);
      }
      if (gres) {
        float r4[4];
        load4_out<OUT>(residual, o, r4);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = r4[e] + y[e] * g4[e];
      }
      store4_out<OUT>(out, o, y);
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The argument rules both entries share, in the order they are refused, in two parts: an entry checks its non-NULL operands and the
// operand dtype itself, calls check_gemm16_shapes, and after any alignment rule of its own check_gemm16_tail.  `kmul`: the entry's
// K multiple.
inline int check_gemm16_shapes(const char* what, int kmul, const void* a, const void* w, const void* out, int out_dtype,
                               const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M,
                               int N, int K) {
  WANQ_REQUIRE(is_fp(out_dtype), WANQ_E_ARG, "%s: out dtype %d must be BF16, F16 or F32", what, out_dtype);
  WANQ_REQUIRE(!bias || is_fp(bias_dtype), WANQ_E_ARG, "%s: bias dtype %d must be BF16, F16 or F32", what, bias_dtype);
  WANQ_REQUIRE((epi_flags & ~(WANQ_EPI_GELU | WANQ_EPI_GATE_RES)) == 0, WANQ_E_ARG, "%s: unknown epilogue flag", what);
  WANQ_REQUIRE(!(epi_flags & WANQ_EPI_GATE_RES) || (gate && residual), WANQ_E_ARG, "%s: WANQ_EPI_GATE_RES needs gate and residual",
               what);
  WANQ_REQUIRE(M >= 0 && M < (1ll << 31) - TM, WANQ_E_SHAPE, "%s: M=%lld out of range", what, (long long)M);
  WANQ_REQUIRE(N >= 8 && N % 8 == 0, WANQ_E_SHAPE, "%s: N=%d must be a positive multiple of 8", what, N);
  WANQ_REQUIRE(K >= kmul && K % kmul == 0, WANQ_E_SHAPE, "%s: K=%d must be a positive multiple of %d", what, K, kmul);
  WANQ_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(out, 16) && aligned(residual, 16), WANQ_E_ARG,
               "%s: a, w, out and residual must be 16-byte aligned", what);
  return WANQ_OK;
}

// (the tile-count limit stands before the entries' M == 0 return here; no tiles pass it)
inline int check_gemm16_tail(const char* what, const void* bias, int bias_dtype, const float* gate, int64_t M, int N) {
  WANQ_REQUIRE(aligned(gate, 16) && (!bias || aligned(bias, bias_dtype == WANQ_F32 ? 16 : 8)), WANQ_E_ARG,
               "%s: gate and bias must be aligned to 4 elements", what);
  WANQ_REQUIRE(((M + TM - 1) / TM) * (((int64_t)N + TN - 1) / TN) < (1ll << 31), WANQ_E_SHAPE, "%s: too many tiles", what);
  return WANQ_OK;
}

}  // namespace
}  // namespace wanq
