// bf16 / fp16 GEMM with the int8 GEMM's fused epilogue, for the Linears a quant config keeps floating point (HipLinearFp):
//   y[m,n] = sum_k a[m,k] w[n,k]  on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation
//   y = y + bias[n];  y = gelu_tanh(y) (WANQ_EPI_GELU);  y = residual[m,n] + y * gate[n] (WANQ_EPI_GATE_RES);  one rounding to out.
//
// Structure, the K loop (gemm_tile_kernel), operand roles and determinism: gemm16_common.h.  Here a K-tile is 64 deep: two 32-deep
// MFMA steps, 16 fragment reads and 32 MFMAs.  K % 32 == 0: when K % 64 == 32 the last tile's second step is read from the first
// step's addresses and its MFMAs are SKIPPED (gemm_fp8.hip multiplies zeros instead; the two are not the same operation).
#include "gemm16_common.h"

namespace wanq {
namespace {

template <bool F16IN, int OUT_>
struct FpPolicy {
  static constexpr int OUT = OUT_, TKE = TK, KMUL = 32, WROW = TROW, XROW = TROW;
  static constexpr bool SCALED = false, TOKEN = false;
  using Side = NoSide;

  static __device__ __forceinline__ void mma(v4f (&acc)[4][4], const v4i (&wb)[2][4], const v4i (&xa)[2][4], const Side&,
                                             bool half) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma<F16IN>(wb[0][j], xa[0][i], acc[i][j]);
    if (!half) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma<F16IN>(wb[1][j], xa[1][i], acc[i][j]);
    }
  }
};

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_bf16(const void* a, const void* w, int dtype, void* out, int out_dtype, const void* bias, int bias_dtype,
                              const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_bf16";
  WANQ_REQUIRE(a && w && out, WANQ_E_ARG, "%s: a, w and out must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  if (const int rc = check_gemm16_shapes(what, 32, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const Gemm16Params p = gemm16_params(a, w, nullptr, nullptr, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  hipStream_t st = (hipStream_t)stream;
  return with_out_dtype(out_dtype, [&](auto o) {
    constexpr int OUT = decltype(o)::value;
    return dtype == WANQ_F16 ? launch_tiles(gemm_tile_kernel<FpPolicy<true, OUT>>, p, st, what)
                             : launch_tiles(gemm_tile_kernel<FpPolicy<false, OUT>>, p, st, what);
  });
}
