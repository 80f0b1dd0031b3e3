// fp8 (OCP e4m3fn) W8A8 GEMM: per-token dynamic e4m3 activations against per-channel e4m3 weights (HipLinearFp8), with the fused
// epilogue of the 16-bit GEMMs:
//   acc[m,n] = sum_k a[m,k] w[n,k]  on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands, unit block scales), fp32 accumulation
//   y = fmaf(acc * sa[m], sw[n], bias[n]);  GELU;  residual + y * gate;  one rounding to out  (epilogue16<.., TOKEN>).
//
// Structure, the K loop (gemm_tile_kernel), operand roles and determinism: gemm16_common.h.  An fp8 row of a K-tile is half the bytes
// of a bf16 row, so a K-tile here is 128 deep and the LDS image is the bf16 kernel's byte for byte.
//
// Matrix instruction.  The block-scaled 16x16x128 MFMA with both formats e4m3 and both scales 2^0 (E8M0 127) multiplies plain fp8
// at twice the rate of v_mfma_f32_16x16x32_fp8_fp8 (which runs at the bf16 rate): one MFMA per 16 x 16 block and K-tile instead of
// four.  Both forms passed the operand-map and integer probes of tests/test_gpu_fp8.py; this one measured faster on both FFN
// shapes (profiles/gemm_fp8.txt) and is the one kept.
//
// Fragments.  The MFMA takes 32 bytes per lane and operand: lane l, row l & 15, 32 k of lane group l >> 4.  A lane keeps the bf16
// kernel's two 16-byte reads -- logical chunk 4 kk + fq of the 64-deep step kk = 0, 1, fq = l >> 4 -- as the low and the high half of
// its fragment.  Both operands are cut the same way, so slot j of lane group fq holds the same k on either side, whichever k the
// hardware calls it.  Per K-tile: 16 reads, 16 MFMAs.  K % 64 == 0: when K % 128 == 64 the last tile's second step is read from the
// first step's addresses and replaced by zeros in both fragments (+0 products: the sum is that of the 64 real k).
//
// Summation order of element (m, n): K-tiles ascending, inside an MFMA the hardware's own.  It depends on K only.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int KSTEP8 = 64;  // the K multiple: one 16-byte fragment read per lane, half of an MFMA's K

// one 128-deep MFMA: the fragments of step 0 (low 16 bytes) and step 1 (high 16 bytes); e4m3 x e4m3, scales 2^0
__device__ __forceinline__ v4f mfma128(const v4i& w0, const v4i& w1, const v4i& x0, const v4i& x1, v4f c) {
  const v8i w = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w}, x = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

template <int OUT_>
struct Fp8Policy {
  static constexpr int OUT = OUT_, TKE = 128, KMUL = KSTEP8, WROW = TROW, XROW = TROW;
  static constexpr bool SCALED = true, TOKEN = true;
  using Side = NoSide;

  // a half-deep last tile (K % 128 == 64): zeros for the second step of both fragments, inside the one MFMA
  static __device__ __forceinline__ void mma(v4f (&acc)[4][4], const v4i (&wb)[2][4], const v4i (&xa)[2][4], const Side&,
                                             bool half) {
    const v4i z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma128(wb[0][j], half ? z : wb[1][j], xa[0][i], half ? z : xa[1][i], acc[i][j]);
  }
};

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_fp8(const uint8_t* a, const uint8_t* w, const float* sa, const float* sw, void* out, int out_dtype,
                             const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M,
                             int N, int K, void* stream) {
  const char* what = "wanq_gemm_fp8";
  WANQ_REQUIRE(a && w && out && sa && sw, WANQ_E_ARG, "%s: a, w, sa, sw and out must be non-NULL", what);
  if (const int rc = check_gemm16_shapes(what, KSTEP8, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  WANQ_REQUIRE(aligned(sw, 16) && aligned(sa, 4), WANQ_E_ARG, "%s: sw must be 16-byte aligned and sa 4-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const Gemm16Params p = gemm16_params(a, w, sa, sw, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  return with_out_dtype(out_dtype, [&](auto o) {
    return launch_tiles(gemm_tile_kernel<Fp8Policy<decltype(o)::value>>, p, (hipStream_t)stream, what);
  });
}
