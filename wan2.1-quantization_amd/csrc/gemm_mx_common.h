// What gemm_mx.hip and gemm_mx_mixed.hip share: the K-tile depth of the scaled MFMA, the instruction with its operand formats, and the
// loader of the E8M0 scale dwords (gemm_mx.hip's header has the fragment cut and the scale operand's place).
#pragma once
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int TKX = 128;  // elements of a K-tile: four blocks of 32, one MFMA

template <bool FP4, bool A4>
__device__ __forceinline__ v4f mfma_mx(const v4i& w0, const v4i& w1, const v4i& x0, const v4i& x1, v4f c, int sw, int sa) {
  if constexpr (A4) {
    static_assert(FP4, "e2m1 tokens go with e2m1 weights");
    const v8i w = {w0.x, w0.y, w0.z, w0.w, 0, 0, 0, 0}, x = {x0.x, x0.y, x0.z, x0.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 4, 0, sw, 0, sa);
  }
  const v8i x = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  if constexpr (FP4) {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 0, 0, sw, 0, sa);
  } else {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, sw, 0, sa);
  }
}

// scale bytes: the dword of K-tile t of this lane's four token rows and four weight rows, loaded one tile ahead and shifted to the
// lane's own block
struct MxScales {
  const uint32_t *sap[4], *swp[4];
  uint32_t sa_nxt[4], sw_nxt[4];
  int sa_cur[4], sw_cur[4], sh;

  __device__ __forceinline__ MxScales(const Gemm16Params& p, const Frame& f) : sh(8 * f.fq) {
    const int KB = p.K / 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mr = f.m0 + f.wm * 64 + i * 16 + f.fr, nr = f.n0 + f.wn * 64 + i * 16 + f.fr;
      sap[i] = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(p.sa) + (int64_t)(mr < p.M ? mr : p.M - 1) * KB);
      swp[i] = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(p.sw) + (int64_t)(nr < p.N ? nr : p.N - 1) * KB);
    }
  }
  __device__ __forceinline__ void load(int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_nxt[i] = sap[i][t];
      sw_nxt[i] = swp[i][t];
    }
  }
  __device__ __forceinline__ void shift() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_cur[i] = (int)(sa_nxt[i] >> sh);
      sw_cur[i] = (int)(sw_nxt[i] >> sh);
    }
  }
};

}  // namespace
}  // namespace wanq
