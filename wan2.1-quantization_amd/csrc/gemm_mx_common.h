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

// Where an MX GEMM entry's own rules sit among the shared ones (mx_gemm_entry)
enum MxRulesAt {
  MX_BEFORE_SHAPES,    // w_fmt; the branch's t, b and dtype16
  MX_AFTER_SHAPES,     // R and ldt; n8
  MX_AFTER_ALIGNMENT,  // the branch's alignment
};

// The host front of every MX GEMM entry, in the order the ABI tests pin: non-NULL operands, the entry's rules before the shapes, the
// shared shape rules with K a multiple of TKX, its rules after them, the scale alignment, its rules after that, the tail, M == 0,
// then launch(params, stream).
template <class Rules, class Launch>
inline int mx_gemm_entry(const char* what, const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, void* out,
                         int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags,
                         int64_t M, int N, int K, void* stream, Rules rules, Launch launch) {
  WANQ_REQUIRE(a && w && out && sa_u8 && sw_u8, WANQ_E_ARG, "%s: a, w, sa_u8, sw_u8 and out must be non-NULL", what);
  if (const int rc = rules(MX_BEFORE_SHAPES)) return rc;
  if (const int rc = check_gemm16_shapes(what, TKX, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  if (const int rc = rules(MX_AFTER_SHAPES)) return rc;
  WANQ_REQUIRE(aligned(sa_u8, 4) && aligned(sw_u8, 4), WANQ_E_ARG, "%s: sa_u8 and sw_u8 must be 4-byte aligned", what);
  if (const int rc = rules(MX_AFTER_ALIGNMENT)) return rc;
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  return launch(gemm16_params(a, w, sa_u8, sw_u8, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K), (hipStream_t)stream);
}

inline int no_rules(MxRulesAt) { return WANQ_OK; }

}  // namespace
}  // namespace wanq
