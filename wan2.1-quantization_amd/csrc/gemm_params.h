// What the int8 GEMM kernels share (gemm_w8a8.hip: v1 and persistent v2; gemm_w8a8_pp.hip: ping-pong v3), and the 16-bit GEMMs
// with them: the launch parameters and the epilogue helpers that convert four outputs and load four per-channel values.  The
// int8 kernels' tile walk and the persistent pair's tile rules are in gemm_i8_common.h.
#pragma once
#include "wanq_common.h"

namespace wanq {

struct GemmParams {
  const int8_t* a;
  const int8_t* w;
  void* out;
  const void* sa;
  const void* asum;
  const void* sw;
  const void* bias;
  const void* zp;
  const float* gate;
  const void* residual;
  int tok_dtype, ch_dtype, zp_dtype, epi;
  int M, N, K;
  int mt, nt;
  int group_m;  // persistent kernels: m-tiles per L2 panel
};

template <int OUT>
__device__ __forceinline__ uint2 pack16x4(const float (&y)[4]) {
  uint2 v;
  if (OUT == WANQ_F16) {
    // the fp32 value first, then its cast (the reference's order, w8a8_gemm_cuda.cu:416-442): without the opaque copies hipcc may
    // contract the last fma and the cast into v_fma_mixlo_f16 -- one rounding instead of two, a different half in rare cases, and
    // which of the two a kernel gets depends on the code around it
    float z[4] = {y[0], y[1], y[2], y[3]};
    asm volatile("" : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]));
    __half2* h = reinterpret_cast<__half2*>(&v);
    h[0] = __floats2half2_rn(z[0], z[1]);
    h[1] = __floats2half2_rn(z[2], z[3]);
  } else {
    uint16_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const __hip_bfloat16 t = __float2bfloat16(y[j]);
      b[j] = *reinterpret_cast<const uint16_t*>(&t);
    }
    v = make_uint2((uint32_t)b[0] | ((uint32_t)b[1] << 16), (uint32_t)b[2] | ((uint32_t)b[3] << 16));
  }
  return v;
}

__device__ __forceinline__ void load4_ch(const void* p, int dt, int idx, float (&o)[4]) {
  if (dt == WANQ_F32) {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + idx);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else if (dt == WANQ_F16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const __half*>(p) + idx);
    const __half2* h = reinterpret_cast<const __half2*>(&v);
    const float2 a = __half22float2(h[0]), b = __half22float2(h[1]);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
  } else {  // WANQ_I16
    const short4 v = *reinterpret_cast<const short4*>(static_cast<const short*>(p) + idx);
    o[0] = (float)v.x; o[1] = (float)v.y; o[2] = (float)v.z; o[3] = (float)v.w;
  }
}

// gemm_w8a8_pp.hip -- the ping-pong persistent kernel (W8 operands, M >= 512, K % 128 == 0, K >= 256; fp16 / bf16 / fp32 / int32
// output; gate + residual with an fp32 output only).  `eligible` says whether a problem may take it; `launch` fills mt / nt itself.
bool gemm_pp_eligible(const GemmParams& p, int out_dtype, bool w4);
int launch_gemm_pp(const GemmParams& p, int out_dtype, hipStream_t st);

}  // namespace wanq
