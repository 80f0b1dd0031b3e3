// The per-block arithmetic of the OCP MX row quantisers, one definition for rowwise.hip (quant_rows_mx_kernel) and quant_project.hip
// (quant_project_kernel): the optional 32-point Hadamard rotation, the block maximum, the E8M0 scale byte, the exact scaling and the
// e2m1 code.  A block of 32 consecutive columns is four 8-element chunks held by four lanes; which four, and how they exchange a
// register, is the caller's layout and comes in as XL:
//   XL::x8(v)   the value of the lane that holds the chunk 8 elements away (chunk index ^ 1)
//   XL::x16(v)  ... 16 elements away (chunk index ^ 2)
// rowwise.hip: the four lanes of an aligned quad, DPP quad permutes.  quant_project.hip: lanes fr, fr + 16, fr + 32, fr + 48 of the
// MFMA's token operand layout, v_permlane16_swap / v_permlane32_swap.  The operations per element and their order are the same in
// both, so codes and scale bytes are bit-equal (mx_hadamard32_host, mx_quant_rows_host).
#pragma once
#include "wanq_common.h"

namespace wanq {

__device__ __forceinline__ uint32_t e2m1_code(float t) {
  const float a = fminf(fabsf(t), 6.0f);
  const uint32_t mag = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return mag | ((__float_as_uint(t) >> 28) & 8u);
}

// one butterfly stage inside a chunk: H = 1, 2 or 4
template <int H>
__device__ __forceinline__ void had_stage(float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j & H) continue;
    const float a = v[j], b = v[j + H];
    v[j] = a + b;
    v[j + H] = a - b;
  }
}

// the quad of rowwise.hip: chunk index = lane & 3
struct MxQuadLanes {
  static __device__ __forceinline__ float x8(float v) { return lane_xor_dpp<1>(v); }
  static __device__ __forceinline__ float x16(float v) { return lane_xor_dpp<2>(v); }
};

// one butterfly stage across the block's lanes: h = 8 (FAR false) or 16 (FAR true); the lane with the bit set keeps partner - own
template <class XL, bool FAR>
__device__ __forceinline__ void had_stage_lanes(float (&v)[8], bool upper) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float o = FAR ? XL::x16(v[j]) : XL::x8(v[j]);
    v[j] = upper ? o - v[j] : v[j] + o;
  }
}

// the five stages h = 1, 2, 4, 8, 16 of the unnormalised Sylvester-Hadamard transform of a block; c: this lane's chunk index (0-3)
template <class XL>
__device__ __forceinline__ void mx_block_hadamard(float (&v)[8], int c) {
  had_stage<1>(v);
  had_stage<2>(v);
  had_stage<4>(v);
  had_stage_lanes<XL, false>(v, c & 1);
  had_stage_lanes<XL, true>(v, c & 2);
}

// max |x| over the block, in all four lanes
template <class XL>
__device__ __forceinline__ float mx_block_amax(const float (&v)[8]) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  m = fmaxf(m, XL::x8(m));
  m = fmaxf(m, XL::x16(m));
  return m;
}

// s = clamp(E(amax) - emax, 0, 254)
template <int EMAX>
__device__ __forceinline__ int mx_block_scale(float amax) {
  const int s = (int)((__float_as_uint(amax) >> 23) & 0xffu) - EMAX;
  return s < 0 ? 0 : (s > 254 ? 254 : s);
}

// t = x 2^(127 - s), exact
__device__ __forceinline__ void mx_block_scaled(const float (&v)[8], int s, float (&t)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = ldexpf(v[j], 127 - s);
}

// eight e2m1 codes of a scaled chunk as one dword, even k in the low nibble
__device__ __forceinline__ uint32_t e2m1_pack8(const float (&t)[8]) {
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w |= e2m1_code(t[j]) << (4 * j);
  return w;
}

// ---- the block-scale rule `search` of e2m1 (wanq_quant_rows_mx4_search; host: mx_quant_rows_host(search=True)) ----------------------
// OCP's byte s0 puts the block maximum in [4, 8) and e2m1 ends at 6: (6, 8) clips.  s0 + 1 puts it in [2, 4), where nothing clips and
// the small elements get twice the step.  Both are legal; the block takes the one with the smaller squared reconstruction error.

// e2m1_code(t) and, in d, the residual |t| - |value(code)| (exact in fp32: both are multiples of ulp(t) and |d| <= |t|).
// a = min(|t|, 6) lies in [0, 2), [2, 4) or [4, 8), where neighbouring codes are q = 1/2, 1, 2 apart; b = 2^floor(log2(max(a, 1))) = 2 q.
// With C = 1.5 * 2^23 * q (ulp(C) = q, bits of b + 22 exponent steps + the mantissa's top bit) the sum a + C is a rounded to a multiple
// of q, to nearest, ties to the even multiple -- at each of the seven midpoints (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5) the even multiple
// is the even code, so this is e2m1_code's rounding -- and its low mantissa bits are that multiple r: the magnitude code is r + 0, 2, 4.
__device__ __forceinline__ uint32_t e2m1_code_residual(float t, float& d) {
  const float a = fminf(fabsf(t), 6.0f);
  const uint32_t b = __float_as_uint(fmaxf(a, 1.0f)) & 0x7f800000u;
  const float C = __uint_as_float(b + 0x0b400000u);
  const float u = a + C;
  d = fabsf(t) - (u - C);
  return ((__float_as_uint(u) & 7u) + (b >> 22) - 254u) | ((__float_as_uint(t) >> 28) & 8u);
}

// e = sum d_i^2 over the block, in all four lanes, in fp32 in ONE order: every square rounded on its own (no fused multiply-add),
// then the butterfly tree h = 1, 2, 4 inside the chunk and h = 8, 16 across the lanes, (i, i + h) summed for bit h of i clear.  Both
// partners of an exchange add the same two numbers, so the four lanes hold the same bits.  On the host: adjacent pairs, five times.
// One candidate byte s: -> e(s) in all four lanes, and in w the chunk's eight codes.  An element is scaled, rounded, squared and folded
// into the tree as soon as its sibling is there: what a candidate needs to keep is the code dword and a few partial sums.  (The
// compiled kernel still holds about 50 VGPRs beyond the row, 68 to 126 in all against the plain kernel's 22 to 76: see
// profiles/mx4_scale_search.txt.)
template <class XL>
__device__ __forceinline__ float mx4_block_candidate(const float (&v)[8], int s, uint32_t& w) {
#pragma clang fp contract(off)
  float p[4];
  w = 0;
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    float d0, d1;
    w |= e2m1_code_residual(ldexpf(v[j], 127 - s), d0) << (4 * j);
    w |= e2m1_code_residual(ldexpf(v[j + 1], 127 - s), d1) << (4 * j + 4);
    p[j >> 1] = d0 * d0 + d1 * d1;
  }
  float e = (p[0] + p[1]) + (p[2] + p[3]);
  e = e + XL::x8(e);
  e = e + XL::x16(e);
  return e;
}

// The rule: -> the block's byte, and in w the eight e2m1 codes of this lane's chunk under it (even k in the low nibble).  Both
// candidates' codes and error sums stay in registers; s0 + 1 wins exactly when 4 e(s0 + 1) < e(s0) (the factor brings both to the
// units of s0; a tie keeps OCP's byte).  No search, and today's bits, for an all-zero block and an infinite maximum; a NaN element
// makes both sums NaN and the comparison false.  (s0 < 254 is the definition's third guard and can never fire: with emax = 2 the byte
// is at most 253, reached by an infinite maximum only.  No test can build it.)
template <class XL>
__device__ __forceinline__ int mx4_block_search(const float (&v)[8], float amax, uint32_t& w) {
  const int s0 = mx_block_scale<2>(amax);
  uint32_t w0, w1;
  const float e0 = mx4_block_candidate<XL>(v, s0, w0);
  const float e1 = mx4_block_candidate<XL>(v, s0 + 1, w1);
  const bool up = amax > 0.f && amax < __builtin_inff() && s0 < 254 && 4.0f * e1 < e0;
  w = up ? w1 : w0;
  return s0 + (up ? 1 : 0);
}

// eight e4m3fn codes of a scaled chunk as two dwords: the clamp to +-448, then the packed hardware conversion (round to nearest even,
// subnormal codes kept).  A COPY of the e4m3 branch of quant_rows_mx_kernel (rowwise.hip), which keeps its own lines so that its
// instruction stream does not move: the two must be kept in step (tests/test_gpu_mx_mixed.py holds this one to the host expression
// that tests/test_gpu_mx.py holds the other to)
__device__ __forceinline__ uint2 e4m3_pack8(const float (&t)[8]) {
  float c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = __builtin_amdgcn_fmed3f(t[j], -448.0f, 448.0f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

}  // namespace wanq
