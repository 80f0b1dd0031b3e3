// What the int8 GEMM kernels share beyond their launch parameters (gemm_params.h): the tile walk of all three kernels; the tile
// geometry, the host-side rules, the per-token scale loads and the dequantisation expression of the two persistent ones
// (gemm_w8a8.hip: gemm_w8a8_big_kernel, "v2"; gemm_w8a8_pp.hip: gemm_w8a8_pp_kernel, "pp").
// The store LOOPS of v2 and pp are twins that stay apart: v2 sits at the 256-register cap, and on pp's loops -- scales in registers
// or re-read from v2's LDS staging area through a scale-source parameter -- its floating-point forms spill (20 - 148 bytes of
// scratch against 0, a reload inside the K loop).  The experiment is kept as tools/probes/gemm_i8_shared_store_loops.patch.
#pragma once
#include "gemm_params.h"

namespace wanq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

// ---- the persistent kernels' tile
constexpr int PM = 256, PN = 256, PK = 128;
constexpr int PBUF = (PM + PN) * PK;  // one K-tile of both operands in LDS (a stage of v2, a ring buffer of pp): 64 KiB

// one workgroup per CU; % 8 == 0 so that a workgroup's tiles all sit in its own XCD's range of the walk
static inline int persistent_grid(int tiles) { return tiles < 256 ? ((tiles + 7) & ~7) : 256; }
// what both persistent kernels need of a problem: enough rows, whole K-tiles, and 32-bit byte offsets into both operands
static inline bool persistent_shape_ok(const GemmParams& p) {
  return p.M >= 512 && p.K % PK == 0 && (int64_t)p.M * p.K < (1ll << 32) && (int64_t)p.N * p.K < (1ll << 32);
}

// tile id t of ntiles -> origin (m0, n0) of a TILE x TILE output tile: XCD-contiguous ids (a bijective remap, so that each XCD's
// L2 sees a compact panel), then groups of group_m m-tiles walked m-fastest, a short last group.
// v1: t = blockIdx.x, ntiles = gridDim.x; persistent kernels: ntiles = mt * nt and t steps by gridDim.x (% 8 == 0).
template <int TILE>
__device__ __forceinline__ void tile_origin(int t, int ntiles, int mt, int nt, int group_m, int& m0, int& n0) {
  const int xq = ntiles >> 3, xr = ntiles & 7, xcd = t & 7;
  const int wg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (t >> 3);
  const int per_group = group_m * nt;
  const int group = wg / per_group;
  const int first_m = group * group_m;
  const int gsz = (mt - first_m < group_m) ? (mt - first_m) : group_m;
  const int in_g = wg - group * per_group;
  m0 = (first_m + in_g % gsz) * TILE;
  n0 = (in_g / gsz) * TILE;
}

// sA / sumA of a lane's 8 tokens tok_base + 16 j + r16 (one per token block j of the persistent kernels' accumulators), straight
// into registers; rows past M are clamped: computed, never stored.  An int32 output takes none (1, 0).
template <int OUT>
__device__ __forceinline__ void load_token_scales(const GemmParams& p, float (&sa)[8], float (&asum)[8], int tok_base, int r16) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sa[j] = 1.f;
    asum[j] = 0.f;
  }
  if (OUT == WANQ_I32) return;
  int mcl[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int mr = tok_base + j * 16 + r16;
    mcl[j] = mr < p.M ? mr : p.M - 1;
  }
  if (p.tok_dtype == WANQ_F32) {  // one uniform branch per dtype so that the eight loads of a kind issue together
#pragma unroll
    for (int j = 0; j < 8; ++j) sa[j] = static_cast<const float*>(p.sa)[mcl[j]];
    if (p.zp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) asum[j] = static_cast<const float*>(p.asum)[mcl[j]];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) sa[j] = __half2float(static_cast<const __half*>(p.sa)[mcl[j]]);
    if (p.zp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) asum[j] = __half2float(static_cast<const __half*>(p.asum)[mcl[j]]);
    }
  }
}

// Four outputs of one accumulator quad of the persistent kernels (one token, four consecutive channels):
// acc*sA*sW + (sumA*(zp*sW) + bias), then GELU.  The one place the expression is written for both kernels: their outputs are
// required to be bit-equal (tests/test_gpu_gemm.py::test_pingpong_kernel_bit_equal_to_the_other_kernels).
// PK: the same expression on channel PAIRS (v_pk_mul_f32 / v_pk_fma_f32: IEEE per half, bit-identical to the scalar form, 2.25
// instead of 4 vector instructions per value).
template <bool GELU, bool PK>
__device__ __forceinline__ void dequant4(const v4i& a, float sa, float asum, const float (&sw)[4], const float (&zs)[4], const float (&b)[4],
                                         float (&y)[4]) {
  if (PK) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f sa2 = {sa, sa}, as2 = {asum, asum};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const v2f af = {(float)a[2 * h], (float)a[2 * h + 1]};
      const v2f sw2 = {sw[2 * h], sw[2 * h + 1]}, zs2 = {zs[2 * h], zs[2 * h + 1]}, b2 = {b[2 * h], b[2 * h + 1]};
      const v2f r = __builtin_elementwise_fma(af * sa2, sw2, __builtin_elementwise_fma(as2, zs2, b2));
      y[2 * h] = r.x;
      y[2 * h + 1] = r.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = fmaf((float)a[e] * sa, sw[e], fmaf(asum, zs[e], b[e]));
  }
  if (GELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = gelu_tanh_fast_f32(y[e]);
  }
}

}  // namespace wanq
