// H += x^T x in one pass: the Hessian accumulation of the GPTQ calibration hook (wan/calib.py, fused.gram_accumulate_onepass_).
//
// x is row-major [rows, C] (bf16 / fp16) and the contraction runs over its ROWS, so both MFMA operands are x^T: lane l of
// v_mfma_f32_16x16x32 wants eight consecutive k (rows of x) of one output row / column (a column of x).  Instead of a transposed
// copy of x in memory, the transpose happens on the way into LDS: a thread fetches a 4 rows x 8 columns patch (four 16-byte loads),
// regroups it in registers into eight (column, 4 rows) runs and stores each as one 8-byte word into an image xs[column][64 rows],
// from which every operand fragment is one 16-byte read.  The image's column pitch is 144 bytes (64 rows + 16): the fragment reads of
// sixteen neighbouring columns start 36 dwords apart and cover all 64 banks once, and a half-wave's stores (sixteen row quads of two
// column octets, 288 dwords apart) fill the 32 banks twice, the minimum for 256 bytes.
//
// H is symmetric, so only the 128 x 128 tile pairs (ti <= tj) are computed, T (T + 1) / 2 workgroups for T = ceil(C / 128) instead of
// T^2.  A workgroup's four waves own the 64 x 64 quarters of its tile (4 x 4 accumulator blocks each); the next 64 rows of x are
// fetched into registers while the current ones are multiplied.  The epilogue adds an element's sum s to H[i, j] and the same s to
// H[j, i]; a diagonal tile takes i <= j only (its lower-left quarter is not even multiplied).  No atomics, no split over the rows: the
// order in which an element's products are summed is a function of `rows` alone, and each element of H is written by one lane.
#include "wanq_common.h"

namespace wanq {
namespace {

typedef int g4i __attribute__((ext_vector_type(4)));
typedef float g4f __attribute__((ext_vector_type(4)));
typedef __bf16 g8bf __attribute__((ext_vector_type(8)));
typedef _Float16 g8h __attribute__((ext_vector_type(8)));

constexpr int GT = 128;             // output tile: GT x GT
constexpr int GK = 64;              // rows of x per step
constexpr int GPITCH = GK * 2 + 16; // bytes of one column of the LDS image

template <bool F16IN>
__device__ __forceinline__ g4f gram_mfma(const g4i& a, const g4i& b, const g4f& c) {
  if constexpr (F16IN) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(g8h, a), __builtin_bit_cast(g8h, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(g8bf, a), __builtin_bit_cast(g8bf, b), c, 0, 0, 0);
}

// 16-bit element e (0..7) of a 16-byte row piece
__device__ __forceinline__ uint32_t half_of(const uint4& r, int e) {
  const uint32_t w = (e >> 1) == 0 ? r.x : (e >> 1) == 1 ? r.y : (e >> 1) == 2 ? r.z : r.w;
  return (e & 1) ? (w >> 16) : (w & 0xffffu);
}

template <bool F16IN>
__global__ __launch_bounds__(256) void gram_kernel(const uint16_t* __restrict__ x, float* H, int64_t rows, int C, int T) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * GT * GPITCH];  // columns of tile row ti, then of tile column tj
  int b = blockIdx.x, ti = 0;  // the b-th pair (ti <= tj) in row-major order
  while (b >= T - ti) {
    b -= T - ti;
    ++ti;
  }
  const int tj = ti + b, i0 = ti * GT, j0 = tj * GT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const bool idle = ti == tj && wm > wn;  // the quarter below a diagonal tile's diagonal

  // staging: this thread's patch is rows 4 q .. 4 q + 3 of the step, columns 8 c .. 8 c + 7 of either block
  const int q = t & 15, c = t >> 4;
  const int ca = i0 + 8 * c, cb = j0 + 8 * c;
  const bool va = ca < C, vb = cb < C;  // (C is a multiple of 8: an octet of columns is inside or outside as a whole)
  uint4 ra[4], rb[4];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = r0 + 4 * q + i;
      const bool in = r < rows;  // rows past the end enter as zeros
      ra[i] = (in && va) ? *reinterpret_cast<const uint4*>(x + r * C + ca) : make_uint4(0, 0, 0, 0);
      rb[i] = (in && vb) ? *reinterpret_cast<const uint4*>(x + r * C + cb) : make_uint4(0, 0, 0, 0);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint2 a = make_uint2(half_of(ra[0], e) | (half_of(ra[1], e) << 16), half_of(ra[2], e) | (half_of(ra[3], e) << 16));
      const uint2 bb = make_uint2(half_of(rb[0], e) | (half_of(rb[1], e) << 16), half_of(rb[2], e) | (half_of(rb[3], e) << 16));
      *reinterpret_cast<uint2*>(xs + (8 * c + e) * GPITCH + 8 * q) = a;
      *reinterpret_cast<uint2*>(xs + (GT + 8 * c + e) * GPITCH + 8 * q) = bb;
    }
  };

  g4f acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[a][n] = g4f{0.f, 0.f, 0.f, 0.f};

  const unsigned char* pa = xs + (wm * 64 + fr) * GPITCH + fq * 16;         // A: H's rows = columns i0 + .. of x
  const unsigned char* pb = xs + (GT + wn * 64 + fr) * GPITCH + fq * 16;    // B: H's columns = columns j0 + .. of x
  fetch(0);
  for (int64_t r0 = 0; r0 < rows; r0 += GK) {
    __syncthreads();  // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (r0 + GK < rows) fetch(r0 + GK);  // in flight under the MFMAs
    if (!idle) {
#pragma unroll
      for (int kk = 0; kk < GK / 32; ++kk) {
        g4i fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          fa[a] = *reinterpret_cast<const g4i*>(pa + a * 16 * GPITCH + kk * 64);
          fb[a] = *reinterpret_cast<const g4i*>(pb + a * 16 * GPITCH + kk * 64);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[a][n] = gram_mfma<F16IN>(fa[a], fb[n], acc[a][n]);
      }
    }
  }
  if (idle) return;  // (behind the last barrier)

  // lane (fr, fq) holds, of block (a, n), H[gi0 + 0 .. 3][gj]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int gi0 = i0 + wm * 64 + a * 16 + fq * 4, gj = j0 + wn * 64 + n * 16 + fr;
      if (gi0 >= C || gj >= C) continue;  // (gi0 is a multiple of 4 and C of 8: the four rows are inside or outside together)
      const g4f v = acc[a][n];
      if (ti != tj) {  // every element lies above the diagonal: the four mirrors are one 16-byte run of row gj
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* p = H + (int64_t)(gi0 + r) * C + gj;
          *p = *p + v[r];
        }
        float4* m = reinterpret_cast<float4*>(H + (int64_t)gj * C + gi0);
        float4 o = *m;
        o.x = o.x + v[0];
        o.y = o.y + v[1];
        o.z = o.z + v[2];
        o.w = o.w + v[3];
        *m = o;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = gi0 + r;
          if (gi > gj) continue;
          float* p = H + (int64_t)gi * C + gj;
          *p = *p + v[r];
          if (gi != gj) {
            float* m = H + (int64_t)gj * C + gi;
            *m = *m + v[r];
          }
        }
      }
    }
  }
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gram_accumulate(const void* x, int x_dtype, float* H, int64_t rows, int C, void* stream) {
  const char* what = "wanq_gram_accumulate";
  WANQ_REQUIRE(x && H, WANQ_E_ARG, "%s: x and H must be non-NULL", what);
  WANQ_REQUIRE(x_dtype == WANQ_BF16 || x_dtype == WANQ_F16, WANQ_E_ARG, "%s: x_dtype=%d must be bf16 or fp16", what, x_dtype);
  WANQ_REQUIRE(rows >= 0, WANQ_E_SHAPE, "%s: rows=%lld must not be negative", what, (long long)rows);
  WANQ_REQUIRE(C >= 8 && C % 8 == 0 && C <= 65536, WANQ_E_SHAPE, "%s: C=%d must be a multiple of 8 in 8..65536", what, C);
  WANQ_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)H % 16 == 0, WANQ_E_ARG, "%s: x and H must be 16-byte aligned", what);
  if (rows == 0) return WANQ_OK;
  const int T = (C + GT - 1) / GT;
  const dim3 grid((unsigned)(T * (T + 1) / 2));
  if (x_dtype == WANQ_F16)
    gram_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(static_cast<const uint16_t*>(x), H, rows, C, T);
  else
    gram_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(static_cast<const uint16_t*>(x), H, rows, C, T);
  return check_launch(what);
}
