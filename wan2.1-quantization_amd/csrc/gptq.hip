// The GPTQ weight solver (Frantar et al., 2022) for the integer Linears: PTQ-time kernels, once per layer.
//
// GPTQ keeps the grid (delta, zero point) of the round-to-nearest quantiser and changes only which code a weight gets: columns
// are quantised in order, and each column's error, scaled by the upper Cholesky factor u of H^-1, is pushed onto the columns
// that are still free.  Two entries carry the loop of qdiff/base/gptq.py:
//   wanq_gptq_block      columns c0 .. c0+cols-1 (cols <= 128), one after the other, the update kept inside the block;
//   wanq_gptq_block_gidx the same block with a group per COLUMN (g_idx; act_order: the columns are a permutation of the input
//                        channels, so neighbours lie in arbitrary groups);
//   wanq_gptq_propagate  the block's errors applied to every column behind it, w[:, k] -= err . u[c0 .. c0+cols, k].
//
// Arithmetic.  Every operation is a single fp32 IEEE operation, rounded once and never contracted (the file is compiled with fp
// contract off; true divisions), and the propagation sums over i ascending from 0: the host model (gptq_solve_host, torch on the
// CPU, one torch operation per step) performs the same operations in the same order, so the two agree bit for bit on any input.
//
// wanq_gptq_block: one wave64 per weight row, the block's 128 columns two per lane in registers (lane l: columns c0 + 2l and
// c0 + 2l + 1).  Step j reads the column's value, delta and zero point from lane j / 2 (v_readlane: wave-uniform), computes code
// and error redundantly in every lane, and each lane updates its own two columns with u[j, :].  The 128 steps of a row are one
// dependent chain, so what matters is the latency of a step, not bandwidth.  u[c0 .. c0+cols, c0 .. c0+128] is kept as a 64 KiB
// LDS image shared by the workgroup's eight waves: a step's row is one conflict-free ds_read_b64 per lane (consecutive float2)
// plus a broadcast read of the diagonal, at LDS latency, and the image is fetched from L2 once per eight rows; the cached form
// would send every wave through the vector memory path for the same 64 KiB (512 B per step) at several times the latency per
// step.  Two workgroups fit a CU's 160 KiB.  Rows are independent: no atomics, no traffic between waves after the fill.
//
// wanq_gptq_block_gidx is the same kernel with a (delta, zero point) pair for each of a lane's two columns, fetched through the
// column's entry of g_idx (clamped into 0 .. G-1): step j reads the pair of its own column, so no pair of columns has to share a
// group and c0 may be odd.  The steps themselves are shared, operation for operation.
#include "wanq_common.h"

// no a * b + c of this file becomes an fma (hipcc contracts by default, and the __fmul_rn / __fadd_rn spellings do not stop it:
// they are inline functions of a header compiled with contraction on)
#pragma clang fp contract(off)

namespace wanq {
namespace {

constexpr int GPTQ_COLS = 128;  // columns of one block: two per lane
constexpr int GPTQ_WAVES = 8;   // rows per workgroup

struct GptqStep {
  float q, what, e;
};

// code, dequantised value and scaled error of one column value x (all wave-uniform)
__device__ __forceinline__ GptqStep gptq_step(float x, float d, float z, float qmin, float qmax, float ujj) {
  GptqStep s;
  s.q = fminf(fmaxf(rintf(x / d) - z, qmin), qmax);
  s.what = (s.q + z) * d;
  s.e = (x - s.what) / ujj;
  return s;
}

__device__ __forceinline__ float lane_read(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// GIDX: the group of a column is its entry of g_idx (group_size unused); else the group of column k is k / group_size (0: one per row)
template <bool GIDX>
__global__ __launch_bounds__(GPTQ_WAVES * 64) void gptq_block_kernel(float* w, int64_t w_stride, const float* u, int64_t u_stride,
                                                                      const float* delta, const float* zp, const int32_t* g_idx,
                                                                      int group_size, int groups, float qmin, float qmax,
                                                                      int8_t* codes, float* err, int64_t N, int K, int c0, int cols) {
  __shared__ float us[GPTQ_COLS * GPTQ_COLS];
  // the image: us[j][k] = u[c0 + j, c0 + k] for j, k < cols, zero elsewhere (a column past the block is never moved)
  for (int idx = threadIdx.x; idx < GPTQ_COLS * GPTQ_COLS; idx += GPTQ_WAVES * 64) {
    const int j = idx / GPTQ_COLS, k = idx % GPTQ_COLS;
    us[idx] = (j < cols && k < cols) ? u[(int64_t)(c0 + j) * u_stride + c0 + k] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * GPTQ_WAVES + wave;
  if (row >= N) return;  // (behind the workgroup's only barrier)
  const int l0 = 2 * lane, l1 = l0 + 1;
  const bool v0 = l0 < cols, v1 = l1 < cols;
  float* wr = w + row * w_stride + c0;
  float x0 = v0 ? wr[l0] : 0.f, x1 = v1 ? wr[l1] : 0.f;
  float d0, z0, d1, z1;  // the grid of the lane's first and of its second column
  if constexpr (GIDX) {
    // a column's group is its entry of the map, clamped into 0 .. groups-1 (a bad map still reads inside delta / zp); a lane
    // without a column reads the block's first column's
    const int g0 = min(max(g_idx[c0 + (v0 ? l0 : 0)], 0), groups - 1), g1 = min(max(g_idx[c0 + (v1 ? l1 : 0)], 0), groups - 1);
    d0 = delta[row * groups + g0], z0 = zp[row * groups + g0];
    d1 = delta[row * groups + g1], z1 = zp[row * groups + g1];
  } else {
    // both columns of a lane lie in one group (checked on the host); a lane without columns reads the block's first group
    const int64_t p = row * groups + (group_size ? (c0 + (v0 ? l0 : 0)) / group_size : 0);
    d1 = d0 = delta[p], z1 = z0 = zp[p];
  }
  float q0 = 0.f, q1 = 0.f, e0 = 0.f, e1 = 0.f;
  for (int jp = 0; 2 * jp < cols; ++jp) {
    {  // column j = 2 jp: lane jp's first
      const int j = 2 * jp;
      const GptqStep s = gptq_step(lane_read(x0, jp), lane_read(d0, jp), lane_read(z0, jp), qmin, qmax, us[j * GPTQ_COLS + j]);
      const float2 ur = *reinterpret_cast<const float2*>(&us[j * GPTQ_COLS + l0]);
      if (lane > jp) x0 = x0 - s.e * ur.x;
      if (lane >= jp) x1 = x1 - s.e * ur.y;
      if (lane == jp) {
        x0 = s.what;
        q0 = s.q;
        e0 = s.e;
      }
    }
    if (2 * jp + 1 < cols) {  // column j = 2 jp + 1: lane jp's second
      const int j = 2 * jp + 1;
      const GptqStep s = gptq_step(lane_read(x1, jp), lane_read(d1, jp), lane_read(z1, jp), qmin, qmax, us[j * GPTQ_COLS + j]);
      const float2 ur = *reinterpret_cast<const float2*>(&us[j * GPTQ_COLS + l0]);
      if (lane > jp) {
        x0 = x0 - s.e * ur.x;
        x1 = x1 - s.e * ur.y;
      }
      if (lane == jp) {
        x1 = s.what;
        q1 = s.q;
        e1 = s.e;
      }
    }
  }
  int8_t* cr = codes + row * K + c0;
  float* er = err + row * cols;
  if (v0) {
    wr[l0] = x0;
    cr[l0] = (int8_t)(int)q0;
    er[l0] = e0;
  }
  if (v1) {
    wr[l1] = x1;
    cr[l1] = (int8_t)(int)q1;
    er[l1] = e1;
  }
}

// w[n, k] -= sum_i err[n, i] u[c0 + i, k] for k >= k0 = c0 + cols: 64 x 64 output tiles, 256 threads with 4 x 4 values each, the
// errors and the rows of u staged through LDS sixteen i at a time; the sum runs over i ascending, unfused.
constexpr int PT = 64, PI = 16;

__global__ __launch_bounds__(256) void gptq_propagate_kernel(float* w, int64_t w_stride, const float* u, int64_t u_stride,
                                                             const float* err, int64_t N, int K, int c0, int cols) {
  __shared__ float es[PI][PT];  // es[i][n]
  __shared__ float ut[PI][PT];  // ut[i][k]
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t n0 = (int64_t)blockIdx.y * PT;
  const int k0 = c0 + cols + blockIdx.x * PT;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int i0 = 0; i0 < cols; i0 += PI) {
    for (int idx = threadIdx.x; idx < PI * PT; idx += 256) {
      const int n = idx / PI, i = idx % PI;  // err: consecutive threads along i
      es[i][n] = (n0 + n < N && i0 + i < cols) ? err[(n0 + n) * cols + i0 + i] : 0.f;
      const int iu = idx / PT, k = idx % PT;  // u: consecutive threads along k
      ut[iu][k] = (i0 + iu < cols && k0 + k < K) ? u[(int64_t)(c0 + i0 + iu) * u_stride + k0 + k] : 0.f;
    }
    __syncthreads();
    const int ni = (cols - i0 < PI) ? cols - i0 : PI;  // (exactly the block's terms: no padded + 0 term enters the sum)
    for (int i = 0; i < ni; ++i) {
      const float4 ev = *reinterpret_cast<const float4*>(&es[i][ty * 4]);
      const float4 uv = *reinterpret_cast<const float4*>(&ut[i][tx * 4]);
      const float e[4] = {ev.x, ev.y, ev.z, ev.w}, uu[4] = {uv.x, uv.y, uv.z, uv.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + e[a] * uu[b];
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int64_t n = n0 + ty * 4 + a;
    if (n >= N) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = k0 + tx * 4 + b;
      if (k < K) w[n * w_stride + k] = w[n * w_stride + k] - acc[a][b];
    }
  }
}

int check_gptq_common(const char* what, const void* w, int64_t w_stride, const void* u, int64_t u_stride, const void* err,
                      int64_t N, int K, int c0, int cols) {
  WANQ_REQUIRE(w && u && err, WANQ_E_ARG, "%s: w, u and err must be non-NULL", what);
  WANQ_REQUIRE(N >= 0 && N <= (int64_t)65535 * PT, WANQ_E_SHAPE, "%s: N=%lld out of range", what, (long long)N);
  WANQ_REQUIRE(K >= 1, WANQ_E_SHAPE, "%s: K=%d must be positive", what, K);
  WANQ_REQUIRE(cols >= 1 && cols <= GPTQ_COLS, WANQ_E_SHAPE, "%s: cols=%d must be 1..%d", what, cols, GPTQ_COLS);
  WANQ_REQUIRE(c0 >= 0 && (int64_t)c0 + cols <= K, WANQ_E_SHAPE, "%s: c0=%d + cols=%d must not exceed K=%d", what, c0, cols, K);
  WANQ_REQUIRE(w_stride >= K && u_stride >= K, WANQ_E_SHAPE, "%s: w_stride=%lld and u_stride=%lld must be at least K=%d", what,
               (long long)w_stride, (long long)u_stride, K);
  return WANQ_OK;
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gptq_block(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* delta, const float* zp,
                               int group_size, int qmin, int qmax, int8_t* codes, float* err, int64_t N, int K, int c0, int cols,
                               void* stream) {
  const char* what = "wanq_gptq_block";
  WANQ_REQUIRE(delta && zp && codes, WANQ_E_ARG, "%s: delta, zp and codes must be non-NULL", what);
  if (const int rc = check_gptq_common(what, w, w_stride, u, u_stride, err, N, K, c0, cols)) return rc;
  WANQ_REQUIRE(qmin >= -128 && qmax <= 127 && qmin <= qmax, WANQ_E_ARG, "%s: qmin=%d, qmax=%d must be an int8 range", what, qmin,
               qmax);
  WANQ_REQUIRE(group_size >= 0, WANQ_E_SHAPE, "%s: group_size=%d must be 0 (one per row) or positive", what, group_size);
  if (group_size) {
    WANQ_REQUIRE(K % group_size == 0, WANQ_E_SHAPE, "%s: group_size=%d must divide K=%d", what, group_size, K);
    WANQ_REQUIRE(group_size % 2 == 0 && c0 % 2 == 0, WANQ_E_SHAPE,
                 "%s: group_size=%d and c0=%d must be even (a lane's pair of columns lies in one group)", what, group_size, c0);
  }
  if (N == 0) return WANQ_OK;
  const int groups = group_size ? K / group_size : 1;
  gptq_block_kernel<false><<<dim3((unsigned)((N + GPTQ_WAVES - 1) / GPTQ_WAVES)), dim3(GPTQ_WAVES * 64), 0, (hipStream_t)stream>>>(
      w, w_stride, u, u_stride, delta, zp, nullptr, group_size, groups, (float)qmin, (float)qmax, codes, err, N, K, c0, cols);
  return check_launch(what);
}

extern "C" int wanq_gptq_block_gidx(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* delta, const float* zp,
                                    const int32_t* g_idx, int G, int qmin, int qmax, int8_t* codes, float* err, int64_t N, int K,
                                    int c0, int cols, void* stream) {
  const char* what = "wanq_gptq_block_gidx";
  WANQ_REQUIRE(delta && zp && codes && g_idx, WANQ_E_ARG, "%s: delta, zp, codes and g_idx must be non-NULL", what);
  if (const int rc = check_gptq_common(what, w, w_stride, u, u_stride, err, N, K, c0, cols)) return rc;
  WANQ_REQUIRE(qmin >= -128 && qmax <= 127 && qmin <= qmax, WANQ_E_ARG, "%s: qmin=%d, qmax=%d must be an int8 range", what, qmin,
               qmax);
  WANQ_REQUIRE(G >= 1, WANQ_E_SHAPE, "%s: G=%d must be at least 1 (the groups of a row of delta / zp)", what, G);
  if (N == 0) return WANQ_OK;
  gptq_block_kernel<true><<<dim3((unsigned)((N + GPTQ_WAVES - 1) / GPTQ_WAVES)), dim3(GPTQ_WAVES * 64), 0, (hipStream_t)stream>>>(
      w, w_stride, u, u_stride, delta, zp, g_idx, 0, G, (float)qmin, (float)qmax, codes, err, N, K, c0, cols);
  return check_launch(what);
}

extern "C" int wanq_gptq_propagate(float* w, int64_t w_stride, const float* u, int64_t u_stride, const float* err, int64_t N, int K,
                                   int c0, int cols, void* stream) {
  const char* what = "wanq_gptq_propagate";
  if (const int rc = check_gptq_common(what, w, w_stride, u, u_stride, err, N, K, c0, cols)) return rc;
  const int rest = K - c0 - cols;
  if (N == 0 || rest == 0) return WANQ_OK;
  gptq_propagate_kernel<<<dim3((unsigned)((rest + PT - 1) / PT), (unsigned)((N + PT - 1) / PT)), dim3(256), 0, (hipStream_t)stream>>>(
      w, w_stride, u, u_stride, err, N, K, c0, cols);
  return check_launch(what);
}
