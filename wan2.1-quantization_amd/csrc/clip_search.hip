// The clip search of the integer weight quantisers (AWQ's auto-clip, Lin et al., 2023; StaticQuantizer.search_clip drives it): PTQ-time
// kernels, once per layer.  The quantiser's grid is StaticQuantizer's with the row's extremes scaled by a ratio r_s = 1 - s / steps,
// s = 0 .. S-1 (s = 0 is the un-clipped grid); per quantiser row the s with the smallest objective is kept, a tie to the lower s.
//
// One definition of a candidate, shared by both kernels (clip_grid, clip_err), every operation one fp32 IEEE operation, never
// contracted (true divisions), so that delta / zp are bit-equal to the torch expression base_quantizer.clip_params:
//   r = 1 - s / steps
//   symmetric:   delta = (absmax r) / (2^(b-1) - 1), zp = 0
//   asymmetric:  hi' = max(hi, 0) r, lo' = min(lo, 0) r, delta = (hi' - lo') / (2^b - 1), zp = rne(lo' / delta) + 2^b / 2
//   code q = clamp(rne(w / delta) - zp, qmin, qmax) -- wanq_weight_quant's expression, the stored range -- and the error
//   e = fma(-(q + zp), delta, w): q + zp is a small integer, so e is the exact error rounded once.
//
// wanq_clip_search, objective sum_j h_j e_j^2 (h = 1: `mse`; h = diag H: `diag`): the row frame of row_frame.h.  A row is read once
// into registers (one wave for up to 2048 columns, four waves up to 16384), its extremes come from the DPP reductions, and all S
// candidates are evaluated from the registers: e^2 rounded, then acc = fma(e^2, h, acc) down the lane's elements in column order,
// the wave butterfly (32, 16, 8, 4, 2, 1), and for four waves the ordered sum of the four.  Nothing is stored but the outputs.
//
// wanq_clip_search_blocks, objective e H_gg e^T on the g x g diagonal block of the Hessian (`hessian`; g = 32, 64, 128), on
// v_mfma_f32_32x32x2_f32.  One workgroup (4 waves) per (group gi, tile of 128 weight rows); a wave owns 32 weight rows.
//   * H_gg is the same for every weight row: it is staged once into LDS, row-major hs[k][c] with a row stride of g + 8 words.
//   * The matrix cores form T^T = H_gg^T E^T in g / 32 accumulator tiles: tile ct is D[c][i], c = 32 ct .. 32 ct + 31 the block's
//     columns, i the wave's 32 weight rows.  In the accumulator layout lane l holds weight row i = l % 32 and, with h = l / 32, the
//     columns c = 32 ct + 8 (v / 4) + 4 h + v % 4, v = 0 .. 15: the columns whose bit 2 equals h.
//   * The contraction index k may be dealt to the MFMA's g / 2 steps in any order as long as both operands agree.  Step 4 m + t
//     (m < g / 8, t < 4) takes k = 8 m + 4 h + t from half h: the B operand, e_i[k], is then the lane's own weight row and exactly
//     the columns it holds in the accumulator layout.  So ONE register copy of the row's weights (g / 2 per lane) and ONE of the
//     candidate's errors serve as MFMA operand and as the second factor of sum_c T[i][c] e_i[c]; no value changes lanes.
//   * The A operand of step 4 m + t, tile ct, is hs[8 m + 4 h + t][32 ct + l % 32], one ds_read_b32: lanes 0-31 read 32
//     consecutive words, lanes 32-63 the same run four rows on.  With a stride of g + 8 words four rows are 4 g + 32 = 32 (mod 64)
//     words on (g is a multiple of 32), so the two runs fall into the two halves of the 64 banks: conflict-free whether the LDS
//     serves 64 lanes or 32 lanes a cycle.  (g + 8) * 4 bytes keeps the rows 16-byte aligned for the float4 fill.  g = 128: 68 KiB.
//     The fragments do not depend on the candidate: at g = 128 hipcc keeps them in AGPRs across the candidate loop (256 + 215
//     registers, no scratch), which leaves one workgroup per CU; a two-waves-per-SIMD launch bound spills 209 registers instead.
//   * The row's value: v = fma(T, e, v) down the lane's g / 2 columns in register order, then the two halves of the row (lane,
//     lane ^ 32) added.  Weight rows past N are masked: they read nothing, compute on zeros and store nothing.
// All outputs are written with plain vector stores by the lanes that own the row.
#include "row_frame.h"

// (the grid must be bit-equal to the torch expression: no a * b + c of this file becomes an fma unless written as one)
#pragma clang fp contract(off)

namespace wanq {
namespace {

constexpr int CLIP_STEPS_MAX = 64;

struct ClipRule {
  int sym;             // symmetric: zp = 0
  float levels, half;  // sym: 2^(b-1) - 1, unused; asym: 2^b - 1, 2^b / 2
  float qmin, qmax;    // the stored range
  int steps, n_cand;   // r_s = 1 - s / steps, s < n_cand
};

struct ClipGrid {
  float d, z;
};

__device__ __forceinline__ ClipGrid clip_grid(const ClipRule& p, float lo, float hi, int s) {
  const float r = 1.0f - (float)s / (float)p.steps;
  ClipGrid g;
  if (p.sym) {
    g.d = (fmaxf(fabsf(lo), fabsf(hi)) * r) / p.levels;
    g.z = 0.f;
  } else {
    const float h = fmaxf(hi, 0.f) * r, l = fminf(lo, 0.f) * r;
    g.d = (h - l) / p.levels;
    g.z = rintf(l / g.d) + p.half;
  }
  return g;
}

__device__ __forceinline__ float clip_err(const ClipRule& p, const ClipGrid& g, float w) {
  const float q = fminf(fmaxf(rintf(w / g.d) - g.z, p.qmin), p.qmax);
  return fmaf(-(q + g.z), g.d, w);
}

// the running minimum over the candidates: strict <, so a tie (and a NaN objective) keeps the lower s
struct ClipBest {
  float obj, d, z;
  int s;
  __device__ __forceinline__ void take(int cand, float o, const ClipGrid& g) {
    if (cand == 0 || o < obj) {
      obj = o;
      d = g.d;
      z = g.z;
      s = cand;
    }
  }
};

// ------------------------------------------------------------------------------ the elementwise form
template <int WPR, int NCH>
__global__ __launch_bounds__(256) void clip_search_rows_kernel(const float* w, const float* chan_w, int64_t chan_rows, ClipRule p,
                                                               float* delta, float* zp, int32_t* sel, float* table, int64_t rows,
                                                               int cols) {
  __shared__ float slots[(2 + CLIP_STEPS_MAX) * WPR];
  RowFrame<WPR, NCH> f;
  if (f.surplus(rows)) return;
  const RowReduce<WPR> red{slots, f.wave};
  float v[NCH][8], h[NCH][8];
  bool ok[NCH];
  f.template load_t<F32>(w, f.row * cols, cols, v, ok);
  if (chan_w) {  // row r of w.view(-1, g) holds the channels (r % chan_rows) * cols ..
    bool okh[NCH];
    f.template load_t<F32>(chan_w, (f.row % chan_rows) * cols, cols, h, okh);
  }
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (ok[i]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        lo = fminf(lo, v[i][j]);
        hi = fmaxf(hi, v[i][j]);
      }
    }
  lo = red.template reduce<OpMin>(lo, 0);
  hi = red.template reduce<OpMax>(hi, 1);
  ClipBest best;
  for (int s = 0; s < p.n_cand; ++s) {
    const ClipGrid g = clip_grid(p, lo, hi, s);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (ok[i]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float e = clip_err(p, g, v[i][j]);
          const float e2 = e * e;
          acc = chan_w ? fmaf(e2, h[i][j], acc) : acc + e2;
        }
      }
    acc = red.template reduce<OpSum>(acc, 2 + s);
    if (table && f.lane == 0 && f.sub == 0) table[f.row * p.n_cand + s] = acc;
    best.take(s, acc, g);
  }
  if (f.lane == 0 && f.sub == 0) {
    delta[f.row] = best.d;
    zp[f.row] = best.z;
    sel[f.row] = best.s;
  }
}

// ------------------------------------------------------------------------------ the block form
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int BLK_ROWS = 128;  // weight rows of a workgroup: 4 waves x 32

template <int G>
__global__ __launch_bounds__(256) void clip_search_blocks_kernel(const float* w, const float* hblocks, ClipRule p, float* delta,
                                                                 float* zp, int32_t* sel, float* table, int64_t N, int K) {
  constexpr int LDH = G + 8;  // words: 4 rows on = 32 (mod 64) banks (file header)
  constexpr int NT = G / 32;  // accumulator tiles
  constexpr int NV = G / 2;   // a row's values in one lane
  __shared__ float hs[G * LDH];
  const int gi = blockIdx.y, groups = K / G;
  const float* hg = hblocks + (int64_t)gi * G * G;
  for (int idx = threadIdx.x * 4; idx < G * G; idx += 256 * 4)
    *reinterpret_cast<float4*>(&hs[(idx / G) * LDH + idx % G]) = *reinterpret_cast<const float4*>(hg + idx);
  __syncthreads();  // (the workgroup's only barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, half = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * BLK_ROWS + wave * 32 + i;
  const bool live = row < N;
  // value x = 4 m + t of the lane is column 8 m + 4 half + t of the block
  float wv[NV];
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int m = 0; m < G / 8; ++m) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) q = *reinterpret_cast<const float4*>(w + row * K + (int64_t)gi * G + 8 * m + 4 * half);
    wv[4 * m] = q.x, wv[4 * m + 1] = q.y, wv[4 * m + 2] = q.z, wv[4 * m + 3] = q.w;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      lo = fminf(lo, wv[4 * m + t]);
      hi = fmaxf(hi, wv[4 * m + t]);
    }
  }
  {  // the row's other half lies in lane ^ 32
    const uint2 a = pair32(__float_as_int(lo)), b = pair32(__float_as_int(hi));
    lo = fminf(__uint_as_float(a.x), __uint_as_float(a.y));
    hi = fmaxf(__uint_as_float(b.x), __uint_as_float(b.y));
  }
  const int64_t out = row * groups + gi;  // the row of w.view(-1, g)
  ClipBest best;
  for (int s = 0; s < p.n_cand; ++s) {
    ClipGrid g = clip_grid(p, lo, hi, s);
    ClipGrid ge = g;
    if (!live) ge.d = 1.f, ge.z = 0.f;  // a masked row computes on zeros: e = 0, no 0 / 0 enters the matrix cores
    float e[NV];
#pragma unroll
    for (int x = 0; x < NV; ++x) e[x] = clip_err(p, ge, wv[x]);
    f32x16 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int x = 0; x < NV; ++x) {
      const float* hrow = &hs[(8 * (x / 4) + 4 * half + x % 4) * LDH + i];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(hrow[32 * ct], e[x], acc[ct], 0, 0, 0);
    }
    // accumulator r of tile ct is column 32 ct + 8 (r / 4) + 4 half + r % 4: the lane's value 16 ct + r
    float val = 0.f;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) val = fmaf(acc[ct][r], e[16 * ct + r], val);
    const uint2 both = pair32(__float_as_int(val));
    val = __uint_as_float(both.x) + __uint_as_float(both.y);
    if (table && live && half == 0) table[out * p.n_cand + s] = val;
    best.take(s, val, g);
  }
  if (live && half == 0) {
    delta[out] = best.d;
    zp[out] = best.z;
    sel[out] = best.s;
  }
}

int check_clip_common(const char* what, const void* w, const void* delta, const void* zp, const void* sel, int n_bits, int sym,
                      int qmin, int qmax, int steps, int n_cand, ClipRule* p) {
  WANQ_REQUIRE(w && delta && zp && sel, WANQ_E_ARG, "%s: w, delta, zp and sel must be non-NULL", what);
  WANQ_REQUIRE((uintptr_t)w % 16 == 0, WANQ_E_ARG, "%s: w must be 16-byte aligned", what);
  WANQ_REQUIRE(n_bits >= 2 && n_bits <= 8, WANQ_E_ARG, "%s: n_bits=%d must be 2..8", what, n_bits);
  WANQ_REQUIRE(qmin >= -128 && qmax <= 127 && qmin <= qmax, WANQ_E_ARG, "%s: qmin=%d, qmax=%d must be an int8 range", what, qmin,
               qmax);
  WANQ_REQUIRE(steps >= 1 && steps <= CLIP_STEPS_MAX, WANQ_E_ARG, "%s: steps=%d must be 1..%d", what, steps, CLIP_STEPS_MAX);
  WANQ_REQUIRE(n_cand >= 1 && n_cand <= steps, WANQ_E_ARG, "%s: n_cand=%d must be 1..steps=%d (the ratio 1 - s / steps stays positive)",
               what, n_cand, steps);
  p->sym = sym != 0;
  p->levels = (float)(sym ? (1 << (n_bits - 1)) - 1 : (1 << n_bits) - 1);
  p->half = (float)((1 << n_bits) / 2);
  p->qmin = (float)qmin, p->qmax = (float)qmax;
  p->steps = steps, p->n_cand = n_cand;
  return WANQ_OK;
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_clip_search(const float* w, const float* chan_w, int chan_len, int n_bits, int sym, int qmin, int qmax, int steps,
                                int n_cand, float* delta, float* zp, int32_t* sel, float* table, int64_t rows, int cols, void* stream) {
  const char* what = "wanq_clip_search";
  ClipRule p;
  if (const int rc = check_clip_common(what, w, delta, zp, sel, n_bits, sym, qmin, qmax, steps, n_cand, &p)) return rc;
  if (const int rc = check_rows_cols(what, rows, cols)) return rc;
  if (chan_w) {
    WANQ_REQUIRE((uintptr_t)chan_w % 16 == 0, WANQ_E_ARG, "%s: chan_w must be 16-byte aligned", what);
    WANQ_REQUIRE(chan_len >= cols && chan_len % cols == 0, WANQ_E_SHAPE,
                 "%s: chan_len=%d must be a positive multiple of cols=%d (row r holds the channels (r %% (chan_len / cols)) cols ..)",
                 what, chan_len, cols);
  }
  if (rows == 0) return WANQ_OK;
  const int64_t chan_rows = chan_w ? chan_len / cols : 1;
  row_ladder(cols, rows, [&](auto wpr, auto nch, dim3 grid) {
    clip_search_rows_kernel<decltype(wpr)::value, decltype(nch)::value><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
        w, chan_w, chan_rows, p, delta, zp, sel, table, rows, cols);
  });
  return check_launch(what);
}

extern "C" int wanq_clip_search_blocks(const float* w, const float* hblocks, int g, int n_bits, int sym, int qmin, int qmax, int steps,
                                       int n_cand, float* delta, float* zp, int32_t* sel, float* table, int64_t N, int K,
                                       void* stream) {
  const char* what = "wanq_clip_search_blocks";
  ClipRule p;
  if (const int rc = check_clip_common(what, w, delta, zp, sel, n_bits, sym, qmin, qmax, steps, n_cand, &p)) return rc;
  WANQ_REQUIRE(hblocks && (uintptr_t)hblocks % 16 == 0, WANQ_E_ARG, "%s: hblocks must be non-NULL and 16-byte aligned", what);
  WANQ_REQUIRE(g == 32 || g == 64 || g == 128, WANQ_E_SHAPE, "%s: g=%d must be 32, 64 or 128 (the block is held in LDS)", what, g);
  WANQ_REQUIRE(K >= g && K % g == 0 && K / g <= 65535, WANQ_E_SHAPE, "%s: K=%d must be a multiple of g=%d, at most 65535 groups",
               what, K, g);
  WANQ_REQUIRE(N >= 0 && N < (1ll << 31), WANQ_E_SHAPE, "%s: N=%lld out of range", what, (long long)N);
  if (N == 0) return WANQ_OK;
  const dim3 grid((unsigned)((N + BLK_ROWS - 1) / BLK_ROWS), (unsigned)(K / g));
  hipStream_t st = (hipStream_t)stream;
  if (g == 32) clip_search_blocks_kernel<32><<<grid, dim3(256), 0, st>>>(w, hblocks, p, delta, zp, sel, table, N, K);
  else if (g == 64) clip_search_blocks_kernel<64><<<grid, dim3(256), 0, st>>>(w, hblocks, p, delta, zp, sel, table, N, K);
  else clip_search_blocks_kernel<128><<<grid, dim3(256), 0, st>>>(w, hblocks, p, delta, zp, sel, table, N, K);
  return check_launch(what);
}
