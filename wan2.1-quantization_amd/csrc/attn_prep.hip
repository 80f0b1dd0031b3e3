// Attention front-end: RMSNorm over the full model dim (WanRMSNorm, wan/modules/model.py:73-89) fused with
// the 3-axis rotary embedding (rope_apply, model.py:43-70) for q and k.  Row-wise, HBM-bound: a row is
// read once, kept in registers across the sum-of-squares reduction, rotated, written once.
//
// rope table: fp32 [positions, head_dim/2, 2] = (cos, sin) per token position and complex pair; the host
// builds it once per (F,H,W) grid in float64 (as the reference does its whole rotation) and rounds to fp32.
// Rows at or beyond `positions` (sequence padding) are normalised but not rotated, as in the reference.
#include "row_frame.h"

namespace wanq {

struct PrepParams {
  const void* x;
  void* out;
  const float* weight;
  const float* rope;
  int x_dtype, out_dtype;
  int64_t rows, rows_per_batch, positions;
  int cols, head_dim;
  float eps;
  // optional int8 form for the int8 Q.K^T attention (wanq_attention_qk8_fwd): per-(token, head) symmetric 8-bit codes of the
  // normalised + rotated row (DynamicQuantizer semantics on [tokens*heads, head_dim] rows, Q/base/quant_attn.py:168-174 /
  // W/models/quant_opensora.py:431-436) and two fp32 planes [heads][scale_stride]: delta, and -12582912 * delta (the
  // constant the attention kernel's dequantising fma takes, see attention.hip)
  int8_t* q8;
  float* qscale;
  int64_t scale_stride;
  // optional scattered store (SC): head h of row r goes to out + head_map[2h] + r * head_map[2h+1] (elements) instead of the
  // row-major [rows, cols] image -- the kernel writes the Ulysses all-to-all send buffers ([P][rows][w] per head chunk) directly
  const int64_t* head_map;
  // optional centre (K smoothing): fp32 [cols] subtracted from y in front of the int8 quantiser only
  const float* center;
};

// The row arithmetic shared by every kernel of this file: row `row` into registers, RMSNorm over all C columns, rotary per head.
// v holds the fp32 y of the row afterwards (slots past the row end: zero, ok[i] false) -- the bits the plain kernel stores, the int8
// forms quantise and the column sums add.  id: the LDS slot set of the row's reduction (WPR = 4).  emit(i, c0) is called for
// every chunk slot i of the row (first column c0) as soon as v[i] is final: the kernels store / quantise / add from there.
template <int WPR, int NCH, typename EMIT>
__device__ __forceinline__ void prep_row(const PrepParams& p, const RowFrame<WPR, NCH>& f, float* slots, int id, int64_t row,
                                         float (&v)[NCH][8], bool (&ok)[NCH], EMIT&& emit) {
  const int C = p.cols;
  f.load(p.x, p.x_dtype, row * (int64_t)C, C, v, ok);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (ok[i]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  ss = RowReduce<WPR>{slots, f.wave}.template reduce<OpSum>(ss, id);
  const float rinv = p.weight ? 1.0f / sqrtf(ss / (float)C + p.eps) : 1.0f;  // weight == NULL: rope only
  const int64_t pos = row % p.rows_per_batch;
  const bool rot = p.rope && pos < p.positions;
  const int half = p.head_dim >> 1;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (!ok[i]) continue;
    const int c0 = f.col(i);
    if (p.weight) {
      float w[8];
      Io<F32>::load8(p.weight, c0, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = v[i][j] * rinv * w[j];
    }
    if (rot) {
      const int pair0 = (c0 % p.head_dim) >> 1;  // 4 consecutive complex pairs of one head
      float cs[8];
      Io<F32>::load8(p.rope, (pos * half + pair0) * 2, cs);
      // BOTH 16-byte pieces of the table row have landed before the first packed fp32 op.  hipcc otherwise waits for the first
      // piece only (s_waitcnt vmcnt(1)); with the attention-map kernels running beside this kernel (another stream or another
      // process on the GPU) a v_pk_mul_f32 reading the high register of a source pair through op_sel then returned 0 for lanes
      // 48-63 in ~0.4 % of launches while the second piece was still returning: one element per 16-byte chunk came out as a*cos
      // instead of a*cos - b*sin (profiles/r04_z_corun_corruption.txt; micro-victim tools/probes/late_beat.py; 0 of 30000 with
      // this wait).
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(cs[0]), "+v"(cs[1]), "+v"(cs[2]), "+v"(cs[3]), "+v"(cs[4]), "+v"(cs[5]), "+v"(cs[6]), "+v"(cs[7]));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // roundings fixed in the source (a product, then one fused multiply-add), so that every instantiation of this kernel and
        // every compiler mood gives the same bits: left to -ffp-contract the plain and the int8 form once disagreed
        const float a = v[i][2 * k], b = v[i][2 * k + 1];
        v[i][2 * k] = fmaf(a, cs[2 * k], -__fmul_rn(b, cs[2 * k + 1]));
        v[i][2 * k + 1] = fmaf(a, cs[2 * k + 1], __fmul_rn(b, cs[2 * k]));
      }
    }
    emit(i, c0);
  }
}

// Q8: also emit the per-(token, head) int8 form (a template flag so that the plain kernel keeps its register count)
// CEN (with Q8): the codes are those of y - center (K smoothing: one fp32 vector [cols] shared by all rows); `out` still gets y
template <int WPR, int NCH, bool Q8, bool SC = false, bool CEN = false>
__global__ __launch_bounds__(256) void rmsnorm_rope_kernel(const PrepParams p) {
  __shared__ float slots[4];
  RowFrame<WPR, NCH> f;
  if (f.surplus(p.rows)) return;
  const int lane = f.lane;
  const int64_t row = f.row;
  const int C = p.cols;
  const int64_t rbase = row * (int64_t)C;
  float v[NCH][8];
  bool ok[NCH];
  prep_row<WPR, NCH>(p, f, slots, 0, row, v, ok, [&](int i, int c0) {
    if (SC) {
      const int hd = c0 / p.head_dim;
      store8_rt(p.out, p.out_dtype, p.head_map[2 * hd] + row * p.head_map[2 * hd + 1] + (c0 - hd * p.head_dim), v[i]);
    } else if (p.out) {
      store8_rt(p.out, p.out_dtype, rbase + c0, v[i]);
    }
    if (Q8) {  // head_dim == 128: a head is the 16 chunks of 16 consecutive lanes
      if (CEN) {
        float c[8];
        Io<F32>::load8(p.center, c0, c);
        {
#pragma clang fp contract(off)  // one fp32 subtraction of the stored y: never folded into the multiply that made y
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][j] = v[i][j] - c[j];
        }
      }
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[i][j]));
      // lane ^ o inside the head's 16 lanes (DPP: wanq_common.h)
      m = fmaxf(m, lane_xor_dpp<1>(m)); m = fmaxf(m, lane_xor_dpp<2>(m)); m = fmaxf(m, lane_xor_dpp<4>(m)); m = fmaxf(m, lane_xor_dpp<8>(m));
      const float scale = dyn_scale(m, 127.0f, 1e-6f);
      uint32_t pk[2];
      quantN_pack_rne<8>(v[i], scale, 1.0f / scale, pk);
      *reinterpret_cast<uint2*>(p.q8 + rbase + c0) = make_uint2(pk[0], pk[1]);
      if ((lane & 15) == 0) {
        const int64_t so = (int64_t)(c0 >> 7) * p.scale_stride + row;
        p.qscale[so] = scale;
        p.qscale[(int64_t)(C >> 7) * p.scale_stride + so] = -12582912.0f * scale;
      }
    }
  });
}

// ---------------------------------------------------------------- column sums of y over all rows (K smoothing's centre)
// Deterministic, a function of (rows, cols) only: rows are cut into slabs of colsum_slab_rows(rows) rows; one row group (a wave for
// cols <= 2048, else the workgroup's four waves) walks its slab in ascending row order, one fp32 accumulator per column, and writes
// the slab's partial [cols] to the workspace; colsum_finish_kernel adds the partials in ascending slab order.  No atomics.
// Two rows are in flight per step (their loads overlap); they are still added one after the other, the lower row first.
template <int WPR, int NCH>
__global__ __launch_bounds__(256) void colsum_rmsnorm_rope_kernel(const PrepParams p, float* partial, int64_t slab_rows) {
  __shared__ float slots[8];
  RowFrame<WPR, NCH> f;  // f.row: the slab this row group sums
  const int64_t r0 = f.row * slab_rows;
  if (WPR == 1 && r0 >= p.rows) return;  // surplus wave of the last workgroup
  const int64_t r1 = r0 + slab_rows < p.rows ? r0 + slab_rows : p.rows;
  float acc[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  }
  bool ok[NCH], ok2[NCH];
  for (int64_t r = r0; r < r1; r += 2) {
    const bool two = r + 1 < r1;  // (uniform over the workgroup: every wave of a row takes the same barriers)
    float a[NCH][8], b[NCH][8];
    prep_row<WPR, NCH>(p, f, slots, 0, r, a, ok, [](int, int) {});
    prep_row<WPR, NCH>(p, f, slots, 1, two ? r + 1 : r, b, ok2, [](int, int) {});
    {
#pragma clang fp contract(off)  // plain additions of the y the other kernels store and quantise
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc[i][j] = acc[i][j] + a[i][j];
          if (two) acc[i][j] = acc[i][j] + b[i][j];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (f.col(i) < p.cols) Io<F32>::store8(partial, f.row * (int64_t)p.cols + f.col(i), acc[i]);
}

__global__ __launch_bounds__(64) void colsum_finish_kernel(const float* partial, float* colsum, int64_t slabs, int cols) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
#pragma unroll 16
  for (int64_t i = 0; i < slabs; ++i) s += partial[i * cols + c];
  colsum[c] = s;
}

}  // namespace wanq

using namespace wanq;

static int rmsnorm_rope_impl(const void* x, int x_dtype, const float* weight, const float* rope, void* out, int out_dtype,
                             int8_t* q8, float* qscale, int64_t scale_stride, int64_t rows, int cols, int head_dim,
                             int64_t rows_per_batch, int64_t positions, float eps, void* stream, const int64_t* head_map = nullptr,
                             const float* center = nullptr) {
  WANQ_REQUIRE(x && (out || q8), WANQ_E_ARG, "wanq_rmsnorm_rope: NULL pointer");
  WANQ_REQUIRE(!q8 || (qscale && head_dim == 128 && cols % 128 == 0 && scale_stride >= rows), WANQ_E_ARG,
               "wanq_rmsnorm_rope_q8: needs qscale, head_dim == 128, cols %% 128 == 0 and scale_stride >= rows");
  WANQ_REQUIRE(is_fp(x_dtype) && (!out || is_fp(out_dtype)), WANQ_E_ARG, "wanq_rmsnorm_rope: bad dtype code");
  WANQ_REQUIRE(weight || rope, WANQ_E_ARG, "wanq_rmsnorm_rope: nothing to do (weight and rope both NULL)");
  if (int e = check_rows_cols("wanq_rmsnorm_rope", rows, cols)) return e;
  WANQ_REQUIRE(!rope || (head_dim >= 8 && head_dim % 8 == 0 && cols % head_dim == 0), WANQ_E_SHAPE,
               "wanq_rmsnorm_rope: head_dim=%d must be a multiple of 8 dividing cols=%d", head_dim, cols);
  WANQ_REQUIRE(rows_per_batch >= 1, WANQ_E_SHAPE, "wanq_rmsnorm_rope: bad rows");
  if (rows == 0) return WANQ_OK;
  PrepParams p{x, out, weight, rope, x_dtype, out_dtype, rows, rows_per_batch, positions, cols, head_dim > 0 ? head_dim : 8, eps,
               q8, qscale, scale_stride, head_map, center};
  hipStream_t st = (hipStream_t)stream;
  row_ladder(cols, rows, [&](auto wpr, auto nch, dim3 grid) {
    constexpr int WPR = decltype(wpr)::value, NCH = decltype(nch)::value;
    if (q8 && center) hipLaunchKernelGGL((rmsnorm_rope_kernel<WPR, NCH, true, false, true>), grid, dim3(256), 0, st, p);
    else if (q8) hipLaunchKernelGGL((rmsnorm_rope_kernel<WPR, NCH, true>), grid, dim3(256), 0, st, p);
    else if (head_map) hipLaunchKernelGGL((rmsnorm_rope_kernel<WPR, NCH, false, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((rmsnorm_rope_kernel<WPR, NCH, false>), grid, dim3(256), 0, st, p);
  });
  return check_launch("wanq_rmsnorm_rope");
}

extern "C" int wanq_rmsnorm_rope(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                                 int out_dtype, int64_t rows, int cols, int head_dim, int64_t rows_per_batch,
                                 int64_t positions, float eps, void* stream) {
  WANQ_REQUIRE(out, WANQ_E_ARG, "wanq_rmsnorm_rope: NULL pointer");
  return rmsnorm_rope_impl(x, x_dtype, weight, rope, out, out_dtype, nullptr, nullptr, 0, rows, cols, head_dim, rows_per_batch,
                           positions, eps, stream);
}

extern "C" int wanq_rmsnorm_rope_q8(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                                    int out_dtype, int8_t* q8, float* qscale, int64_t scale_stride, int64_t rows, int cols,
                                    int head_dim, int64_t rows_per_batch, int64_t positions, float eps, void* stream) {
  WANQ_REQUIRE(q8, WANQ_E_ARG, "wanq_rmsnorm_rope_q8: q8 is required");
  return rmsnorm_rope_impl(x, x_dtype, weight, rope, out, out_dtype, q8, qscale, scale_stride, rows, cols, head_dim,
                           rows_per_batch, positions, eps, stream);
}

// wanq_rmsnorm_rope_q8 on y - center (K smoothing): `out`, when given, still receives the uncentred y
extern "C" int wanq_rmsnorm_rope_q8_centered(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                                             int out_dtype, int8_t* q8, float* qscale, int64_t scale_stride, const float* center,
                                             int64_t rows, int cols, int head_dim, int64_t rows_per_batch, int64_t positions,
                                             float eps, void* stream) {
  WANQ_REQUIRE(q8, WANQ_E_ARG, "wanq_rmsnorm_rope_q8_centered: q8 is required");
  WANQ_REQUIRE(center, WANQ_E_ARG, "wanq_rmsnorm_rope_q8_centered: center is NULL (fp32 [cols]; wanq_rmsnorm_rope_q8 is the uncentred form)");
  return rmsnorm_rope_impl(x, x_dtype, weight, rope, out, out_dtype, q8, qscale, scale_stride, rows, cols, head_dim,
                           rows_per_batch, positions, eps, stream, nullptr, center);
}

// Rows per slab of the column sums: 64, doubled until at most 1024 slabs remain -- a function of `rows` alone (never of the
// device), so that the order of the additions, and with it every bit of the result, is fixed by the shape.
static int64_t colsum_slab_rows(int64_t rows) {
  int64_t s = 64;
  while ((rows + s - 1) / s > 1024) s *= 2;
  return s;
}

extern "C" int64_t wanq_rmsnorm_rope_colsum_workspace(int64_t rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  const int64_t s = colsum_slab_rows(rows);
  return (rows + s - 1) / s * (int64_t)cols * (int64_t)sizeof(float);
}

extern "C" int wanq_rmsnorm_rope_colsum(const void* x, int x_dtype, const float* weight, const float* rope, int64_t rows, int cols,
                                        int head_dim, int64_t rows_per_batch, int64_t positions, float eps, float* colsum,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  WANQ_REQUIRE(x, WANQ_E_ARG, "wanq_rmsnorm_rope_colsum: NULL pointer");
  WANQ_REQUIRE(colsum, WANQ_E_ARG, "wanq_rmsnorm_rope_colsum: colsum is NULL (fp32 [cols])");
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "wanq_rmsnorm_rope_colsum: bad dtype code");
  if (int e = check_rows_cols("wanq_rmsnorm_rope_colsum", rows, cols)) return e;
  WANQ_REQUIRE(!rope || (head_dim >= 8 && head_dim % 8 == 0 && cols % head_dim == 0), WANQ_E_SHAPE,
               "wanq_rmsnorm_rope_colsum: head_dim=%d must be a multiple of 8 dividing cols=%d", head_dim, cols);
  WANQ_REQUIRE(rows_per_batch >= 1, WANQ_E_SHAPE, "wanq_rmsnorm_rope_colsum: bad rows");
  const int64_t need = wanq_rmsnorm_rope_colsum_workspace(rows, cols);
  WANQ_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), WANQ_E_ARG,
               "wanq_rmsnorm_rope_colsum: workspace of %lld bytes, %lld needed (wanq_rmsnorm_rope_colsum_workspace)",
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int64_t slab_rows = colsum_slab_rows(rows), slabs = (rows + slab_rows - 1) / slab_rows;  // rows == 0: no slab, zeros
  float* partial = static_cast<float*>(workspace);
  if (slabs > 0) {
    PrepParams p{x, nullptr, weight, rope, x_dtype, WANQ_F32, rows, rows_per_batch, positions, cols, head_dim > 0 ? head_dim : 8, eps,
                 nullptr, nullptr, 0, nullptr, nullptr};
    row_ladder(cols, slabs, [&](auto wpr, auto nch, dim3 grid) {
      constexpr int WPR = decltype(wpr)::value, NCH = decltype(nch)::value;
      hipLaunchKernelGGL((colsum_rmsnorm_rope_kernel<WPR, NCH>), grid, dim3(256), 0, st, p, partial, slab_rows);
    });
  }
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((cols + 63) / 64)), dim3(64), 0, st, partial, colsum, slabs, cols);
  return check_launch("wanq_rmsnorm_rope_colsum");
}

// RMSNorm + RoPE with the store scattered per head: head h (head_dim columns) of row r lands at
// out + head_map[2h] + r * head_map[2h+1] (elements of out_dtype; head_map is a DEVICE array of 2 * cols/head_dim int64).
// Writes the Ulysses head-scatter send buffers in place of the torch transpose().contiguous() pack (the reference's
// all_to_all_4D, ViDiT-Q/examples/Wan2.1/wan/distributed/xdit_context_parallel.py:147-192 via yunchang, does the same permute
// + contiguous on the host side of the collective).
extern "C" int wanq_rmsnorm_rope_scatter(const void* x, int x_dtype, const float* weight, const float* rope, void* out,
                                         int out_dtype, const int64_t* head_map, int64_t rows, int cols, int head_dim,
                                         int64_t rows_per_batch, int64_t positions, float eps, void* stream) {
  WANQ_REQUIRE(out && head_map, WANQ_E_ARG, "wanq_rmsnorm_rope_scatter: NULL pointer");
  WANQ_REQUIRE(head_dim >= 8 && head_dim % 8 == 0 && cols % head_dim == 0, WANQ_E_SHAPE,
               "wanq_rmsnorm_rope_scatter: head_dim=%d must be a multiple of 8 dividing cols=%d", head_dim, cols);
  return rmsnorm_rope_impl(x, x_dtype, weight, rope, out, out_dtype, nullptr, nullptr, 0, rows, cols, head_dim, rows_per_batch,
                           positions, eps, stream, head_map);
}
