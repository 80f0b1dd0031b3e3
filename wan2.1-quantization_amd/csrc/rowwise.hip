// Row-wise HBM-bound kernels of the denoising step: per-token int8 quantisation, LayerNorm+modulate(+quant), gate-residual.
// Layout, row frame, reduction and dispatch ladder: row_frame.h.  (Calibration and once-per-model kernels: quant_tools.hip.)
#include "row_frame.h"

namespace wanq {

struct RowParams {
  const void* x;
  int x_dtype;
  // layernorm
  const void* gamma;
  const void* mshift;
  const void* mscale;
  int mod_dtype;
  int64_t mod_stride;
  int64_t rows_per_batch;
  float eps;
  // outputs
  void* out_fp;
  int out_dtype;
  int8_t* q;
  void* scale;
  void* sum;
  int vec_dtype;
  int64_t rows;
  int cols;
  int act;
  int static_amax;
  const float* premul;  // [cols] fp32 multiplier applied before quantisation (SmoothQuant channel mask), or NULL
  // dynamic quantiser range: scale = absmax / levels floored at `floor` (127 and 1e-6 for every 8-bit entry point;
  // wanq_quant_rows_levels: 2^(b-1) - 1 and the caller's floor, 0 = none: a zero row then gets scale 0 and codes 0)
  float levels, floor;
};

// v <- v * m (MUL) / v * (1 + m) (MUL1P) / v + m (ADD) with a per-column vector m; one dtype branch per row (row_frame.h)
enum { MOD_MUL = 0, MOD_MUL1P = 1, MOD_ADD = 2 };
template <typename T, int OP, int WPR, int NCH>
__device__ __forceinline__ void mod_row_t(const RowFrame<WPR, NCH>& f, const void* m, int64_t mbase, float (&v)[NCH][8], const bool (&ok)[NCH]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (ok[i]) {
      float t[8];
      Io<T>::load8(m, mbase + f.col(i), t);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = OP == MOD_MUL ? v[i][j] * t[j] : OP == MOD_MUL1P ? v[i][j] * (1.0f + t[j]) : v[i][j] + t[j];
    }
}
template <int OP, int WPR, int NCH>
__device__ __forceinline__ void mod_row(const RowFrame<WPR, NCH>& f, const void* m, int dt, int64_t mbase, float (&v)[NCH][8], const bool (&ok)[NCH]) {
  if (dt == WANQ_F32) mod_row_t<F32, OP>(f, m, mbase, v, ok);
  else if (dt == WANQ_BF16) mod_row_t<BF16, OP>(f, m, mbase, v, ok);
  else mod_row_t<F16, OP>(f, m, mbase, v, ok);
}

template <int WPR, int NCH, bool LN>
__global__ __launch_bounds__(256) void rowwise_kernel(const RowParams p) {
  __shared__ float red_slots[4 * 4];
  RowFrame<WPR, NCH> f;
  if (f.surplus(p.rows)) return;
  const RowReduce<WPR> red{red_slots, f.wave};
  const int64_t row = f.row;
  const int C = p.cols;
  const int64_t rbase = row * (int64_t)C;

  float v[NCH][8];
  bool ok[NCH];
  f.load(p.x, p.x_dtype, rbase, C, v, ok);

  if (LN) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[i][j];
    const float mean = red.template reduce<OpSum>(s, 0) / (float)C;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (ok[i]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[i][j] - mean;
          s2 += d * d;
        }
      }
    const float var = red.template reduce<OpSum>(s2, 1) / (float)C;
    const float rstd = 1.0f / sqrtf(var + p.eps);
    const int64_t mb = (row / p.rows_per_batch) * p.mod_stride;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (ok[i]) {  // chunks past the row end stay zero: they take part in the row max and sum
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = (v[i][j] - mean) * rstd;
      }
    if (p.gamma) mod_row<MOD_MUL>(f, p.gamma, p.mod_dtype, 0, v, ok);
    if (p.mscale) mod_row<MOD_MUL1P>(f, p.mscale, p.mod_dtype, mb, v, ok);
    if (p.mshift) mod_row<MOD_ADD>(f, p.mshift, p.mod_dtype, mb, v, ok);
  } else if (p.act == 1) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = gelu_tanh_fast_f32(v[i][j]);  // branch-free form (3e-6 rel): libm tanhf x 8 NCH bloats every variant
  }

  if (p.premul) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (ok[i]) {
        float pm[8];
        Io<F32>::load8(p.premul, f.col(i), pm);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] *= pm[j];
      }
  }
  if (p.out_fp) f.store(p.out_fp, p.out_dtype, rbase, v, ok);
  if (!p.q) return;

  float amax;
  if (p.static_amax) {
    amax = vec_load(p.scale, p.vec_dtype, row);
  } else {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[i][j]));
    amax = red.template reduce<OpMax>(m, 2);
  }
  const float scale = dyn_scale(amax, p.levels, p.floor);
  const float inv = scale > 0.f ? 1.0f / scale : 0.f;  // (no floor and an all-zero row: every code is 0)
  const bool writer = f.lane == 0 && f.sub == 0;
  int isum = 0;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    uint32_t lo, hi;
    if (p.static_amax) {  // a given scale: values may exceed the code range and are clamped
      int qi[8];
      quant8_div_rne(v[i], scale, inv, qi);
      lo = pack4_i8_fast(qi[0], qi[1], qi[2], qi[3]), hi = pack4_i8_fast(qi[4], qi[5], qi[6], qi[7]);
    } else {              // the row's own scale: |v / scale| <= 127.5 by construction
      uint32_t pk[2];
      quantN_pack_rne<8>(v[i], scale, inv, pk);
      lo = pk[0], hi = pk[1];
    }
    isum = byte_sum(hi, byte_sum(lo, isum));
    if (ok[i]) *reinterpret_cast<uint2*>(p.q + rbase + f.col(i)) = make_uint2(lo, hi);
  }
  if (p.sum) {
    const int tot = red.template reduce<OpSum>(isum, 3);
    if (writer) vec_store(p.sum, p.vec_dtype, row, (float)tot * scale);
  }
  if (!p.static_amax && writer) vec_store(p.scale, p.vec_dtype, row, scale);
}

template <bool LN>
static int launch_rowwise(const RowParams& p, hipStream_t st, const char* what) {
  row_ladder(p.cols, p.rows, [&](auto wpr, auto nch, dim3 grid) {
    hipLaunchKernelGGL((rowwise_kernel<decltype(wpr)::value, decltype(nch)::value, LN>), grid, dim3(256), 0, st, p);
  });
  return check_launch(what);
}

// ------------------------------------------------------------------------------ gate * y + residual
struct GateParams {
  const void* y;
  const void* gate;
  const void* res;
  void* out;
  int y_dtype, gate_dtype, res_dtype, out_dtype;
  int64_t gate_stride, rows_per_batch, rows;
  int cols;
};

__global__ __launch_bounds__(256) void gate_residual_kernel(const GateParams p) {
  const int cpr = p.cols / 8;  // chunks per row
  const int64_t total = p.rows * (int64_t)cpr;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < total; ch += (int64_t)gridDim.x * 256) {
    const int64_t row = ch / cpr;
    const int c0 = (int)(ch - row * cpr) * 8;
    float y[8], g[8], r[8];
    load8_rt(p.y, p.y_dtype, row * p.cols + c0, y);
    load8_rt(p.gate, p.gate_dtype, (row / p.rows_per_batch) * p.gate_stride + c0, g);
    load8_rt(p.res, p.res_dtype, row * p.cols + c0, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = y[j] * g[j] + r[j];
    store8_rt(p.out, p.out_dtype, row * p.cols + c0, y);
  }
}

// ------------------------------------------------------------------------------ wide 16-bit rows: one WAVE per row
// The FFN hidden of the 1.3B model ([L, 8960] bf16 -> int8, with or without the tanh-GELU: quant_sum / gelu_quant_sum) through
// the general kernel is four waves per row, two workgroup barriers per row (row maximum, integer sum), five chunk slots per
// lane of which the row fills 4.4, and a control-flow graph that carries every option of the general entry: 26 vector
// instructions per element (profiles/r03_h_rowwise_sq.csv) for a job that needs about ten.  Here a wave owns a row: NCH
// 16-byte chunks per lane (chunk lane + 64 i), all requested up front, the row kept in registers, both reductions inside
// the wave (DPP / permlane swaps: no LDS, no barrier), one dtype per instantiation, no other options.  Bit-identical
// outputs (same operations per element, same reduction tree per wave; the cross-wave LDS step of the general kernel is a
// max / an integer sum).
template <typename T, int NCH, bool GELU>
__global__ __launch_bounds__(256, 2) void quant_rows_wave_kernel(const void* x, int8_t* q, void* scale_out, void* sum_out, int vec_dtype,
                                                                 int64_t rows, int cols) {
  static_assert(NCH % 2 == 0, "chunks are owned in pairs");
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole wave (no barriers in this kernel)
  const int64_t rbase = row * (int64_t)cols;
  const int last = cols / 8 - 1;  // last valid chunk
  // a lane owns PAIRS of adjacent chunks (pair lane + 64 h = chunks 2 pair, 2 pair + 1): 32 contiguous input bytes and, for the
  // codes, ONE 16-byte store per pair (8-byte stores run at about half the rate per byte)
  float v[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int ch = 2 * (lane + 64 * (i >> 1)) + (i & 1);
    Io<T>::load8(x, rbase + (int64_t)(ch <= last ? ch : last) * 8, v[i]);  // (a lane past the row end re-reads the last chunk)
  }
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const bool ok = 2 * (lane + 64 * (i >> 1)) + (i & 1) <= last;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      float t0 = v[i][j], t1 = v[i][j + 1];
      if (GELU) {
        // gelu_tanh_fast_f32 on element PAIRS: the same operations, the plain ones as packed fp32 (bit-identical)
        typedef float v2f __attribute__((ext_vector_type(2)));
        const v2f x = {t0, t1}, c3 = {-0.10294324f, -0.10294324f}, c1 = {-2.3022082f, -2.3022082f}, one = {1.0f, 1.0f};
        const v2f u = x * __builtin_elementwise_fma(x * x, c3, c1);
        const v2f d = one + (v2f){__builtin_amdgcn_exp2f(u.x), __builtin_amdgcn_exp2f(u.y)};
        const v2f r = x * (v2f){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        t0 = r.x;
        t1 = r.y;
      }
      t0 = ok ? t0 : 0.f;
      t1 = ok ? t1 : 0.f;
      v[i][j] = t0;
      v[i][j + 1] = t1;
      m = fmaxf(m, fmaxf(fabsf(t0), fabsf(t1)));
    }
  }
  const float scale = dyn_scale(wave_max(m), 127.0f, 1e-6f);
  const float inv = 1.0f / scale;
  int isum = 0;
#pragma unroll
  for (int h = 0; h < NCH / 2; ++h) {
    uint32_t pa[2], pb[2];
    quantN_pack_rne<8>(v[2 * h], scale, inv, pa);
    quantN_pack_rne<8>(v[2 * h + 1], scale, inv, pb);
    isum = byte_sum(pb[1], byte_sum(pb[0], byte_sum(pa[1], byte_sum(pa[0], isum))));
    const int ch = 2 * (lane + 64 * h);
    int8_t* dst = q + rbase + (int64_t)ch * 8;
    if (ch + 1 <= last) *reinterpret_cast<uint4*>(dst) = make_uint4(pa[0], pa[1], pb[0], pb[1]);
    else if (ch <= last) *reinterpret_cast<uint2*>(dst) = make_uint2(pa[0], pa[1]);
  }
  if (sum_out) {
    const int tot = wave_sum(isum);
    if (lane == 0) vec_store(sum_out, vec_dtype, row, (float)tot * scale);
  }
  if (lane == 0) vec_store(scale_out, vec_dtype, row, scale);
}

// cols in (8704, 9216] (the 1.3B FFN width 8960 = 17.5 chunks per lane): NCH = 18
static bool launch_quant_rows_wave(const void* x, int x_dtype, int8_t* q, void* scale, void* sum, int vec_dtype, int64_t rows, int cols, int act,
                                   hipStream_t st) {
  if (cols <= 8704 || cols > 9216 || (x_dtype != WANQ_BF16 && x_dtype != WANQ_F16)) return false;
  const dim3 grid((unsigned)((rows + 3) / 4));
#define WANQ_QW(T, G) hipLaunchKernelGGL((quant_rows_wave_kernel<T, 18, G>), grid, dim3(256), 0, st, x, q, scale, sum, vec_dtype, rows, cols)
  if (x_dtype == WANQ_BF16) { if (act) WANQ_QW(BF16, true); else WANQ_QW(BF16, false); }
  else { if (act) WANQ_QW(F16, true); else WANQ_QW(F16, false); }
#undef WANQ_QW
  return true;
}

// ------------------------------------------------------------------------------ per-row dynamic OCP e4m3 (fp8) quantiser
// scale = max(absmax / 448, 1e-6), q = e4m3fn_rne(clamp(x / scale, -448, 448)): the row frame and ladder of the int8 quantiser, the
// true fp32 division, and one rounding, made by the packed hardware conversion (v_cvt_pk_fp8_f32: OCP e4m3fn on gfx950, round to
// nearest even, subnormal codes kept) behind the clamp, so the conversion never meets a value past the format's largest.  Codes
// leave as whole 8-byte chunks per lane.  Activations per token and, once at conversion time, weights per output channel.
struct Fp8RowParams {
  const void* x;
  int x_dtype;
  uint8_t* q;
  float* scale;
  int64_t rows;
  int cols;
  int act;
};

constexpr float FP8_E4M3_MAX = 448.0f;

template <int WPR, int NCH>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const Fp8RowParams p) {
  __shared__ float red_slots[4];
  RowFrame<WPR, NCH> f;
  if (f.surplus(p.rows)) return;
  const RowReduce<WPR> red{red_slots, f.wave};
  const int C = p.cols;
  const int64_t rbase = f.row * (int64_t)C;

  float v[NCH][8];
  bool ok[NCH];
  f.load(p.x, p.x_dtype, rbase, C, v, ok);
  if (p.act == 1) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = gelu_tanh_fast_f32(v[i][j]);  // (a slot past the row end stays 0)
  }
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[i][j]));
  const float scale = dyn_scale(red.template reduce<OpMax>(m, 0), FP8_E4M3_MAX, 1e-6f);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (!ok[i]) continue;
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = __builtin_amdgcn_fmed3f(v[i][j] / scale, -FP8_E4M3_MAX, FP8_E4M3_MAX);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], hi, true);
    *reinterpret_cast<uint2*>(p.q + rbase + f.col(i)) = make_uint2((uint32_t)lo, (uint32_t)hi);
  }
  if (f.lane == 0 && f.sub == 0) p.scale[f.row] = scale;
}

// ------------------------------------------------------------------------------ OCP MX block quantiser (e4m3 / e2m1 codes, E8M0 scales)
// One power-of-two scale per block of 32 consecutive columns: s = clamp(E(amax) - emax, 0, 254), c = rne(clamp(ldexp(x, 127 - s))).
// The row frame and ladder of the other quantisers.  A block is four consecutive 8-element chunks, and chunk slot i of a lane is
// chunk (a multiple of 64) + lane, so a block sits in the four lanes of one aligned quad at one slot: its maximum is two DPP quad
// exchanges per slot, never a reduction over the row (no LDS, no barrier, in the four-wave form too).  cols % 32 == 0, so a quad is
// inside the row or past it as a whole.  The scaling is one exact v_ldexp_f32; e4m3 is rounded by the packed hardware conversion
// behind the clamp as in the fp8 quantiser, e2m1 by seven comparisons against the midpoints (> where the tie goes down to the even
// code, >= where it goes up).  e4m3 codes leave as 8-byte chunks, e2m1 codes as one dword of eight nibbles (even k low), the scale
// byte from the quad's first lane.
// FP6 (wanq_quant_rows_mx6, e2m3): the scale of e2m1 (emax 2); the code is rne(|t| / q) + {0, 8, 16} with the binade's quantum q = 1/8,
// 1/4, 1/2 (one v_rndne_f32 of an exact product; the magnitude codes ascend with the value, so a carry into the next binade is the
// next code).  A lane's eight codes are 48 bits and the quad's 192 bits are the block's 24 bytes: lane k of the quad takes the low
// dword and high half-word of lane k + 1 by one DPP quad rotation each and lanes 0-2 store the aligned 8-byte words 0-2 of the block.
// HAD (wanq_quant_rows_mx_had32): behind the GELU and in front of the block maximum every block is replaced by its unnormalised 32-point
// Sylvester-Hadamard transform, five fp32 butterfly stages h = 1, 2, 4, 8, 16 with (x_i, x_{i+h}) <- (x_i + x_{i+h}, x_i - x_{i+h})
// for bit h of i clear.  Element i of a block is chunk element i & 7 of quad lane i >> 3: stages 1, 2, 4 stay inside the chunk, stages
// 8 and 16 are the quad exchanges the maximum uses, the lane with the bit set keeping partner - own.  Additions and subtractions
// only, one rounding each, in a fixed order: bit-equal to mx_hadamard32_host.  Still no LDS and no barrier.
struct MxRowParams {
  const void* x;
  int x_dtype;
  uint8_t* q;
  uint8_t* scale;
  int64_t rows;
  int cols;
  int act;
};

__device__ __forceinline__ uint32_t e2m1_code(float t) {
  const float a = fminf(fabsf(t), 6.0f);
  const uint32_t mag = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return mag | ((__float_as_uint(t) >> 28) & 8u);
}

__device__ __forceinline__ uint32_t e2m3_code(float t) {
  const float a = fminf(fabsf(t), 7.5f);
  const float r = a < 2.0f ? rintf(a * 8.0f) : a < 4.0f ? rintf(a * 4.0f) + 8.0f : rintf(a * 2.0f) + 16.0f;
  return (uint32_t)r | ((__float_as_uint(t) >> 26) & 32u);
}

// the value of the quad's next lane (lane 3: lane 0's, unused)
__device__ __forceinline__ uint32_t quad_next_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x39, 0xf, 0xf, true);  // quad_perm:[1,2,3,0]
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

// one butterfly stage across the quad: MASK = 1 (h = 8) or 2 (h = 16)
template <int MASK>
__device__ __forceinline__ void had_stage_quad(float (&v)[8], bool upper) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float o = lane_xor_dpp<MASK>(v[j]);
    v[j] = upper ? o - v[j] : v[j] + o;
  }
}

template <int WPR, int NCH, bool FP4, bool HAD = false, bool FP6 = false>
__global__ __launch_bounds__(256) void quant_rows_mx_kernel(const MxRowParams p) {
  static_assert(!(FP6 && (FP4 || HAD)), "e2m3 is a format of its own, without the rotation");
  RowFrame<WPR, NCH> f;
  if (f.surplus(p.rows)) return;
  const int C = p.cols;
  const int64_t rbase = f.row * (int64_t)C;
  constexpr int EMAX = FP4 || FP6 ? 2 : 8;

  float v[NCH][8];
  bool ok[NCH];
  f.load(p.x, p.x_dtype, rbase, C, v, ok);
  if (p.act == 1) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = gelu_tanh_fast_f32(v[i][j]);  // (a slot past the row end stays 0)
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if constexpr (HAD) {
      had_stage<1>(v[i]);
      had_stage<2>(v[i]);
      had_stage<4>(v[i]);
      had_stage_quad<1>(v[i], f.lane & 1);
      had_stage_quad<2>(v[i], f.lane & 2);
    }
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[i][j]));
    m = fmaxf(m, lane_xor_dpp<1>(m));
    m = fmaxf(m, lane_xor_dpp<2>(m));
    if (!ok[i]) continue;
    int s = (int)((__float_as_uint(m) >> 23) & 0xffu) - EMAX;
    s = s < 0 ? 0 : (s > 254 ? 254 : s);
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = ldexpf(v[i][j], 127 - s);
    const int col = f.col(i);
    if constexpr (FP6) {
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) c |= (uint64_t)e2m3_code(t[j]) << (6 * j);
      const uint32_t lo = (uint32_t)c, hi = (uint32_t)(c >> 32);  // 48 bits: bits 48 k .. 48 k + 47 of the block, k the quad lane
      const uint32_t nlo = quad_next_dpp(lo), nhi = quad_next_dpp(hi);
      const int k = (col >> 3) & 3;
      const uint2 w = k == 0 ? make_uint2(lo, hi | (nlo << 16))
                    : k == 1 ? make_uint2((lo >> 16) | (hi << 16), nlo)
                             : make_uint2(hi | (nlo << 16), (nlo >> 16) | (nhi << 16));
      if (k < 3) *reinterpret_cast<uint2*>(p.q + ((rbase + col) >> 5) * 24 + 8 * k) = w;
    } else if constexpr (FP4) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) w |= e2m1_code(t[j]) << (4 * j);
      *reinterpret_cast<uint32_t*>(p.q + ((rbase + col) >> 1)) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = __builtin_amdgcn_fmed3f(t[j], -FP8_E4M3_MAX, FP8_E4M3_MAX);
      int lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], lo, true);
      int hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], 0, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], hi, true);
      *reinterpret_cast<uint2*>(p.q + rbase + col) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
    if ((f.lane & 3) == 0) p.scale[((rbase + col) >> 5)] = (uint8_t)s;
  }
}

// x * premul (-> LayerNorm + modulate first when `ln`) -> fp output and / or int8 quantise: the transform entry points of
// rotate.hip with had_k == 0 (channel scale without rotation: SmoothQuant, Q/smooth_quant/sq_quant_layer.py:52-60).
int premul_quant_rows(bool ln, const void* x, int x_dtype, const void* gamma, const void* mshift, const void* mscale,
                      int64_t mod_stride, int64_t rows_per_batch, float eps, const float* premul, void* out_fp, int out_dtype,
                      int8_t* q, void* scale, void* sum, int vec_dtype, int64_t rows, int cols, hipStream_t st, const char* what) {
  if (int e = check_rows_cols(what, rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  RowParams p{};
  p.levels = 127.0f; p.floor = 1e-6f;
  p.x = x; p.x_dtype = x_dtype; p.gamma = gamma; p.mshift = mshift; p.mscale = mscale; p.mod_dtype = WANQ_F32;
  p.mod_stride = mod_stride; p.rows_per_batch = rows_per_batch; p.eps = eps; p.out_fp = out_fp; p.out_dtype = out_dtype;
  p.q = q; p.scale = scale; p.sum = sum; p.vec_dtype = vec_dtype; p.rows = rows; p.cols = cols; p.premul = premul;
  return ln ? launch_rowwise<true>(p, st, what) : launch_rowwise<false>(p, st, what);
}

}  // namespace wanq

using namespace wanq;

extern "C" int wanq_quant_rows(const void* x, int x_dtype, int8_t* q, void* scale, void* sum, int vec_dtype,
                               int64_t rows, int cols, int act, int static_amax, void* stream) {
  WANQ_REQUIRE(x && q && scale, WANQ_E_ARG, "wanq_quant_rows: x, q and scale must be non-NULL");
  WANQ_REQUIRE(is_fp(x_dtype) && is_vec(vec_dtype), WANQ_E_ARG, "wanq_quant_rows: bad dtype code (x=%d vec=%d)", x_dtype, vec_dtype);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "wanq_quant_rows: act must be 0 or 1");
  if (int e = check_rows_cols("wanq_quant_rows", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  if (!static_amax && launch_quant_rows_wave(x, x_dtype, q, scale, sum, vec_dtype, rows, cols, act, (hipStream_t)stream))
    return check_launch("wanq_quant_rows");
  RowParams p{};
  p.levels = 127.0f; p.floor = 1e-6f;
  p.x = x; p.x_dtype = x_dtype; p.q = q; p.scale = scale; p.sum = sum; p.vec_dtype = vec_dtype;
  p.rows = rows; p.cols = cols; p.act = act; p.static_amax = static_amax; p.rows_per_batch = 1;
  return launch_rowwise<false>(p, (hipStream_t)stream, "wanq_quant_rows");
}

extern "C" int wanq_quant_rows_levels(const void* x, int x_dtype, int8_t* q, void* scale, void* sum, int vec_dtype, int64_t rows,
                                      int cols, int n_levels, float floor, void* stream) {
  WANQ_REQUIRE(x && q && scale, WANQ_E_ARG, "wanq_quant_rows_levels: x, q and scale must be non-NULL");
  WANQ_REQUIRE(is_fp(x_dtype) && is_vec(vec_dtype), WANQ_E_ARG, "wanq_quant_rows_levels: bad dtype code (x=%d vec=%d)", x_dtype, vec_dtype);
  WANQ_REQUIRE(n_levels >= 1 && n_levels <= 127, WANQ_E_ARG, "wanq_quant_rows_levels: n_levels=%d must be in [1, 127] (int8 codes)", n_levels);
  WANQ_REQUIRE(floor >= 0.f && floor == floor, WANQ_E_ARG, "wanq_quant_rows_levels: floor must be >= 0");
  if (int e = check_rows_cols("wanq_quant_rows_levels", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  RowParams p{};
  p.x = x; p.x_dtype = x_dtype; p.q = q; p.scale = scale; p.sum = sum; p.vec_dtype = vec_dtype;
  p.rows = rows; p.cols = cols; p.rows_per_batch = 1; p.levels = (float)n_levels; p.floor = floor;
  return launch_rowwise<false>(p, (hipStream_t)stream, "wanq_quant_rows_levels");
}

extern "C" int wanq_quant_rows_fp8(const void* x, int x_dtype, uint8_t* q, float* scale, int64_t rows, int cols, int act,
                                   void* stream) {
  WANQ_REQUIRE(x && q && scale, WANQ_E_ARG, "wanq_quant_rows_fp8: x, q and scale must be non-NULL");
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "wanq_quant_rows_fp8: bad x dtype %d", x_dtype);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "wanq_quant_rows_fp8: act must be 0 or 1");
  if (int e = check_rows_cols("wanq_quant_rows_fp8", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  const Fp8RowParams p{x, x_dtype, q, scale, rows, cols, act};
  row_ladder(cols, rows, [&](auto wpr, auto nch, dim3 grid) {
    hipLaunchKernelGGL((quant_rows_fp8_kernel<decltype(wpr)::value, decltype(nch)::value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  return check_launch("wanq_quant_rows_fp8");
}

template <bool HAD>
static int quant_rows_mx_entry(const char* what, const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int fmt,
                               int act, void* stream) {
  WANQ_REQUIRE(x && q && scale_u8, WANQ_E_ARG, "%s: x, q and scale_u8 must be non-NULL", what);
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "%s: bad x dtype %d", what, x_dtype);
  WANQ_REQUIRE(fmt == WANQ_MX_E4M3 || fmt == WANQ_MX_E2M1, WANQ_E_ARG, "%s: fmt=%d must be WANQ_MX_E4M3 or WANQ_MX_E2M1", what, fmt);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "%s: act must be 0 or 1", what);
  if (int e = check_rows_cols(what, rows, cols)) return e;
  WANQ_REQUIRE(cols % 32 == 0, WANQ_E_SHAPE, "%s: cols=%d must be a multiple of 32 (one scale per block of 32)", what, cols);
  WANQ_REQUIRE((reinterpret_cast<uintptr_t>(q) & 15) == 0, WANQ_E_ARG, "%s: q must be 16-byte aligned", what);
  if (rows == 0) return WANQ_OK;
  const MxRowParams p{x, x_dtype, q, scale_u8, rows, cols, act};
  row_ladder(cols, rows, [&](auto wpr, auto nch, dim3 grid) {
    constexpr int W = decltype(wpr)::value, NC = decltype(nch)::value;
    if (fmt == WANQ_MX_E2M1) hipLaunchKernelGGL((quant_rows_mx_kernel<W, NC, true, HAD>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((quant_rows_mx_kernel<W, NC, false, HAD>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  return check_launch(what);
}

extern "C" int wanq_quant_rows_mx(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int fmt, int act,
                                  void* stream) {
  return quant_rows_mx_entry<false>("wanq_quant_rows_mx", x, x_dtype, q, scale_u8, rows, cols, fmt, act, stream);
}

extern "C" int wanq_quant_rows_mx_had32(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int fmt,
                                        int act, void* stream) {
  return quant_rows_mx_entry<true>("wanq_quant_rows_mx_had32", x, x_dtype, q, scale_u8, rows, cols, fmt, act, stream);
}

extern "C" int wanq_quant_rows_mx6(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, int64_t rows, int cols, int act,
                                   void* stream) {
  const char* what = "wanq_quant_rows_mx6";
  WANQ_REQUIRE(x && q && scale_u8, WANQ_E_ARG, "%s: x, q and scale_u8 must be non-NULL", what);
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "%s: bad x dtype %d", what, x_dtype);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "%s: act must be 0 or 1", what);
  if (int e = check_rows_cols(what, rows, cols)) return e;
  WANQ_REQUIRE(cols % 32 == 0, WANQ_E_SHAPE, "%s: cols=%d must be a multiple of 32 (one scale per block of 32)", what, cols);
  WANQ_REQUIRE((reinterpret_cast<uintptr_t>(q) & 15) == 0, WANQ_E_ARG, "%s: q must be 16-byte aligned", what);
  if (rows == 0) return WANQ_OK;
  const MxRowParams p{x, x_dtype, q, scale_u8, rows, cols, act};
  row_ladder(cols, rows, [&](auto wpr, auto nch, dim3 grid) {
    hipLaunchKernelGGL((quant_rows_mx_kernel<decltype(wpr)::value, decltype(nch)::value, false, false, true>), grid, dim3(256), 0,
                       (hipStream_t)stream, p);
  });
  return check_launch(what);
}

extern "C" int wanq_layernorm_rows(const void* x, int x_dtype, const void* gamma, const void* mshift,
                                   const void* mscale, int mod_dtype, int64_t mod_stride, int64_t rows_per_batch,
                                   float eps, void* out_fp, int out_dtype, int8_t* q, void* scale, void* sum,
                                   int vec_dtype, int64_t rows, int cols, void* stream) {
  WANQ_REQUIRE(x && (out_fp || q), WANQ_E_ARG, "wanq_layernorm_rows: need x and at least one of out_fp / q");
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "wanq_layernorm_rows: bad x dtype %d", x_dtype);
  WANQ_REQUIRE(!(gamma || mshift || mscale) || is_fp(mod_dtype), WANQ_E_ARG, "wanq_layernorm_rows: bad mod dtype %d", mod_dtype);
  WANQ_REQUIRE(!out_fp || is_fp(out_dtype), WANQ_E_ARG, "wanq_layernorm_rows: bad out dtype %d", out_dtype);
  WANQ_REQUIRE(!q || (scale && is_vec(vec_dtype)), WANQ_E_ARG, "wanq_layernorm_rows: q needs scale and a valid vec dtype");
  WANQ_REQUIRE(rows_per_batch >= 1, WANQ_E_ARG, "wanq_layernorm_rows: rows_per_batch must be >= 1");
  if (int e = check_rows_cols("wanq_layernorm_rows", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  RowParams p{};
  p.levels = 127.0f; p.floor = 1e-6f;
  p.x = x; p.x_dtype = x_dtype; p.gamma = gamma; p.mshift = mshift; p.mscale = mscale; p.mod_dtype = mod_dtype;
  p.mod_stride = mod_stride; p.rows_per_batch = rows_per_batch; p.eps = eps; p.out_fp = out_fp; p.out_dtype = out_dtype;
  p.q = q; p.scale = scale; p.sum = sum; p.vec_dtype = vec_dtype; p.rows = rows; p.cols = cols;
  return launch_rowwise<true>(p, (hipStream_t)stream, "wanq_layernorm_rows");
}

extern "C" int wanq_gate_residual(const void* y, int y_dtype, const void* gate, int gate_dtype, int64_t gate_stride,
                                  const void* residual, int res_dtype, void* out, int out_dtype, int64_t rows,
                                  int cols, int64_t rows_per_batch, void* stream) {
  WANQ_REQUIRE(y && gate && residual && out, WANQ_E_ARG, "wanq_gate_residual: NULL pointer");
  WANQ_REQUIRE(is_fp(y_dtype) && is_fp(gate_dtype) && is_fp(res_dtype) && is_fp(out_dtype), WANQ_E_ARG,
               "wanq_gate_residual: bad dtype code");
  WANQ_REQUIRE(rows_per_batch >= 1, WANQ_E_ARG, "wanq_gate_residual: rows_per_batch must be >= 1");
  if (int e = check_rows_cols("wanq_gate_residual", rows, cols)) return e;
  if (rows == 0) return WANQ_OK;
  GateParams p{y, gate, residual, out, y_dtype, gate_dtype, res_dtype, out_dtype, gate_stride, rows_per_batch, rows, cols};
  const int64_t total = rows * (cols / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(gate_residual_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch("wanq_gate_residual");
}
