// Group-wise W8A8 / W4A8 GEMM on gfx950 int8 MFMA (v_mfma_i32_32x32x32_i8): int8 activations against integer weight codes with one
// scale and one zero point per output channel and per group of `group_size` input channels (the W4A8-g128 form of QServe-style
// checkpoints), the sibling of gemm_w8a8.hip's 128 x 128 kernel:
//   part_g[m,n] = sum_{k in group g} a[m,k] * (u[n,k] + zp[g,n])      int32, exact
//   acc         = fma((float)part_g, sw[g,n], acc)                    g ascending from acc = 0
//   y           = fma(acc, sa[m], bias[n]);  GELU;  residual + y * gate;  one rounding to out
//
// Zero point.  The 4-bit operand u + zp[g,n] is formed in registers while the staging pass expands the nibbles, so the matrix cores
// multiply the centred weight itself and no per-token, per-group activation sums are needed.  For every StaticQuantizer output
// u + zp = q + zero_point lies in [-15, 15]; the entry's precondition is the wider "zp integer valued, u + zp in [-128, 127]".  With
// x a dword of four expanded nibbles (each byte <= 15) and z the byte-replicated zp & 0xff,
//   (x + (z & 0x7f7f7f7f)) ^ (z & 0x80808080)
// adds per byte modulo 256: the low seven bits of z plus a nibble stay below 256, so no carry crosses a byte, and the top bit is
// added without carry by the xor.
//
// Structure.  gemm_w8a8_kernel's tile (128 x 128 per 256-thread workgroup, 4 waves as 2 x 2, each 2 x 2 MFMA blocks), its 128-byte
// K step, its two LDS stages with the swizzled 128-B rows, and its operand roles (token on the lane, 16 channels in registers).  A
// group is a whole number of K-tiles (group_size % 128 == 0).  Added to it:
//  * a second accumulator set: part[2][2] (int32) next to accf[2][2] (fp32); the last K-tile of a group folds part into accf with
//    the group's sw row and zeroes part;
//  * the sw row of the tile's 128 channels goes through LDS (two 512-B buffers behind the stages): threads 0-127 load the row of
//    the NEXT K-tile's group next to that tile's operands and write it with them, so the barrier that publishes the tile publishes
//    the row, and a fold reads its 32 values with 8 ds_read_b128 (held in registers for the whole loop they would not fit);
//  * the zp values of a staging thread's four weight rows are fetched one GROUP ahead (at the first tile of group g for g + 1) and
//    are applied when the tile is written to LDS, after the MFMAs: neither waits a memory latency.
// Determinism: one kernel form, no split-K; element (m, n) is summed in an order that depends on K and group_size only.
#include "gemm_i8_common.h"

namespace wanq {
namespace {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 128;
constexpr int STAGE_BYTES = (BM + BN) * BK;        // 32 KiB
constexpr int SWROW = BN * 4;                      // one group's sw row of the tile, fp32
constexpr int LDS_BYTES = 2 * STAGE_BYTES + 2 * SWROW;
constexpr int GROUP_M = 4;                         // m-tiles per L2 panel, as gemm_w8a8_kernel

struct GroupedParams {
  const int8_t* a;
  const int8_t* w;
  void* out;
  const void* sa;
  const float* sw;
  const float* zp;
  const void* bias;
  const float* gate;
  const void* residual;
  int tok_dtype, ch_dtype, epi;
  int M, N, K;
  int mt, nt;
  int tpg;  // K-tiles per group
};

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 4); }

// four outputs of one token: load (residual) and store in the output type
template <int OUT>
__device__ __forceinline__ void load4_out(const void* p, int64_t i, float (&o)[4]) {
  if (OUT == WANQ_F32) {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else if (OUT == WANQ_F16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const __half*>(p) + i);
    const __half2* h = reinterpret_cast<const __half2*>(&v);
    const float2 a = __half22float2(h[0]), b = __half22float2(h[1]);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + i);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  }
}
template <int OUT>
__device__ __forceinline__ void store4_out(void* p, int64_t i, const float (&y)[4]) {
  if constexpr (OUT == WANQ_F32) *reinterpret_cast<float4*>(static_cast<float*>(p) + i) = make_float4(y[0], y[1], y[2], y[3]);
  else *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p) + i) = pack16x4<OUT>(y);  // fp32 value first, then its cast
}

template <int OUT, bool W4>
__global__ __launch_bounds__(256, 2) void gemm_i8_grouped_kernel(const GroupedParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int fr = lane & 31, fh = lane >> 5;

  int m0, n0;
  tile_origin<BM>(blockIdx.x, gridDim.x, p.mt, p.nt, GROUP_M, m0, n0);

  const int K = p.K, N = p.N;
  const int nk = K / BK, tpg = p.tpg, ng = nk / tpg;

  // ---- staging assignment: 4 x 16-B chunks of the activation tile and 4 of the weight tile per thread; rows past M / N are
  // clamped: computed, never stored
  const int8_t* ga[4];
  const int8_t* gw[4];
  const float* gz[4];  // W4: zp[0][n] of the thread's weight rows
  int soff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + 256 * i;
    const int row = id >> 3, c = id & 7;
    const int gm = (m0 + row < p.M) ? (m0 + row) : (p.M - 1);
    const int gn = (n0 + row < N) ? (n0 + row) : (N - 1);
    ga[i] = p.a + (int64_t)gm * K + c * 16;
    gw[i] = W4 ? p.w + (int64_t)gn * (K / 2) + c * 8 : p.w + (int64_t)gn * K + c * 16;
    gz[i] = p.zp ? p.zp + gn : nullptr;
    soff[i] = lds_off(row, c);
  }
  const bool has_zp = W4 && p.zp != nullptr;
  const bool sw_thread = tid < BN;
  const float* gs = p.sw + ((n0 + tid < N) ? (n0 + tid) : (N - 1));  // threads 0-127: sw[0][n0 + tid]

  v4i ra[4], rw[4];  // W4: rw[i].xy are the 8 packed bytes
  float rs = 0.f;             // sw[g][n0 + tid] of the tile in flight (first tile of a group only)
  float zn[4] = {0, 0, 0, 0};  // zp of the NEXT group, as loaded
  uint32_t zlo[4] = {0, 0, 0, 0}, zhi[4] = {0, 0, 0, 0};  // zp of the group being staged, byte-replicated and split
  auto zload = [&](int g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) zn[i] = gz[i][(int64_t)g * N];
  };
  // t: the K-tile to fetch; first: it opens group g
  auto gload = [&](int t, bool first, int g) {
    const int kb = t * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const v4i*>(ga[i] + kb);
      if (W4) {
        const v2i v = *reinterpret_cast<const v2i*>(gw[i] + kb / 2);
        rw[i] = v4i{v.x, v.y, 0, 0};
      } else {
        rw[i] = *reinterpret_cast<const v4i*>(gw[i] + kb);
      }
    }
    if (first) {
      if (sw_thread) rs = gs[(int64_t)g * N];
      if (has_zp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // the values requested a group ago
          const uint32_t z = ((uint32_t)(int)zn[i] & 0xffu) * 0x01010101u;
          zlo[i] = z & 0x7f7f7f7fu;
          zhi[i] = z & 0x80808080u;
        }
        if (g + 1 < ng) zload(g + 1);
      }
    }
  };
  auto lstore = [&](int stage, bool first, int g) {
    char* sx = smem + stage * STAGE_BYTES;
    char* sw = sx + BM * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<v4i*>(sx + soff[i]) = ra[i];
      v4i v = rw[i];
      if (W4) {
        const uint32_t vx = (uint32_t)v.x, vy = (uint32_t)v.y;
        const uint32_t x0 = vx & 0x0f0f0f0fu, x1 = (vx >> 4) & 0x0f0f0f0fu, x2 = vy & 0x0f0f0f0fu, x3 = (vy >> 4) & 0x0f0f0f0fu;
        v = v4i{(int)((x0 + zlo[i]) ^ zhi[i]), (int)((x1 + zlo[i]) ^ zhi[i]), (int)((x2 + zlo[i]) ^ zhi[i]),
                (int)((x3 + zlo[i]) ^ zhi[i])};
      }
      *reinterpret_cast<v4i*>(sw + soff[i]) = v;
    }
    if (first && sw_thread) *reinterpret_cast<float*>(smem + 2 * STAGE_BYTES + (g & 1) * SWROW + tid * 4) = rs;
  };

  const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v16i part[2][2];
  v16f accf[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      part[i][j] = zero16;
      accf[i][j] = __builtin_convertvector(zero16, v16f);
    }

  if (has_zp) zload(0);
  gload(0, true, 0);
  lstore(0, true, 0);
  __syncthreads();

  int g = 0, tin = 0;  // group of tile kt and kt's place in it
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    const bool last = tin + 1 == tpg;  // kt closes group g; then kt + 1 opens g + 1
    if (more) gload(kt + 1, last, g + 1);
    const char* sx = smem + cur * STAGE_BYTES;
    const char* sw = sx + BM * BK;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int chunk = 2 * ks + fh;
      v4i wf[2], xf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) wf[i] = *reinterpret_cast<const v4i*>(sw + lds_off(wn * 64 + i * 32 + fr, chunk));
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = *reinterpret_cast<const v4i*>(sx + lds_off(wm * 64 + j * 32 + fr, chunk));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[i], xf[j], part[i][j], 0, 0, 0);
    }
    if (last) {
      // part[i][j][4 q + e] is channel n0 + wn*64 + i*32 + 8 q + 4 fh + e
      const char* srow = smem + 2 * STAGE_BYTES + (g & 1) * SWROW + (wn * 64 + 4 * fh) * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float4 s4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s4[q] = *reinterpret_cast<const float4*>(srow + (i * 32 + 8 * q) * 4);
        const v16f sv = {s4[0].x, s4[0].y, s4[0].z, s4[0].w, s4[1].x, s4[1].y, s4[1].z, s4[1].w,
                         s4[2].x, s4[2].y, s4[2].z, s4[2].w, s4[3].x, s4[3].y, s4[3].z, s4[3].w};
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // whole vectors: one v_cvt_f32_i32 and one v_fma_f32 per element
          accf[i][j] = __builtin_elementwise_fma(__builtin_convertvector(part[i][j], v16f), sv, accf[i][j]);
          part[i][j] = zero16;
        }
      }
    }
    if (more) lstore(cur ^ 1, last, g + 1);
    __syncthreads();
    if (last) { ++g; tin = 0; } else { ++tin; }
  }

  // ---- epilogue: accf[i][j][4q+e] is (n = n0 + wn*64 + i*32 + 8q + 4*fh + e, m = m0 + wm*64 + j*32 + fr)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm * 64 + j * 32 + fr;
    if (m >= p.M) continue;
    const float sa_m = vec_load(p.sa, p.tok_dtype, m);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 64 + i * 32 + 8 * q + 4 * fh;
        if (n >= N) continue;
        const int64_t o = (int64_t)m * N + n;
        float y[4], b4[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) load4_ch(p.bias, p.ch_dtype, n, b4);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = __fmaf_rn(accf[i][j][4 * q + e], sa_m, b4[e]);
        if (p.epi & WANQ_EPI_GELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = gelu_tanh_fast_f32(y[e]);
        }
        if (p.epi & WANQ_EPI_GATE_RES) {
          float g4[4], r4[4];
          load4_ch(p.gate, WANQ_F32, n, g4);
          load4_out<OUT>(p.residual, o, r4);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = __fmaf_rn(y[e], g4[e], r4[e]);
        }
        store4_out<OUT>(p.out, o, y);
      }
    }
  }
}

template <int OUT, bool W4>
int launch_grouped(const GroupedParams& p, hipStream_t st) {
  static const bool attr_set = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_i8_grouped_kernel<OUT, W4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              LDS_BYTES);
    return true;
  }();
  (void)attr_set;
  hipLaunchKernelGGL((gemm_i8_grouped_kernel<OUT, W4>), dim3((unsigned)(p.mt * p.nt)), dim3(256), LDS_BYTES, st, p);
  return check_launch("wanq_gemm_w8a8_grouped");
}

template <bool W4>
int launch_grouped_out(const GroupedParams& p, int out_dtype, hipStream_t st) {
  switch (out_dtype) {
    case WANQ_F16: return launch_grouped<WANQ_F16, W4>(p, st);
    case WANQ_BF16: return launch_grouped<WANQ_BF16, W4>(p, st);
    default: return launch_grouped<WANQ_F32, W4>(p, st);
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_w8a8_grouped(const int8_t* a, const void* w, int w_bits, const float* sw, const float* zp, int group_size,
                                      void* out, int out_dtype, const void* sa, int tok_dtype, const void* bias, int ch_dtype,
                                      const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_w8a8_grouped";
  WANQ_REQUIRE(a && w && out && sw && sa, WANQ_E_ARG, "%s: a, w, sw, out and sa must be non-NULL", what);
  WANQ_REQUIRE(w_bits == 4 || w_bits == 8, WANQ_E_ARG, "%s: w_bits=%d must be 4 or 8", what, w_bits);
  WANQ_REQUIRE(w_bits == 4 || !zp, WANQ_E_ARG,
               "%s: w_bits=8 takes symmetric weights only, zp must be NULL (c + zp does not fit int8 and no producer writes "
               "per-group token sums)",
               what);
  WANQ_REQUIRE(out_dtype != WANQ_I32, WANQ_E_ARG, "%s: out dtype I32 is refused: there is no single integer accumulator to return",
               what);
  WANQ_REQUIRE(is_fp(out_dtype), WANQ_E_ARG, "%s: out dtype %d must be F16, BF16 or F32", what, out_dtype);
  WANQ_REQUIRE(is_vec(tok_dtype), WANQ_E_ARG, "%s: tok dtype %d must be F16 or F32", what, tok_dtype);
  WANQ_REQUIRE(!bias || is_vec(ch_dtype), WANQ_E_ARG, "%s: ch dtype %d must be F16 or F32", what, ch_dtype);
  WANQ_REQUIRE((epi_flags & ~(WANQ_EPI_GELU | WANQ_EPI_GATE_RES)) == 0, WANQ_E_ARG, "%s: unknown epilogue flag", what);
  WANQ_REQUIRE(!(epi_flags & WANQ_EPI_GATE_RES) || (gate && residual), WANQ_E_ARG, "%s: WANQ_EPI_GATE_RES needs gate and residual",
               what);
  WANQ_REQUIRE(M >= 0 && M < (1ll << 31) - BM, WANQ_E_SHAPE, "%s: M=%lld out of range", what, (long long)M);
  WANQ_REQUIRE(N >= 8 && N % 8 == 0, WANQ_E_SHAPE, "%s: N=%d must be a positive multiple of 8", what, N);
  WANQ_REQUIRE(group_size >= 128 && group_size % 128 == 0, WANQ_E_SHAPE, "%s: group_size=%d must be a positive multiple of 128", what,
               group_size);
  WANQ_REQUIRE(K >= group_size && K % group_size == 0, WANQ_E_SHAPE, "%s: K=%d must be a positive multiple of group_size=%d", what, K,
               group_size);
  WANQ_REQUIRE(aligned_to(a, 16) && aligned_to(w, 16) && aligned_to(out, 16) && aligned_to(residual, 16), WANQ_E_ARG,
               "%s: a, w, out and residual must be 16-byte aligned", what);
  WANQ_REQUIRE(aligned_to(sw, 16) && aligned_to(zp, 16), WANQ_E_ARG, "%s: sw and zp must be 16-byte aligned", what);
  WANQ_REQUIRE(aligned_to(gate, 16) && (!bias || aligned_to(bias, ch_dtype == WANQ_F32 ? 16 : 8)), WANQ_E_ARG,
               "%s: gate and bias must be aligned to 4 elements", what);
  const int64_t mt = (M + BM - 1) / BM, nt = ((int64_t)N + BN - 1) / BN;
  WANQ_REQUIRE(mt * nt < (1ll << 31), WANQ_E_SHAPE, "%s: too many tiles", what);
  if (M == 0) return WANQ_OK;
  GroupedParams p{};
  p.a = a; p.w = static_cast<const int8_t*>(w); p.out = out; p.sa = sa; p.sw = sw; p.zp = zp; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.tok_dtype = tok_dtype; p.ch_dtype = ch_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.mt = (int)mt; p.nt = (int)nt;
  p.tpg = group_size / BK;
  hipStream_t st = (hipStream_t)stream;
  return w_bits == 4 ? launch_grouped_out<true>(p, out_dtype, st) : launch_grouped_out<false>(p, out_dtype, st);
}
