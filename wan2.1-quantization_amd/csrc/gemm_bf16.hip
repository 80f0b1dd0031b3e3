// bf16 / fp16 GEMM with the int8 GEMM's fused epilogue, for the Linears a quant config keeps floating point (HipLinearFp):
//   y[m,n] = sum_k a[m,k] w[n,k]  on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation
//   y = y + bias[n];  y = gelu_tanh(y) (WANQ_EPI_GELU);  y = residual[m,n] + y * gate[n] (WANQ_EPI_GATE_RES);  one rounding to out.
//
// Structure.  One 128(M) x 128(N) output tile per 256-thread workgroup (4 waves, 2 x 2, 64 x 64 each = 4 x 4 MFMA tiles), K in
// tiles of 64.  A K-tile (128 token rows and 128 weight rows of 128 B) is copied global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, 8 per wave) into one of two 32-KiB buffers; rows are 128 B with the 16-B chunk index XORed with
// (row >> 1) & 7, on the DMA source address and on the fragment reads (the LDS image of gemm_w8a8_pp.hip: a 16x16x32 bf16
// fragment takes the same 16 bytes per lane as a 16x16x64 int8 one).  One barrier per K-tile:
//   wait for this wave's DMA of tile t | barrier | issue the DMA of tile t+1 into the other buffer | 16 fragment reads of tile t
//   | 32 MFMAs
// so the copy of tile t+1 runs under the reads and MFMAs of tile t, and the buffer it overwrites was last read before every wave
// passed the barrier.  64 KiB of LDS: two workgroups per CU, whose bursts interleave on the SIMDs.
//
// The MFMA takes the WEIGHT fragment as its A operand and the token fragment as B, so a lane's four accumulators are four
// consecutive channels of one token: bias / gate loads and the stores are 4-wide vectors.
//
// Determinism.  Every output element is summed by one lane, over k in K-tile order and within a tile in two 32-deep MFMA steps:
// its fp32 summation order depends on K only -- not on M, on the row's place in the launch or on which workgroup ran it.  There
// is no split-K and one kernel form.  Rows past M are read from row M - 1 (computed, never stored); channels past N likewise.
// When K % 64 == 32 the last tile's second half is read from the first half's addresses and its MFMAs are skipped.
#include "gemm_params.h"

namespace wanq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

constexpr int FM = 128, FN = 128, FK = 64;
constexpr int FROW = FK * 2;                // bytes of one LDS row
constexpr int FTILE = (FM + FN) * FROW;     // one K-tile buffer: 32 KiB (token rows 0-127, weight rows 128-255)
constexpr int FLDS = 2 * FTILE;

struct FpGemmParams {
  const uint16_t* a;
  const uint16_t* w;
  void* out;
  const void* bias;
  const float* gate;
  const void* residual;
  int bias_dtype, epi;
  int M, N, K, nt;
};

template <int OFF>
__device__ __forceinline__ void dsr(v4i& d, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

template <bool F16IN>
__device__ __forceinline__ v4f mfma(const v4i& a, const v4i& b, const v4f& c) {
  if constexpr (F16IN) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
  }
}

// four consecutive per-channel values of dtype F16 / BF16 / F32
__device__ __forceinline__ void load4_any(const void* p, int dt, int idx, float (&o)[4]) {
  if (dt == WANQ_BF16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p) + idx);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
    load4_ch(p, dt, idx, o);
  }
}

template <int OUT>
__device__ __forceinline__ void load4_out(const void* p, int64_t idx, float (&o)[4]) {
  if constexpr (OUT == WANQ_F32) {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + idx);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    load4_any(static_cast<const uint16_t*>(p) + idx, OUT, 0, o);
  }
}

template <int OUT>
__device__ __forceinline__ void store4_out(void* p, int64_t idx, const float (&y)[4]) {
  if constexpr (OUT == WANQ_F32) {
    *reinterpret_cast<float4*>(static_cast<float*>(p) + idx) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
    *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p) + idx) = pack16x4<OUT>(y);
  }
}

template <bool F16IN, int OUT>
__global__ void __launch_bounds__(256, 2) gemm_fp16_kernel(FpGemmParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[FLDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / p.nt, tn = blockIdx.x - tm * p.nt;
  const int m0 = tm * FM, n0 = tn * FN;
  const int K = p.K, nk = (K + FK - 1) / FK;

  // ---- LDS-DMA sources: instruction q (0-7) of this wave fills LDS rows 8 g .. 8 g + 7, g = 4 q + wave (q < 4: token rows,
  // q >= 4: weight rows); lane l writes row 8 g + (l >> 3), physical chunk l & 7 = logical chunk c ^ ((row >> 1) & 7)
  const uint16_t* src[8];
  const int lrow = lane >> 3, pchunk = lane & 7;
  int kc = 0;  // logical chunk of this lane (the same for all eight instructions: 8 g is a multiple of 16 / 2)
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = 8 * (4 * q + wave) + lrow;
    const int c = pchunk ^ ((r >> 1) & 7);
    kc = c;
    if (q < 4) {
      const int m = m0 + r < p.M ? m0 + r : p.M - 1;
      src[q] = p.a + (int64_t)m * K + c * 8;
    } else {
      const int n = n0 + r - FM < p.N ? n0 + r - FM : p.N - 1;
      src[q] = p.w + (int64_t)n * K + c * 8;
    }
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int t) {
    // k past K only in the second half of a last tile when K % 64 == 32: re-read the first half (never multiplied)
    const int koff = t * FK + kc * 8 < K ? t * FK : t * FK - 32;
    char* dst = smem + (t & 1) * FTILE + wave * 1024;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(src[q] + koff), (lds_void*)(dst + q * 4096), 16, 0, 0);
  };

  // ---- fragment reads: lane l reads row (16-row block) + (l & 15), logical chunk 4 kk + (l >> 4)
  const int fr = lane & 15, fq = lane >> 4, sw = (fr >> 1) & 7;
  const uint32_t rd0 = lds0 + fr * FROW + ((fq ^ sw) << 4), rd1 = lds0 + fr * FROW + (((4 + fq) ^ sw) << 4);

  v4f acc[4][4];  // [token block i][channel block j]: channel (lane >> 4) * 4 + e, token lane & 15
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue(t + 1);
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t boff = (t & 1) * FTILE;
    const uint32_t a0 = rd0 + boff + wm * 64 * FROW, a1 = rd1 + boff + wm * 64 * FROW;
    const uint32_t b0 = rd0 + boff + (FM + wn * 64) * FROW, b1 = rd1 + boff + (FM + wn * 64) * FROW;
    v4i xa[2][4], wb[2][4];
    dsr<0>(wb[0][0], b0); dsr<16 * FROW>(wb[0][1], b0); dsr<32 * FROW>(wb[0][2], b0); dsr<48 * FROW>(wb[0][3], b0);
    dsr<0>(xa[0][0], a0); dsr<16 * FROW>(xa[0][1], a0); dsr<32 * FROW>(xa[0][2], a0); dsr<48 * FROW>(xa[0][3], a0);
    dsr<0>(wb[1][0], b1); dsr<16 * FROW>(wb[1][1], b1); dsr<32 * FROW>(wb[1][2], b1); dsr<48 * FROW>(wb[1][3], b1);
    dsr<0>(xa[1][0], a1); dsr<16 * FROW>(xa[1][1], a1); dsr<32 * FROW>(xa[1][2], a1); dsr<48 * FROW>(xa[1][3], a1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const bool half = t * FK + 32 >= K;  // K % 64 == 32, last tile: its second 32-deep step does not exist
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma<F16IN>(wb[0][j], xa[0][i], acc[i][j]);
    if (!half) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma<F16IN>(wb[1][j], xa[1][i], acc[i][j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- epilogue, fp32: + bias, GELU, residual + y * gate, one rounding
  const bool gelu = p.epi & WANQ_EPI_GELU, gres = p.epi & WANQ_EPI_GATE_RES;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + fq * 4;
    if (n >= p.N) continue;
    float b4[4] = {0.f, 0.f, 0.f, 0.f}, g4[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) load4_any(p.bias, p.bias_dtype, n, b4);
    if (gres) load4_ch(p.gate, WANQ_F32, n, g4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fr;
      if (m >= p.M) continue;
      const int64_t o = (int64_t)m * p.N + n;
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = acc[i][j][e] + b4[e];
      if (gelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = gelu_tanh_fast_f32(y[e]);
      }
      if (gres) {
        float r4[4];
        load4_out<OUT>(p.residual, o, r4);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = r4[e] + y[e] * g4[e];
      }
      store4_out<OUT>(p.out, o, y);
    }
  }
}

template <bool F16IN, int OUT>
int launch(const FpGemmParams& p, hipStream_t st) {
  const int64_t tiles = (int64_t)((p.M + FM - 1) / FM) * p.nt;
  hipLaunchKernelGGL((gemm_fp16_kernel<F16IN, OUT>), dim3((unsigned)tiles), dim3(256), 0, st, p);
  return check_launch("wanq_gemm_bf16");
}

template <bool F16IN>
int launch_out(const FpGemmParams& p, int out_dtype, hipStream_t st) {
  switch (out_dtype) {
    case WANQ_F16: return launch<F16IN, WANQ_F16>(p, st);
    case WANQ_BF16: return launch<F16IN, WANQ_BF16>(p, st);
    default: return launch<F16IN, WANQ_F32>(p, st);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_bf16(const void* a, const void* w, int dtype, void* out, int out_dtype, const void* bias, int bias_dtype,
                              const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_bf16";
  WANQ_REQUIRE(a && w && out, WANQ_E_ARG, "%s: a, w and out must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  WANQ_REQUIRE(is_fp(out_dtype), WANQ_E_ARG, "%s: out dtype %d must be BF16, F16 or F32", what, out_dtype);
  WANQ_REQUIRE(!bias || is_fp(bias_dtype), WANQ_E_ARG, "%s: bias dtype %d must be BF16, F16 or F32", what, bias_dtype);
  WANQ_REQUIRE((epi_flags & ~(WANQ_EPI_GELU | WANQ_EPI_GATE_RES)) == 0, WANQ_E_ARG, "%s: unknown epilogue flag", what);
  WANQ_REQUIRE(!(epi_flags & WANQ_EPI_GATE_RES) || (gate && residual), WANQ_E_ARG, "%s: WANQ_EPI_GATE_RES needs gate and residual",
               what);
  WANQ_REQUIRE(M >= 0 && M < (1ll << 31) - FM, WANQ_E_SHAPE, "%s: M=%lld out of range", what, (long long)M);
  WANQ_REQUIRE(N >= 8 && N % 8 == 0, WANQ_E_SHAPE, "%s: N=%d must be a positive multiple of 8", what, N);
  WANQ_REQUIRE(K >= 32 && K % 32 == 0, WANQ_E_SHAPE, "%s: K=%d must be a positive multiple of 32", what, K);
  WANQ_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(out, 16) && aligned(residual, 16), WANQ_E_ARG,
               "%s: a, w, out and residual must be 16-byte aligned", what);
  WANQ_REQUIRE(aligned(gate, 16) && (!bias || aligned(bias, bias_dtype == WANQ_F32 ? 16 : 8)), WANQ_E_ARG,
               "%s: gate and bias must be aligned to 4 elements", what);
  if (M == 0) return WANQ_OK;
  FpGemmParams p{};
  p.a = static_cast<const uint16_t*>(a); p.w = static_cast<const uint16_t*>(w); p.out = out; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.bias_dtype = bias_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.nt = (N + FN - 1) / FN;
  WANQ_REQUIRE(((M + FM - 1) / FM) * p.nt < (1ll << 31), WANQ_E_SHAPE, "%s: too many tiles", what);
  hipStream_t st = (hipStream_t)stream;
  return dtype == WANQ_F16 ? launch_out<true>(p, out_dtype, st) : launch_out<false>(p, out_dtype, st);
}
