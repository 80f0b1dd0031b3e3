// bf16 / fp16 GEMM with the int8 GEMM's fused epilogue, for the Linears a quant config keeps floating point (HipLinearFp):
//   y[m,n] = sum_k a[m,k] w[n,k]  on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation
//   y = y + bias[n];  y = gelu_tanh(y) (WANQ_EPI_GELU);  y = residual[m,n] + y * gate[n] (WANQ_EPI_GATE_RES);  one rounding to out.
//
// Structure, operand roles and determinism: gemm16_common.h.  Here a K-tile is 128 token rows and 128 weight rows of 128 B, both
// copied by LDS-DMA (8 per wave) into one of two 32-KiB buffers.  One barrier per K-tile:
//   wait for this wave's DMA of tile t | barrier | issue the DMA of tile t+1 into the other buffer | 16 fragment reads of tile t
//   | 32 MFMAs
// so the copy of tile t+1 runs under the reads and MFMAs of tile t, and the buffer it overwrites was last read before every wave
// passed the barrier.  64 KiB of LDS: two workgroups per CU, whose bursts interleave on the SIMDs.
// When K % 64 == 32 the last tile's second half is read from the first half's addresses and its MFMAs are skipped.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int FTILE = (TM + TN) * TROW;  // one K-tile buffer: 32 KiB (token rows 0-127, weight rows 128-255)
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

template <bool F16IN, int OUT>
__global__ void __launch_bounds__(256, 2) gemm_fp16_kernel(FpGemmParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[FLDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / p.nt, tn = blockIdx.x - tm * p.nt;
  const int m0 = tm * TM, n0 = tn * TN;
  const int K = p.K, nk = (K + TK - 1) / TK;

  // ---- LDS-DMA sources: instruction q (0-7) of this wave fills LDS rows 8 g .. 8 g + 7, g = 4 q + wave (q < 4: token rows, see
  // token_dma_sources; q >= 4: weight rows, the same lane -> row, chunk map 128 rows further down)
  const uint16_t *src[4], *wsrc[4];
  token_dma_sources(p.a, m0, p.M, K, wave, lane, src);
  int kc = 0;  // logical chunk of this lane (the same for all eight instructions: 8 g is a multiple of 16 / 2)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + wave) + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    kc = c;
    const int n = n0 + r < p.N ? n0 + r : p.N - 1;
    wsrc[q] = p.w + (int64_t)n * K + c * 8;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int t) {
    // k past K only in the second half of a last tile when K % 64 == 32: re-read the first half (never multiplied)
    const int koff = t * TK + kc * 8 < K ? t * TK : t * TK - 32;
    char* dst = smem + (t & 1) * FTILE + wave * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(src[q] + koff), (lds_void*)(dst + q * 4096), 16, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(wsrc[q] + koff), (lds_void*)(dst + (4 + q) * 4096), 16, 0, 0);
  };

  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t rd0 = frag_addr(lds0, fr, fq, 0), rd1 = frag_addr(lds0, fr, fq, 1);

  v4f acc[4][4];
  zero_acc(acc);

  issue(0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue(t + 1);
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t boff = (t & 1) * FTILE;
    const uint32_t a0 = rd0 + boff + wm * 64 * TROW, a1 = rd1 + boff + wm * 64 * TROW;
    const uint32_t b0 = rd0 + boff + (TM + wn * 64) * TROW, b1 = rd1 + boff + (TM + wn * 64) * TROW;
    v4i xa[2][4], wb[2][4];
    dsr<0>(wb[0][0], b0); dsr<16 * TROW>(wb[0][1], b0); dsr<32 * TROW>(wb[0][2], b0); dsr<48 * TROW>(wb[0][3], b0);
    dsr<0>(xa[0][0], a0); dsr<16 * TROW>(xa[0][1], a0); dsr<32 * TROW>(xa[0][2], a0); dsr<48 * TROW>(xa[0][3], a0);
    dsr<0>(wb[1][0], b1); dsr<16 * TROW>(wb[1][1], b1); dsr<32 * TROW>(wb[1][2], b1); dsr<48 * TROW>(wb[1][3], b1);
    dsr<0>(xa[1][0], a1); dsr<16 * TROW>(xa[1][1], a1); dsr<32 * TROW>(xa[1][2], a1); dsr<48 * TROW>(xa[1][3], a1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const bool half = t * TK + 32 >= K;  // K % 64 == 32, last tile: its second 32-deep step does not exist
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

  epilogue16<OUT, false>(acc, m0, n0, wm, wn, fr, fq, p.M, p.N, nullptr, p.bias, p.bias_dtype, p.gate, p.residual, p.out, p.epi);
}

template <bool F16IN, int OUT>
int launch(const FpGemmParams& p, hipStream_t st) {
  const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
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

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_bf16(const void* a, const void* w, int dtype, void* out, int out_dtype, const void* bias, int bias_dtype,
                              const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_bf16";
  WANQ_REQUIRE(a && w && out, WANQ_E_ARG, "%s: a, w and out must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  if (const int rc = check_gemm16_shapes(what, 32, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  FpGemmParams p{};
  p.a = static_cast<const uint16_t*>(a); p.w = static_cast<const uint16_t*>(w); p.out = out; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.bias_dtype = bias_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.nt = (N + TN - 1) / TN;
  hipStream_t st = (hipStream_t)stream;
  return dtype == WANQ_F16 ? launch_out<true>(p, out_dtype, st) : launch_out<false>(p, out_dtype, st);
}
