// fp8 (OCP e4m3fn) W8A8 GEMM: per-token dynamic e4m3 activations against per-channel e4m3 weights (HipLinearFp8), with the fused
// epilogue of the 16-bit GEMMs:
//   acc[m,n] = sum_k a[m,k] w[n,k]  on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands, unit block scales), fp32 accumulation
//   y = fmaf(acc * sa[m], sw[n], bias[n]);  GELU;  residual + y * gate;  one rounding to out  (epilogue16<.., TOKEN>).
//
// Structure, operand roles and determinism: gemm16_common.h, as gemm_bf16.hip uses it.  An fp8 row of a K-tile is half the bytes of a
// bf16 row, so a K-tile here is 128 deep and the LDS image is the bf16 kernel's byte for byte: 128 token rows and 128 weight rows
// of 128 B, the 16-B chunk index XORed with (row >> 1) & 7, both halves copied by LDS-DMA (8 per wave) into one of two 32-KiB
// buffers, one barrier per K-tile, the copy of tile t+1 under the reads and MFMAs of tile t.
//
// Matrix instruction.  The block-scaled 16x16x128 MFMA with both formats e4m3 and both scales 2^0 (E8M0 127) multiplies plain fp8
// at twice the rate of v_mfma_f32_16x16x32_fp8_fp8 (which runs at the bf16 rate): one MFMA per 16 x 16 block and K-tile instead of
// four.  Both forms passed the operand-map and integer probes of tests/test_gpu_fp8.py; this one measured faster on both FFN
// shapes (profiles/gemm_fp8.txt) and is the one kept.
//
// Fragments.  The MFMA takes 32 bytes per lane and operand: lane l, row l & 15, 32 k of lane group l >> 4.  A lane keeps the bf16
// kernel's two 16-byte reads -- logical chunk 4 kk + fq of the 64-deep step kk = 0, 1, fq = l >> 4 -- as the low and the high half of
// its fragment.  Both operands are cut the same way, so slot j of lane group fq holds the same k on either side, whichever k the
// hardware calls it.  Per K-tile: 16 reads, 16 MFMAs.  K % 64 == 0: when K % 128 == 64 the last tile's second step is read from the
// first step's addresses and replaced by zeros in both fragments (+0 products: the sum is that of the 64 real k).
//
// Summation order of element (m, n): K-tiles ascending, inside an MFMA the hardware's own.  It depends on K only.
#include "gemm16_common.h"

namespace wanq {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int TK8 = 128;                 // fp8 elements of a K-tile: TROW bytes per LDS row
constexpr int KSTEP8 = 64;               // the K multiple: one 16-byte fragment read per lane, half of an MFMA's K
constexpr int FTILE = (TM + TN) * TROW;  // one K-tile buffer: 32 KiB (token rows 0-127, weight rows 128-255)
constexpr int FLDS = 2 * FTILE;
static_assert(TK8 == TROW, "an fp8 K-tile row fills the 128-byte LDS row");

struct Fp8GemmParams {
  const uint8_t* a;
  const uint8_t* w;
  const float* sa;
  const float* sw;
  void* out;
  const void* bias;
  const float* gate;
  const void* residual;
  int bias_dtype, epi;
  int M, N, K, nt;
};

// one 128-deep MFMA: the fragments of step 0 (low 16 bytes) and step 1 (high 16 bytes); e4m3 x e4m3, scales 2^0
__device__ __forceinline__ v4f mfma128(const v4i& w0, const v4i& w1, const v4i& x0, const v4i& x1, v4f c) {
  const v8i w = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w}, x = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

template <int OUT>
__global__ void __launch_bounds__(256, 2) gemm_fp8_kernel(Fp8GemmParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[FLDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / p.nt, tn = blockIdx.x - tm * p.nt;
  const int m0 = tm * TM, n0 = tn * TN;
  const int K = p.K, nk = (K + TK8 - 1) / TK8;

  // ---- LDS-DMA sources: instruction q (0-7) of this wave fills LDS rows 8 g .. 8 g + 7, g = 4 q + wave (q < 4: token rows, q >= 4:
  // weight rows 128 further down); lane l writes row 8 g + (l >> 3), physical chunk l & 7 = logical chunk c ^ ((row >> 1) & 7).
  // Rows past M / N are read from row M - 1 / N - 1 (computed, never stored).
  const uint8_t *src[4], *wsrc[4];
  int kc = 0;  // logical chunk of this lane (the same for all eight instructions: 8 g is a multiple of 16 / 2)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + wave) + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    kc = c;
    const int m = m0 + r < p.M ? m0 + r : p.M - 1;
    const int n = n0 + r < p.N ? n0 + r : p.N - 1;
    src[q] = p.a + (int64_t)m * K + c * 16;
    wsrc[q] = p.w + (int64_t)n * K + c * 16;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int t) {
    // k past K only in the second step of a last tile when K % 128 == 64: re-read the first step (never multiplied)
    const int koff = t * TK8 + kc * 16 < K ? t * TK8 : t * TK8 - KSTEP8;
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
    const bool half = t * TK8 + KSTEP8 >= K;  // K % 128 == 64, last tile: its second 64-deep step does not exist
    const v4i z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma128(wb[0][j], half ? z : wb[1][j], xa[0][i], half ? z : xa[1][i], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
  }

  epilogue16<OUT, true, true>(acc, m0, n0, wm, wn, fr, fq, p.M, p.N, p.sw, p.bias, p.bias_dtype, p.gate, p.residual, p.out, p.epi,
                              p.sa);
}

template <int OUT>
int launch(const Fp8GemmParams& p, hipStream_t st) {
  const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
  hipLaunchKernelGGL((gemm_fp8_kernel<OUT>), dim3((unsigned)tiles), dim3(256), 0, st, p);
  return check_launch("wanq_gemm_fp8");
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_fp8(const uint8_t* a, const uint8_t* w, const float* sa, const float* sw, void* out, int out_dtype,
                             const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M,
                             int N, int K, void* stream) {
  const char* what = "wanq_gemm_fp8";
  WANQ_REQUIRE(a && w && out && sa && sw, WANQ_E_ARG, "%s: a, w, sa, sw and out must be non-NULL", what);
  if (const int rc = check_gemm16_shapes(what, KSTEP8, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  WANQ_REQUIRE(aligned(sw, 16) && aligned(sa, 4), WANQ_E_ARG, "%s: sw must be 16-byte aligned and sa 4-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  Fp8GemmParams p{};
  p.a = a; p.w = w; p.sa = sa; p.sw = sw; p.out = out; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.bias_dtype = bias_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.nt = (N + TN - 1) / TN;
  hipStream_t st = (hipStream_t)stream;
  switch (out_dtype) {
    case WANQ_F16: return launch<WANQ_F16>(p, st);
    case WANQ_BF16: return launch<WANQ_BF16>(p, st);
    default: return launch<WANQ_F32>(p, st);
  }
}
