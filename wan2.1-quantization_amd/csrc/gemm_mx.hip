// OCP MX GEMM: MXFP8 (e4m3) activations against MXFP8 (e4m3) or MXFP4 (e2m1) weights, one E8M0 power-of-two scale per row and block
// of 32 input channels on either side (HipLinearMx), with the fused epilogue of the 16-bit GEMMs:
//   acc[m,n] = sum_b 2^(sa[m,b]-127) 2^(sw[n,b]-127) sum_{k in b} a[m,k] w[n,k]  on v_mfma_scale_f32_16x16x128_f8f6f4, which applies
//   both block scales itself; fp32 accumulation.   y = acc + bias;  GELU;  residual + y * gate;  one rounding to out
//   (epilogue16<.., false>: no fp32 row or channel scale is left to apply).
//
// Structure, operand roles and determinism: gemm16_common.h, as gemm_fp8.hip uses it -- 128 x 128 tile, 4 waves, a 128-deep K-tile,
// both halves copied by LDS-DMA into one of two buffers, one barrier per K-tile, the copy of tile t+1 under the reads and MFMAs of
// tile t.  Three things differ from gemm_fp8.hip.
//
// Fragment cut, as probes 1-3 of tests/test_gpu_mx.py found it on the hardware (not as the instruction's summary suggests).  Lane l
// holds row l & 15.  An 8-bit operand's eight fragment registers are two 64-deep halves: registers 0-3 of lane group fq = l >> 4 are
// the K-tile's k 16 fq .. 16 fq + 15, registers 4-7 are k 64 + 16 fq .. 64 + 16 fq + 15 -- the 16-byte chunks fq and 4 + fq of the
// row, which is exactly gemm_fp8.hip's cut.  A 4-bit operand's four registers are the 32 CONSECUTIVE k 32 fq .. 32 fq + 31 (the one
// 16-byte chunk fq of a packed row, even k in the low nibble).  The scale operand of lane (row, fq) is the E8M0 byte of that row's
// block fq = k 32 fq .. 32 fq + 31 of the K-tile in both cases: for an e2m1 operand that is the lane's own fragment, for an e4m3
// operand the block's elements sit in lane groups 2 fq mod 4 and 2 fq mod 4 + 1 (half fq >> 1), but the byte still comes from
// lane group fq.  So a one-block-per-lane cut of the e4m3 rows multiplies the wrong k against an e2m1 weight and scales the wrong
// blocks; with the cut below every operand and both scale maps agree with the stored format.
//
// LDS image.  e4m3 rows (tokens, and e4m3 weights) are gemm_fp8.hip's byte for byte: 128-B rows, the 16-B chunk index XORed with
// (row >> 1) & 7, read at chunks fq and 4 + fq (frag_addr), conflict-free.  A packed e2m1 weight row of a K-tile is 64 B: the weight
// half is 128 rows of 64 B (8 KiB, 2 DMA instructions per wave, each 16 rows), logical chunk c at physical chunk c ^ g((row >> 2) &
// 3), g(u) = u ^ ((u & 1) << 1).  Four such rows make one 256-B bank line; a ds_read_b128 group holds rows {0-3, 12-15} of lane
// group fq and rows {4-11} of fq ^ 1, i.e. per row residue mod 4 the chunks fq ^ g(0), fq ^ g(3), fq ^ 1 ^ g(1), fq ^ 1 ^ g(2) = fq ^
// {0, 1, 2, 3}: all sixteen 16-byte slots, no conflict.
//
// Scale operands.  A row's four E8M0 bytes of a K-tile are one aligned dword of sa_u8 / sw_u8 (K % 128 == 0).  A lane loads the dword of
// each of its four token rows and four weight rows once per K-tile -- for tile t + 1 right behind the DMA of tile t + 1, so the
// wait that covers the DMA covers them -- and shifts it right by 8 fq: byte 0 (op_sel 0) is then the byte of its own (row, block).
//
// Matrix instruction.  The weight is the first operand: cbsz 0 (e4m3, eight fragment registers) or 4 (e2m1, the first four), the
// token operand stays e4m3 (blgp 0).
//
// Summation order of element (m, n): K-tiles ascending, inside an MFMA the hardware's own.  It depends on K only.
#include "gemm16_common.h"

namespace wanq {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int TKX = 128;            // elements of a K-tile: four blocks of 32, one MFMA
constexpr int XTILE = TM * TROW;    // token half of a K-tile buffer: 16 KiB
constexpr int W4ROW = TKX / 2;      // bytes of a packed e2m1 weight row of a K-tile
static_assert(TKX == TROW, "an e4m3 K-tile row fills the 128-byte LDS row");

template <bool FP4>
struct MxGeom {
  static constexpr int WTILE = TN * (FP4 ? W4ROW : TROW);  // weight half: 8 KiB or 16 KiB
  static constexpr int TILE = XTILE + WTILE;
  static constexpr int NWQ = WTILE / 4096;                 // DMA instructions per wave for the weight half
};

struct MxGemmParams {
  const uint8_t* a;
  const uint8_t* w;
  const uint8_t* sa;
  const uint8_t* sw;
  void* out;
  const void* bias;
  const float* gate;
  const void* residual;
  int bias_dtype, epi;
  int M, N, K, nt;
};

__device__ __forceinline__ int w4_swz(int r) {
  const int u = (r >> 2) & 3;
  return u ^ ((u & 1) << 1);
}

template <bool FP4>
__device__ __forceinline__ v4f mfma_mx(const v4i& w0, const v4i& w1, const v4i& x0, const v4i& x1, v4f c, int sw, int sa) {
  const v8i x = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  if constexpr (FP4) {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 0, 0, sw, 0, sa);
  } else {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, sw, 0, sa);
  }
}

template <int OUT, bool FP4>
__global__ void __launch_bounds__(256, 2) gemm_mx_kernel(MxGemmParams p) {
  using G = MxGeom<FP4>;
  __shared__ __attribute__((aligned(1024))) char smem[2 * G::TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / p.nt, tn = blockIdx.x - tm * p.nt;
  const int m0 = tm * TM, n0 = tn * TN;
  const int K = p.K, nk = K / TKX, KB = K / 32;

  // ---- LDS-DMA sources.  Token rows (and e4m3 weight rows): instruction q (0-3) of this wave fills LDS rows 8 g .. 8 g + 7, g = 4 q +
  // wave; lane l writes row 8 g + (l >> 3), physical chunk l & 7 = logical chunk c ^ ((row >> 1) & 7).  e2m1 weight rows: instruction q (0-1) fills rows 16 g .. 16 g + 15,
  // lane l row 16 g + (l >> 2), physical chunk l & 3.  Rows past M / N are read from row M - 1 / N - 1 (computed, never stored).
  const uint8_t *src[4], *wsrc[G::NWQ];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + wave) + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int m = m0 + r < p.M ? m0 + r : p.M - 1;
    src[q] = p.a + (int64_t)m * K + c * 16;
    if constexpr (!FP4) {
      const int n = n0 + r < p.N ? n0 + r : p.N - 1;
      wsrc[q] = p.w + (int64_t)n * K + c * 16;
    }
  }
  if constexpr (FP4) {
#pragma unroll
    for (int q = 0; q < G::NWQ; ++q) {
      const int r = 16 * (4 * q + wave) + (lane >> 2);
      const int c = (lane & 3) ^ w4_swz(r);
      const int n = n0 + r < p.N ? n0 + r : p.N - 1;
      wsrc[q] = p.w + (int64_t)n * (K / 2) + c * 16;
    }
  }
  constexpr int WSTEP = FP4 ? W4ROW : TKX;  // bytes of a weight row per K-tile
  auto issue = [&](int t) {
    char* dst = smem + (t & 1) * G::TILE + wave * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(src[q] + t * TKX), (lds_void*)(dst + q * 4096), 16, 0, 0);
#pragma unroll
    for (int q = 0; q < G::NWQ; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(wsrc[q] + t * WSTEP), (lds_void*)(dst + XTILE + q * 4096), 16, 0, 0);
  };

  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const uint32_t rd0 = frag_addr(lds0, fr, fq, 0), rd1 = frag_addr(lds0, fr, fq, 1);
  const uint32_t rdw4 = lds0 + fr * W4ROW + ((fq ^ w4_swz(fr)) << 4);

  // ---- scale bytes: the dword of K-tile t of this lane's four token rows and four weight rows, shifted to its own block
  const uint32_t *sap[4], *swp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mr = m0 + wm * 64 + i * 16 + fr, nr = n0 + wn * 64 + i * 16 + fr;
    sap[i] = reinterpret_cast<const uint32_t*>(p.sa + (int64_t)(mr < p.M ? mr : p.M - 1) * KB);
    swp[i] = reinterpret_cast<const uint32_t*>(p.sw + (int64_t)(nr < p.N ? nr : p.N - 1) * KB);
  }
  const int sh = 8 * fq;
  uint32_t sa_nxt[4], sw_nxt[4];
  auto load_scales = [&](int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_nxt[i] = sap[i][t];
      sw_nxt[i] = swp[i][t];
    }
  };

  v4f acc[4][4];
  zero_acc(acc);

  issue(0);
  load_scales(0);
  for (int t = 0; t < nk; ++t) {
    int sa_cur[4], sw_cur[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_cur[i] = (int)(sa_nxt[i] >> sh);
      sw_cur[i] = (int)(sw_nxt[i] >> sh);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) {
      issue(t + 1);
      load_scales(t + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t boff = (t & 1) * G::TILE;
    const uint32_t a0 = rd0 + boff + wm * 64 * TROW, a1 = rd1 + boff + wm * 64 * TROW;
    v4i xa[2][4], wb[2][4];
    if constexpr (FP4) {
      const uint32_t b0 = rdw4 + boff + XTILE + wn * 64 * W4ROW;
      dsr<0>(wb[0][0], b0); dsr<16 * W4ROW>(wb[0][1], b0); dsr<32 * W4ROW>(wb[0][2], b0); dsr<48 * W4ROW>(wb[0][3], b0);
    } else {
      const uint32_t b0 = rd0 + boff + XTILE + wn * 64 * TROW, b1 = rd1 + boff + XTILE + wn * 64 * TROW;
      dsr<0>(wb[0][0], b0); dsr<16 * TROW>(wb[0][1], b0); dsr<32 * TROW>(wb[0][2], b0); dsr<48 * TROW>(wb[0][3], b0);
      dsr<0>(wb[1][0], b1); dsr<16 * TROW>(wb[1][1], b1); dsr<32 * TROW>(wb[1][2], b1); dsr<48 * TROW>(wb[1][3], b1);
    }
    dsr<0>(xa[0][0], a0); dsr<16 * TROW>(xa[0][1], a0); dsr<32 * TROW>(xa[0][2], a0); dsr<48 * TROW>(xa[0][3], a0);
    dsr<0>(xa[1][0], a1); dsr<16 * TROW>(xa[1][1], a1); dsr<32 * TROW>(xa[1][2], a1); dsr<48 * TROW>(xa[1][3], a1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma_mx<FP4>(wb[0][j], wb[FP4 ? 0 : 1][j], xa[0][i], xa[1][i], acc[i][j], sw_cur[j], sa_cur[i]);
    __builtin_amdgcn_sched_barrier(0);
  }

  epilogue16<OUT, false>(acc, m0, n0, wm, wn, fr, fq, p.M, p.N, nullptr, p.bias, p.bias_dtype, p.gate, p.residual, p.out, p.epi);
}

template <int OUT>
int launch(const MxGemmParams& p, bool fp4, hipStream_t st) {
  const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
  if (fp4) hipLaunchKernelGGL((gemm_mx_kernel<OUT, true>), dim3((unsigned)tiles), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((gemm_mx_kernel<OUT, false>), dim3((unsigned)tiles), dim3(256), 0, st, p);
  return check_launch("wanq_gemm_mx");
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_mx(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, int w_fmt, void* out,
                            int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags,
                            int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_mx";
  WANQ_REQUIRE(a && w && out && sa_u8 && sw_u8, WANQ_E_ARG, "%s: a, w, sa_u8, sw_u8 and out must be non-NULL", what);
  WANQ_REQUIRE(w_fmt == WANQ_MX_E4M3 || w_fmt == WANQ_MX_E2M1, WANQ_E_ARG, "%s: w_fmt=%d must be WANQ_MX_E4M3 or WANQ_MX_E2M1", what,
               w_fmt);
  if (const int rc = check_gemm16_shapes(what, TKX, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  WANQ_REQUIRE(aligned(sa_u8, 4) && aligned(sw_u8, 4), WANQ_E_ARG, "%s: sa_u8 and sw_u8 must be 4-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  MxGemmParams p{};
  p.a = a; p.w = w; p.sa = sa_u8; p.sw = sw_u8; p.out = out; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.bias_dtype = bias_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.nt = (N + TN - 1) / TN;
  hipStream_t st = (hipStream_t)stream;
  const bool fp4 = w_fmt == WANQ_MX_E2M1;
  switch (out_dtype) {
    case WANQ_F16: return launch<WANQ_F16>(p, fp4, st);
    case WANQ_BF16: return launch<WANQ_BF16>(p, fp4, st);
    default: return launch<WANQ_F32>(p, fp4, st);
  }
}
