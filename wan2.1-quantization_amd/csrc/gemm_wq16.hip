// Weight-only quantised GEMM (W8A16 / W4A16): 16-bit activations against integer weight codes, the sibling of gemm_bf16.hip for
// the Linears of a quant config with a `weight:` section and no `act:` section (HipLinearWq16):
//   y[m,n] = sw[n] * sum_k a[m,k] (c[n,k] + zp[n])  on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation
//   y = fma(acc, sw[n], bias[n]);  y = gelu_tanh(y) (WANQ_EPI_GELU);  y = residual[m,n] + y * gate[n] (WANQ_EPI_GATE_RES);  one
//   rounding to out.
//
// Exactness.  c + zp is an integer with |c + zp| <= 255 for every StaticQuantizer output (8-bit asymmetric: c in [-128, 127],
// zp in [-127, 128]; 4-bit: nibbles 0..15 with zp = zero_point - 8), and such an integer is exact in bf16 (8 significant bits) and
// in fp16, so the matrix cores get the weight WITHOUT any rounding and every product a (c + zp) is exact in fp32.  sw is applied
// once, in fp32, in the epilogue (one fma with the bias).  The reference multiplies (c + zp) delta first and, under autocast, rounds
// that product to bf16 before F.linear (ViDiT-Q/quant_utils/qdiff/base/quant_layer.py:68-72): this path is the more exact one.
// zp must be integer valued (every StaticQuantizer zero point is): the 16-bit operand is cut from the fp32 sum c + zp, not rounded.
//
// Structure.  gemm_bf16.hip's tile, MFMA operand roles and epilogue (gemm16_common.h); the TOKEN half of a K-tile goes into one of
// two 16-KiB buffers.  The WEIGHT half never touches LDS and no dequantised copy is written anywhere: each lane loads the codes of
// its own MFMA fragments straight from global memory -- channel (lane & 15) of each of its four 16-channel blocks, the 8 codes at
// k = 32 kk + 8 (lane >> 4) of each of the two 32-deep steps: 8 bytes (W8, global_load_dwordx2) or the one dword of wanq_pack_w4's
// 16-byte group that holds exactly those 8 nibbles (W4, global_load_dword); 8 loads per lane per K-tile -- one K-tile ahead, into
// registers, and converts them next to the MFMAs:
//   wait for this wave's DMA and codes of tile t | barrier | issue the DMA of tile t+1 | convert the codes of tile t | load the
//   codes of tile t+1 | 8 fragment reads of tile t | 32 MFMAs
// The two waves that share a channel half load and convert the same codes (L1 / L2 hits).
//
// Conversion cost, per lane and K-tile (64 codes -> 32 operand dwords), next to 32 MFMAs:
//   W8: 16 v_xor (c + 128 as an unsigned byte) + 64 v_cvt_f32_ubyte{0-3} + 64 v_add_f32 (zp - 128) + 32 packs
//       (bf16: v_perm_b32 of the two high halves; fp16: v_cvt_pkrtz_f16_f32, exact here)               = 176 vector instructions
//   W4: 8 v_and + 8 v_lshrrev + 8 v_and (nibbles -> bytes) + 64 + 64 + 32                             = 184 vector instructions
// i.e. 2.75 / 2.9 per code and 5.5 / 5.75 per MFMA, against ~16 cycles of matrix core per MFMA: the conversion does not hide
// inside one wave's MFMA shadow; it overlaps with the MFMAs of the other workgroup on the SIMD (32 KiB of LDS, two per CU).
//
// Determinism.  gemm_bf16.hip's summation order (gemm16_common.h), so with sw = 1 the output is bit-equal to wanq_gemm_bf16 on the
// weight (c + zp) cast to the activation dtype.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int QTILE = TM * TROW;  // one K-tile buffer: 16 KiB of token rows
constexpr int QLDS = 2 * QTILE;

struct WqGemmParams {
  const uint16_t* a;
  const uint8_t* w;
  void* out;
  const float* sw;
  const float* zp;
  const void* bias;
  const float* gate;
  const void* residual;
  int bias_dtype, epi;
  int M, N, K, nt;
};

// two integer-valued floats (|x| <= 256) -> one dword of the 16-bit operand type, exactly
template <bool F16IN>
__device__ __forceinline__ int pack2(float lo, float hi) {
  if constexpr (F16IN) {
    return __builtin_bit_cast(int, __builtin_amdgcn_cvt_pkrtz(lo, hi));
  } else {
    return (int)__builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
  }
}

// four unsigned bytes u (codes k .. k + 3 from the low byte up) + z -> two operand dwords
template <bool F16IN>
__device__ __forceinline__ void cvt4(uint32_t u, float z, int& d0, int& d1) {
  const float f0 = (float)(u & 0xffu) + z, f1 = (float)((u >> 8) & 0xffu) + z;
  const float f2 = (float)((u >> 16) & 0xffu) + z, f3 = (float)(u >> 24) + z;
  d0 = pack2<F16IN>(f0, f1);
  d1 = pack2<F16IN>(f2, f3);
}

template <bool F16IN, bool W4, int OUT>
__global__ void __launch_bounds__(256, 2) gemm_wq16_kernel(WqGemmParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[QLDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x / p.nt, tn = blockIdx.x - tm * p.nt;
  const int m0 = tm * TM, n0 = tn * TN;
  const int K = p.K, nk = K / TK;

  const uint16_t* src[4];  // LDS-DMA sources (token rows only)
  token_dma_sources(p.a, m0, p.M, K, wave, lane, src);
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int t) {
    char* dst = smem + (t & 1) * QTILE + wave * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(src[q] + t * TK), (lds_void*)(dst + q * 4096), 16, 0, 0);
  };

  // ---- fragment geometry: lane l holds row (16-row block) + (l & 15), the 8 k of logical chunk 4 kk + (l >> 4)
  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t rd0 = frag_addr(lds0, fr, fq, 0), rd1 = frag_addr(lds0, fr, fq, 1);

  // ---- weight codes of this lane: channel block j, step kk -> W8: 8 bytes at k = 64 t + 32 kk + 8 fq; W4: dword fq of the 16-byte
  // group of codes 64 t + 32 kk .. + 31 (low nibbles = codes 8 fq .. + 3, high nibbles = codes 8 fq + 4 .. + 7)
  constexpr int CT = W4 ? TK / 2 : TK;  // bytes of codes per row and K-tile
  const uint8_t* wp[4];
  float zadj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nr = n0 + wn * 64 + j * 16 + fr;
    const int n = nr < p.N ? nr : p.N - 1;
    wp[j] = p.w + (int64_t)n * (W4 ? K / 2 : K) + fq * (CT / 8);
    zadj[j] = (p.zp ? p.zp[n] : 0.f) - (W4 ? 0.f : 128.f);
  }
  uint2 raw[2][4];  // W4 uses .x only
  auto load_codes = [&](int t) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* s = wp[j] + (int64_t)t * CT + kk * (CT / 2);
        if constexpr (W4) raw[kk][j].x = *reinterpret_cast<const uint32_t*>(s);
        else raw[kk][j] = *reinterpret_cast<const uint2*>(s);
      }
  };

  v4f acc[4][4];
  zero_acc(acc);

  issue(0);
  load_codes(0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue(t + 1);
    __builtin_amdgcn_sched_barrier(0);
    v4i wb[2][4];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t u0, u1;
        if constexpr (W4) {
          u0 = raw[kk][j].x & 0x0f0f0f0fu; u1 = (raw[kk][j].x >> 4) & 0x0f0f0f0fu;
        } else {
          u0 = raw[kk][j].x ^ 0x80808080u; u1 = raw[kk][j].y ^ 0x80808080u;
        }
        int d0, d1, d2, d3;
        cvt4<F16IN>(u0, zadj[j], d0, d1);
        cvt4<F16IN>(u1, zadj[j], d2, d3);
        wb[kk][j] = v4i{d0, d1, d2, d3};
      }
    load_codes(t + 1 < nk ? t + 1 : t);  // last tile: re-read itself (never used)
    const uint32_t boff = (t & 1) * QTILE;
    const uint32_t a0 = rd0 + boff + wm * 64 * TROW, a1 = rd1 + boff + wm * 64 * TROW;
    v4i xa[2][4];
    dsr<0>(xa[0][0], a0); dsr<16 * TROW>(xa[0][1], a0); dsr<32 * TROW>(xa[0][2], a0); dsr<48 * TROW>(xa[0][3], a0);
    dsr<0>(xa[1][0], a1); dsr<16 * TROW>(xa[1][1], a1); dsr<32 * TROW>(xa[1][2], a1); dsr<48 * TROW>(xa[1][3], a1);
    // tied to the fragments: the MFMAs that read them cannot be scheduled above the wait (the compiler does not count the asm
    // reads in lgkmcnt), while the conversion of the codes stays free to interleave with the MFMAs
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(xa[0][0]), "+v"(xa[0][1]), "+v"(xa[0][2]), "+v"(xa[0][3]), "+v"(xa[1][0]), "+v"(xa[1][1]), "+v"(xa[1][2]),
                   "+v"(xa[1][3])
                 :
                 : "memory");
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma<F16IN>(wb[kk][j], xa[kk][i], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
  }

  epilogue16<OUT, true>(acc, m0, n0, wm, wn, fr, fq, p.M, p.N, p.sw, p.bias, p.bias_dtype, p.gate, p.residual, p.out, p.epi);
}

template <bool F16IN, bool W4, int OUT>
int launch(const WqGemmParams& p, hipStream_t st) {
  const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
  hipLaunchKernelGGL((gemm_wq16_kernel<F16IN, W4, OUT>), dim3((unsigned)tiles), dim3(256), 0, st, p);
  return check_launch("wanq_gemm_wq16");
}

template <bool F16IN, bool W4>
int launch_out(const WqGemmParams& p, int out_dtype, hipStream_t st) {
  switch (out_dtype) {
    case WANQ_F16: return launch<F16IN, W4, WANQ_F16>(p, st);
    case WANQ_BF16: return launch<F16IN, W4, WANQ_BF16>(p, st);
    default: return launch<F16IN, W4, WANQ_F32>(p, st);
  }
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_wq16(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp, void* out,
                              int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual,
                              int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_wq16";
  WANQ_REQUIRE(a && w && out && sw, WANQ_E_ARG, "%s: a, w, out and sw must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  WANQ_REQUIRE(w_bits == 4 || w_bits == 8, WANQ_E_ARG, "%s: w_bits=%d must be 4 or 8", what, w_bits);
  if (const int rc = check_gemm16_shapes(what, 64, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  WANQ_REQUIRE(aligned(sw, 16) && aligned(zp, 16), WANQ_E_ARG, "%s: sw and zp must be 16-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  WqGemmParams p{};
  p.a = static_cast<const uint16_t*>(a); p.w = static_cast<const uint8_t*>(w); p.out = out; p.sw = sw; p.zp = zp; p.bias = bias;
  p.gate = (epi_flags & WANQ_EPI_GATE_RES) ? gate : nullptr;
  p.residual = (epi_flags & WANQ_EPI_GATE_RES) ? residual : nullptr;
  p.bias_dtype = bias_dtype; p.epi = epi_flags;
  p.M = (int)M; p.N = N; p.K = K; p.nt = (N + TN - 1) / TN;
  hipStream_t st = (hipStream_t)stream;
  if (w_bits == 4) return dtype == WANQ_F16 ? launch_out<true, true>(p, out_dtype, st) : launch_out<false, true>(p, out_dtype, st);
  return dtype == WANQ_F16 ? launch_out<true, false>(p, out_dtype, st) : launch_out<false, false>(p, out_dtype, st);
}
