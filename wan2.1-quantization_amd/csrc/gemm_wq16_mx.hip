// W4A16 MXFP4 GEMM (wanq_gemm_wq16_mx): 16-bit activations against OCP MXFP4 weights -- packed e2m1 codes [N, K / 2] in the layout
// of wanq_gemm_mx (element k in byte k / 2, even k in the low nibble) with one E8M0 scale byte per 32 input channels [N, K / 32] --
// for the Linears of a config that says `weight: {format: mxfp4_e2m1, weight_only: True}` and has no `act:` section (HipLinearWq16Mx):
//   r       = sw_u8[n, k / 32] - row_exp[n]
//   op[n,k] = e2m1(w[n,k]) 2^r  for RLO <= r <= 13, else 0 for r < RLO   (RLO = -13 fp16, -112 bf16)
//   acc     = sum_k a[m,k] op[n,k]   on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation
//   y       = fma(acc, 2^(row_exp[n] - 127), bias[n]);  GELU, gate + residual, one rounding (epilogue16 with EXP8).
//
// Exactness.  An E8M0 scale is a power of two and an e2m1 magnitude (0, 0.5, 1, 1.5, 2, 3, 4, 6) has at most two significant bits, so
// value 2^r is a bf16 / fp16 number whenever it is in the type's normal range: the scale is ADDED TO THE EXPONENT FIELD of the 16-bit
// operand and never touches an fp32 accumulator.  gemm_wq16.hip's grouped form needs a second accumulator set and a fold per group
// because an arbitrary fp32 scale cannot ride in the operand; this kernel has neither.  row_exp, one reference exponent per output
// channel chosen by the caller, centres the row's blocks in the operand's range (fp16: 27 binades, r in [-13, 13]; bf16: [-112, 13])
// and comes back in the epilogue's one fma as an exact power of two.  Blocks below the range are flushed to zero, as a whole.
//
// Structure.  gemm_wq16.hip's frame: the token half of a K-tile goes by LDS-DMA into one of two 16-KiB buffers, the weight half
// never touches LDS.  Each lane loads, one K-tile ahead, what its own MFMA fragments need and decodes next to the MFMAs:
//   wait for this wave's DMA, codes and scales of tile t | barrier | issue the DMA of tile t+1 | decode the codes of tile t | load
//   the codes and scales of tile t+1 | 8 fragment reads of tile t | 32 MFMAs
// A 64-deep K-tile is two MX blocks and a 32-deep MFMA step kk is one, so every fragment dword a lane builds in a step shares one r.
//
// Fragment cut.  A lane holds channel fr = lane & 15 of each of its four 16-channel blocks j and, in step kk, the 8 codes at
// k = 64 t + 32 kk + 8 fq, fq = lane >> 4.  In the plain packed layout these are the 4 bytes at byte 32 t + 16 kk + 4 fq of the row:
// dword 8 t + 4 kk + fq, code k0 + i in bits 4 i .. 4 i + 3 (wanq_pack_w4's layout interleaves low and high nibbles instead).  The
// operand fragment is 4 dwords, element k0 + 2 d in the low half of dword d and k0 + 2 d + 1 in the high half.  8 dword loads per lane
// and K-tile, plus 4 two-byte loads: the two scale bytes of tile t of each channel, sw_u8[n, 2 t .. 2 t + 1] (2-byte aligned for every
// n since K / 32 is even; a dword for two tiles would be unaligned for odd n K / 64 and is not built).  row_exp of the lane's four
// channels stays in registers, as q0[j] = row_exp + RLO.
//
// Decode (decode8).  Per block: q = s - q0[j] = r - RLO; q < 0 clears the code dword (every magnitude and sign 0: the flush).  The
// eight 16-bit table entries are kept rebased by RLO binades as constant pairs (bf16 0x0700 0780 07C0 0800 0840 0880 08C0, fp16
// 0x0400 0800 0A00 0C00 0E00 1000 1200, entry 0 = 0) so that the exponent add q << 7 / q << 10 is non-negative and two entries add
// in one 32-bit instruction without a carry between halves (q <= 125 / 26); entry 0 gets none.  Two v_perm_b32 per pool split the
// four pairs into a low-byte pool and a high-byte pool of 8 bytes each (fp16: every low byte is 0, no low pool); the magnitudes of
// the even and of the odd codes are two selector dwords (w & 0x07070707, (w >> 4) & 0x07070707), looked up with one v_perm_b32 per
// pool, four codes each; the signs go into the high bytes (v_and_or_b32) and the bytes are interleaved into the four operand dwords
// by v_perm_b32 again (bf16: 4 + 4; fp16: 4, with the selector's zero byte for the low halves).
//
// Decode cost, per lane and K-tile (64 codes -> 32 operand dwords, 8 blocks), next to 32 MFMAs and next to gemm_wq16.hip's 2.75 /
// 2.9 vector instructions per code of W8 / W4:
//   per block, the table: scale byte, q, compare, clear, shift, replicate, 4 adds, 2 (fp16) or 4 (bf16) splits   = 12 / 14
//   per block, the codes: 3 selectors, 3 signs, 2 / 4 lookups, 4 / 8 interleaves                                  = 12 / 18
//   fp16: 24 per block = 192 per K-tile = 3.0 per code;  bf16: 32 per block = 256 per K-tile = 4.0 per code
// and no fold.  Like gemm_wq16.hip's conversion this does not hide in one wave's MFMA shadow; it overlaps with the other workgroup
// on the SIMD (32 KiB of LDS, two per CU).  Registers and timings of the build: profiles/gemm_wq16_mx.txt.
//
// Outside the contract.  r > 13 (the layer never writes such a byte: its row_exp puts the row's largest block at r = 13): the
// exponent add may run into the sign or the next entry -- the result is unspecified, but every access stays in bounds (the decode
// is register arithmetic).  Scale byte 255, OCP's NaN: the host's mx_decode reads it as the exponent 2^128 (no NaN, +-inf after the
// cast to fp32 for a nonzero code), and here it is the plain byte too, r = 255 - row_exp: in the contract for row_exp >= 242, else r > 13.
// row_exp = 255 makes the epilogue's factor +inf.
//
// Determinism.  gemm_bf16.hip's summation order (gemm16_common.h): with row_exp = 127 and bias NULL the output is bit-equal to
// wanq_gemm_bf16 on op cast to the activation dtype, and a row gives the same bits in any launch.  tests/test_gpu_wq16_mx.py.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int QLDS = 2 * XTILE;  // two K-tile buffers of token rows, 16 KiB each

// V_PERM_B32: byte i of the result is byte sel[i] of the 8 bytes (hi : lo) for sel[i] < 8, 0x00 for sel[i] = 12
__host__ __device__ __forceinline__ uint32_t perm8(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else  // (the host's model of the four selector values this file uses: a stand-alone check of decode8 runs it)
  const uint64_t pool = ((uint64_t)hi << 32) | lo;
  uint32_t d = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 0xffu;
    d |= (s < 8 ? (uint32_t)(pool >> (8 * s)) & 0xffu : 0u) << (8 * i);
  }
  return d;
#endif
}

template <bool F16IN>
struct MxOp {
  static constexpr int SH = F16IN ? 10 : 7;       // the exponent field's place in the 16-bit operand
  static constexpr int RLO = F16IN ? -13 : -112;  // the lowest r whose products are all normal
  // entries 2 i | 2 i + 1 << 16 of magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6, rebased by RLO binades
  static constexpr uint32_t C01 = F16IN ? 0x04000000u : 0x07000000u, C23 = F16IN ? 0x0A000800u : 0x07C00780u;
  static constexpr uint32_t C45 = F16IN ? 0x0E000C00u : 0x08400800u, C67 = F16IN ? 0x12001000u : 0x08C00880u;
};

// the 8 codes of dword w (code i in bits 4 i .. 4 i + 3) with q = r - RLO -> the 4 operand dwords of e2m1(code) 2^r; q < 0: zeros
template <bool F16IN>
__host__ __device__ __forceinline__ void decode8(uint32_t w, int q, int (&d)[4]) {
  using O = MxOp<F16IN>;
  w = q < 0 ? 0u : w;
  const uint32_t qq = (uint32_t)q << O::SH, qq2 = (qq << 16) | qq;
  const uint32_t e01 = (qq << 16) + O::C01, e23 = qq2 + O::C23, e45 = qq2 + O::C45, e67 = qq2 + O::C67;
  const uint32_t hi0 = perm8(e23, e01, 0x07050301u), hi1 = perm8(e67, e45, 0x07050301u);
  const uint32_t se = w & 0x07070707u, so = (w >> 4) & 0x07070707u;  // magnitudes of codes 0, 2, 4, 6 and of 1, 3, 5, 7
  const uint32_t he = ((w << 4) & 0x80808080u) | perm8(hi1, hi0, se), ho = (w & 0x80808080u) | perm8(hi1, hi0, so);
  if constexpr (F16IN) {
    d[0] = (int)perm8(ho, he, 0x040c000cu); d[1] = (int)perm8(ho, he, 0x050c010cu);
    d[2] = (int)perm8(ho, he, 0x060c020cu); d[3] = (int)perm8(ho, he, 0x070c030cu);
  } else {
    const uint32_t lo0 = perm8(e23, e01, 0x06040200u), lo1 = perm8(e67, e45, 0x06040200u);
    const uint32_t le = perm8(lo1, lo0, se), lo = perm8(lo1, lo0, so);
    const uint32_t x01 = perm8(he, le, 0x05010400u), x23 = perm8(he, le, 0x07030602u);  // elements 0, 2 and 4, 6
    const uint32_t y01 = perm8(ho, lo, 0x05010400u), y23 = perm8(ho, lo, 0x07030602u);  // elements 1, 3 and 5, 7
    d[0] = (int)perm8(y01, x01, 0x05040100u); d[1] = (int)perm8(y01, x01, 0x07060302u);
    d[2] = (int)perm8(y23, x23, 0x05040100u); d[3] = (int)perm8(y23, x23, 0x07060302u);
  }
}

// Gemm16Params with w: packed e2m1 [N, K / 2]; sa: E8M0 bytes [N, K / 32]; sw: row_exp uint8 [N] (the epilogue's EXP8 factor)
template <bool F16IN, int OUT>
__global__ void __launch_bounds__(256, 2) gemm_wq16_mx_kernel(Gemm16Params p) {
  __shared__ __attribute__((aligned(1024))) char smem[QLDS];
  const Frame f(p.nt);
  const int K = p.K, nk = K / TK;

  const char* src[4];  // LDS-DMA sources (token rows only)
  dma_sources(p.a, f.m0, p.M, (int64_t)K * 2, f, src);
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int t) { dma_issue<4>(src, (int64_t)(t * TK) * 2, smem + (t & 1) * XTILE + f.wave * 1024); };
  const uint32_t rd0 = frag_addr(lds0, f.fr, f.fq, 0), rd1 = frag_addr(lds0, f.fr, f.fq, 1);

  // ---- this lane's weight side: channel block j -> its code dwords (header: the fragment cut), its scale byte pairs, its row_exp
  const uint8_t *wp[4], *sp[4];
  int q0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nr = f.n0 + f.wn * 64 + j * 16 + f.fr;
    const int n = nr < p.N ? nr : p.N - 1;
    wp[j] = static_cast<const uint8_t*>(p.w) + (int64_t)n * (K / 2) + f.fq * 4;
    sp[j] = static_cast<const uint8_t*>(p.sa) + (int64_t)n * (K / 32);
    q0[j] = (int)static_cast<const uint8_t*>(p.sw)[n] + MxOp<F16IN>::RLO;
  }
  uint32_t raw[2][4], sraw[4];  // sraw: scale byte of step 0 | step 1 << 8
  auto load_codes = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sraw[j] = *reinterpret_cast<const uint16_t*>(sp[j] + (int64_t)t * 2);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) raw[kk][j] = *reinterpret_cast<const uint32_t*>(wp[j] + (int64_t)t * 32 + kk * 16);
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
        int d[4];
        decode8<F16IN>(raw[kk][j], (int)((sraw[j] >> (8 * kk)) & 0xffu) - q0[j], d);
        wb[kk][j] = v4i{d[0], d[1], d[2], d[3]};
      }
    load_codes(t + 1 < nk ? t + 1 : t);  // last tile: re-read itself (never used)
    const uint32_t xo = (t & 1) * XTILE + f.wm * 64 * TROW;
    v4i xa[2][4];
    dsr4<TROW>(xa[0], rd0 + xo);
    dsr4<TROW>(xa[1], rd1 + xo);
    // tied to the fragments: the MFMAs that read them cannot be scheduled above the wait, while the decode stays free to interleave
    // with the MFMAs (gemm_wq16.hip)
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

  epilogue16<OUT, true, false, false, true>(acc, acc, f, p);
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_wq16_mx(const void* a, const uint8_t* w, int dtype, const uint8_t* sw_u8, const uint8_t* row_exp, void* out,
                                 int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual,
                                 int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_wq16_mx";
  WANQ_REQUIRE(a && w && out && sw_u8 && row_exp, WANQ_E_ARG, "%s: a, w, out, sw_u8 and row_exp must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  if (const int rc = check_gemm16_shapes(what, 64, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  WANQ_REQUIRE(aligned(sw_u8, 16) && aligned(row_exp, 16), WANQ_E_ARG, "%s: sw_u8 and row_exp must be 16-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const Gemm16Params p = gemm16_params(a, w, sw_u8, row_exp, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  return with_out_dtype(out_dtype, [&](auto o) {
    constexpr int OUT = decltype(o)::value;
    return dtype == WANQ_F16 ? launch_tiles(gemm_wq16_mx_kernel<true, OUT>, p, (hipStream_t)stream, what)
                             : launch_tiles(gemm_wq16_mx_kernel<false, OUT>, p, (hipStream_t)stream, what);
  });
}
