// OCP MX GEMMs: MXFP8 (e4m3) activations against MXFP8 (e4m3) or MXFP4 (e2m1) weights (wanq_gemm_mx), MXFP4 activations against
// MXFP4 weights (wanq_gemm_mx4, W4A4), and MXFP6 (e2m3) activations against MXFP6 or MXFP4 weights (wanq_gemm_mx6, W6A6 / W4A6), one E8M0 power-of-two scale per row and block of 32 input channels on either side
// (HipLinearMx), with the fused epilogue of the 16-bit GEMMs:
//   acc[m,n] = sum_b 2^(sa[m,b]-127) 2^(sw[n,b]-127) sum_{k in b} a[m,k] w[n,k]  on v_mfma_scale_f32_16x16x128_f8f6f4, which applies
//   both block scales itself; fp32 accumulation.   y = acc + bias;  GELU;  residual + y * gate;  one rounding to out
//   (epilogue16<.., false>: no fp32 row or channel scale is left to apply).
//
// Structure, the K loop (gemm_tile_kernel), operand roles and determinism: gemm16_common.h, with gemm_fp8.hip's 128-deep K-tile.
// Three things differ from gemm_fp8.hip.
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
// 3), g(u) = u ^ ((u & 1) << 1) (w4_swz, gemm16_common.h).  Four such rows make one 256-B bank line; a ds_read_b128 group holds
// rows {0-3, 12-15} of lane group fq and rows {4-11} of fq ^ 1, i.e. per row residue mod 4 the chunks fq ^ g(0), fq ^ g(3), fq ^ 1 ^
// g(1), fq ^ 1 ^ g(2) = fq ^ {0, 1, 2, 3}: all sixteen 16-byte slots, no conflict.
//
// Scale operands.  A row's four E8M0 bytes of a K-tile are one aligned dword of sa_u8 / sw_u8 (K % 128 == 0).  A lane loads the dword of
// each of its four token rows and four weight rows once per K-tile -- for tile t + 1 right behind the DMA of tile t + 1, so the
// wait that covers the DMA covers them -- and shifts it right by 8 fq: byte 0 (op_sel 0) is then the byte of its own (row, block).
//
// Matrix instruction.  The weight is the first operand: cbsz 0 (e4m3, eight fragment registers) or 4 (e2m1, the first four); the
// token operand is the second: blgp 0 (e4m3) or 4 (e2m1).
//
// W4A4 (wanq_gemm_mx4).  The token half is what the packed weight half is: 128 rows of 64 B, two DMA instructions per wave, w4_swz,
// one ds_read_b128 of chunk fq per fragment, registers 4-7 zero.  A wave reads token rows wm * 64 + i * 16 + fr exactly as it reads
// weight rows wn * 64 + j * 16 + fr, so the bank derivation above holds for both halves.  A K-tile buffer is 16 KiB, a fragment
// set 8 reads instead of 12 (16), and with both operands 4 bits wide the instruction runs at the fp4 rate, twice the rate any
// e4m3 operand holds it to.  The scale dwords do not change.  128-deep K-tile, one MFMA per accumulator and barrier.
//
// W6A6 / W4A6 (wanq_gemm_mx6, Mx6Policy).  A 6-bit operand is cut like a 4-bit one: the six fragment registers of lane (row, fq) are
// the 32 CONSECUTIVE k 32 fq .. 32 fq + 31 of the K-tile, element j in bits 6 j .. 6 j + 5 of the 192-bit little-endian string the
// registers make, the scale byte that of block fq (probes A and B of tests/test_gpu_mx6.py, both operand sides; they passed on the
// first version of the kernel).  That string is the stored format (include/wanq_hip.h: block b of a row at bytes 24 b .. 24 b + 23),
// so nothing is re-packed: cbsz / blgp 2, registers 6-7 zero.  A packed e2m3 row of a K-tile is 96 B (W6ROW, the third row geometry
// of gemm16_common.h): a half is 128 rows x 96 B = 12 KiB = 768 16-byte chunks, three 1-KiB LDS-DMA instructions per wave, LDS chunk
// g = row g / 6, physical chunk g % 6, lane-linear; a K-tile buffer is 24 KiB (W6A6) or 20 KiB (W4A6, the weight half as above).
// Reads and banks.  The 24 bytes of block fq start at byte 24 fq of the row: 8-byte aligned, 16-byte aligned for even fq only, and a
// ds_read_b128 off its alignment is replayed.  So a fragment is read as its three 8-byte pieces p = 0, 1, 2, piece p = 8-byte slot
// 3 fq + p of the row's twelve, by ds_read_b64 (conflict-free it moves 256 B per clock, as ds_read_b128 does: 3 x 2 LDS cycles per
// fragment against 4 + 2 for a b128 + b64 pair that only even fq could use).  A ds_read_b64 is served in two groups of 32 lanes,
// lanes 0-31 = rows fr 0-15 of lane groups fq 0 and 1 (lanes 32-63: fq 2 and 3), bank (a / 4) mod 64, i.e. 32 slots of 8 bytes.
// Unswizzled, row fr's slot 3 fq + p sits at 12 fr + 3 fq + p mod 32, and 12 fr mod 32 takes only the eight multiples of 4, each
// for fr and fr + 8: two-way conflicts, half the slots unused.  Swizzle (w6_swz, on the DMA source address and on the reads): logical
// chunk c of row r at physical chunk c ^ ((r >> 3) & 1), which stays inside the row's six chunks.  Piece p of lane groups fq = 0, 1
// reads half h0 of logical chunk c0 and half h1 != h0 of chunk c1 ((c, h) = ((3 fq + p) >> 1, (3 fq + p) & 1): p = 0: (0, 0), (1, 1);
// p = 1: (0, 1), (2, 0); p = 2: (1, 0), (2, 1); fq = 2, 3 the same three chunks up), so the two lane groups take slots of opposite
// parity, and within one lane group the chunk positions 6 fr + (c ^ (fr >> 3)) mod 16 are, for fr = 0-7, the eight positions of
// c's parity and, for fr = 8-15, the eight of the other parity: sixteen distinct 16-byte positions, 32 distinct slots per group, no
// conflict.  Row offsets of the 16-row blocks (1536 B) and of the halves (12 KiB, 8 KiB) are multiples of 256 B and leave the banks
// alone.  A fragment set is 24 ds_read_b64 (W6A6) or 12 + 4 ds_read_b128 (W4A6); the pieces are assembled into the operand
// registers behind the wait, without a move (the K loop holds none).
//
// Summation order of element (m, n): K-tiles ascending, inside an MFMA the hardware's own.  It depends on K only.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int TKX = 128;  // elements of a K-tile: four blocks of 32, one MFMA

template <bool FP4, bool A4>
__device__ __forceinline__ v4f mfma_mx(const v4i& w0, const v4i& w1, const v4i& x0, const v4i& x1, v4f c, int sw, int sa) {
  if constexpr (A4) {
    static_assert(FP4, "e2m1 tokens go with e2m1 weights");
    const v8i w = {w0.x, w0.y, w0.z, w0.w, 0, 0, 0, 0}, x = {x0.x, x0.y, x0.z, x0.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 4, 0, sw, 0, sa);
  }
  const v8i x = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  if constexpr (FP4) {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 0, 0, sw, 0, sa);
  } else {
    const v8i w = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, sw, 0, sa);
  }
}

// scale bytes: the dword of K-tile t of this lane's four token rows and four weight rows, loaded one tile ahead and shifted to the
// lane's own block
struct MxScales {
  const uint32_t *sap[4], *swp[4];
  uint32_t sa_nxt[4], sw_nxt[4];
  int sa_cur[4], sw_cur[4], sh;

  __device__ __forceinline__ MxScales(const Gemm16Params& p, const Frame& f) : sh(8 * f.fq) {
    const int KB = p.K / 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mr = f.m0 + f.wm * 64 + i * 16 + f.fr, nr = f.n0 + f.wn * 64 + i * 16 + f.fr;
      sap[i] = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(p.sa) + (int64_t)(mr < p.M ? mr : p.M - 1) * KB);
      swp[i] = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(p.sw) + (int64_t)(nr < p.N ? nr : p.N - 1) * KB);
    }
  }
  __device__ __forceinline__ void load(int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_nxt[i] = sap[i][t];
      sw_nxt[i] = swp[i][t];
    }
  }
  __device__ __forceinline__ void shift() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sa_cur[i] = (int)(sa_nxt[i] >> sh);
      sw_cur[i] = (int)(sw_nxt[i] >> sh);
    }
  }
};

template <int OUT_, bool FP4, bool A4 = false>
struct MxPolicy {
  static constexpr int OUT = OUT_, TKE = TKX, KMUL = TKX, WROW = FP4 ? W4ROW : TROW, XROW = A4 ? W4ROW : TROW;
  static constexpr bool SCALED = false, TOKEN = false;
  using Side = MxScales;

  static __device__ __forceinline__ void mma(v4f (&acc)[4][4], const v4i (&wb)[2][4], const v4i (&xa)[2][4], const Side& s, bool) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma_mx<FP4, A4>(wb[0][j], wb[FP4 ? 0 : 1][j], xa[0][i], xa[A4 ? 0 : 1][i], acc[i][j], s.sw_cur[j], s.sa_cur[i]);
  }
};

// e2m3 tokens (blgp 2, six fragment registers) against e2m3 (cbsz 2) or e2m1 (cbsz 4) weights; the pieces are assembled behind the wait
template <bool W4>
__device__ __forceinline__ v4f mfma_mx6(const v4i& w4, const v2i& w0, const v2i& w1, const v2i& w2, const v2i& x0, const v2i& x1,
                                        const v2i& x2, v4f c, int sw, int sa) {
  const v8i x = {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y, 0, 0};
  if constexpr (W4) {
    const v8i w = {w4.x, w4.y, w4.z, w4.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 4, 2, 0, sw, 0, sa);
  } else {
    const v8i w = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 2, 2, 0, sw, 0, sa);
  }
}

template <int OUT_, bool W4>
struct Mx6Policy {
  static constexpr int OUT = OUT_, TKE = TKX, KMUL = TKX, WROW = W4 ? W4ROW : W6ROW, XROW = W6ROW;
  static constexpr bool SCALED = false, TOKEN = false;
  using Side = MxScales;

  static __device__ __forceinline__ void mma6(v4f (&acc)[4][4], const v4i (&wb)[4], const v2i (&w6)[3][4], const v2i (&x6)[3][4],
                                              const Side& s) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma_mx6<W4>(wb[j], w6[0][j], w6[1][j], w6[2][j], x6[0][i], x6[1][i], x6[2][i], acc[i][j], s.sw_cur[j], s.sa_cur[i]);
  }
};

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
  const Gemm16Params p = gemm16_params(a, w, sa_u8, sw_u8, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  hipStream_t st = (hipStream_t)stream;
  return with_out_dtype(out_dtype, [&](auto o) {
    constexpr int OUT = decltype(o)::value;
    return w_fmt == WANQ_MX_E2M1 ? launch_tiles(gemm_tile_kernel<MxPolicy<OUT, true>>, p, st, what)
                                 : launch_tiles(gemm_tile_kernel<MxPolicy<OUT, false>>, p, st, what);
  });
}

extern "C" int wanq_gemm_mx4(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, void* out, int out_dtype,
                             const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N,
                             int K, void* stream) {
  const char* what = "wanq_gemm_mx4";
  WANQ_REQUIRE(a && w && out && sa_u8 && sw_u8, WANQ_E_ARG, "%s: a, w, sa_u8, sw_u8 and out must be non-NULL", what);
  if (const int rc = check_gemm16_shapes(what, TKX, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  WANQ_REQUIRE(aligned(sa_u8, 4) && aligned(sw_u8, 4), WANQ_E_ARG, "%s: sa_u8 and sw_u8 must be 4-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const Gemm16Params p = gemm16_params(a, w, sa_u8, sw_u8, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  hipStream_t st = (hipStream_t)stream;
  return with_out_dtype(out_dtype, [&](auto o) {
    return launch_tiles(gemm_tile_kernel<MxPolicy<decltype(o)::value, true, true>>, p, st, what);
  });
}

extern "C" int wanq_gemm_mx6(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, int w_fmt, void* out,
                             int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags,
                             int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_mx6";
  WANQ_REQUIRE(a && w && out && sa_u8 && sw_u8, WANQ_E_ARG, "%s: a, w, sa_u8, sw_u8 and out must be non-NULL", what);
  WANQ_REQUIRE(w_fmt == WANQ_MX_E2M3 || w_fmt == WANQ_MX_E2M1, WANQ_E_ARG, "%s: w_fmt=%d must be WANQ_MX_E2M3 or WANQ_MX_E2M1", what,
               w_fmt);
  if (const int rc = check_gemm16_shapes(what, TKX, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K))
    return rc;
  WANQ_REQUIRE(aligned(sa_u8, 4) && aligned(sw_u8, 4), WANQ_E_ARG, "%s: sa_u8 and sw_u8 must be 4-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const Gemm16Params p = gemm16_params(a, w, sa_u8, sw_u8, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K);
  hipStream_t st = (hipStream_t)stream;
  return with_out_dtype(out_dtype, [&](auto o) {
    constexpr int OUT = decltype(o)::value;
    return w_fmt == WANQ_MX_E2M1 ? launch_tiles(gemm_tile_kernel<Mx6Policy<OUT, true>>, p, st, what)
                                 : launch_tiles(gemm_tile_kernel<Mx6Policy<OUT, false>>, p, st, what);
  });
}
