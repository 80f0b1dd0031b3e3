// wanq_gemm_mx_mixed: the W4A4 MX GEMM with outlier channels.  Both operands are stored in one permuted channel order (include/wanq_hip.h:
// the mixed MX row format): the first n8 channels of every row are e4m3 bytes, the other K - n8 packed e2m1 nibbles, one E8M0 scale
// byte per block of 32 permuted channels on either side.
//   acc[m,n] = sum_b 2^(sa[m,b]-127) 2^(sw[n,b]-127) sum_{k in b} a[m,k] w[n,k],  b over all K / 32 permuted blocks
//   y = acc + bias;  GELU;  residual + y * gate;  one rounding to out   (epilogue16<.., false, false>: the MFMA applied every scale)
// v_mfma_scale_f32_16x16x128_f8f6f4 takes its operand formats per instruction, so ONE K loop runs n8 / 128 K-tiles with e4m3 on both
// sides (cbsz 0, blgp 0, the fp8 rate) and then (K - n8) / 128 K-tiles with e2m1 on both sides (cbsz 4, blgp 4, the fp4 rate) into the
// same 4 x 4 accumulators: no second accumulator set, no second launch, the epilogue of the other MX GEMMs.
//
// Structure: gemm16_common.h's -- 128 x 128 output tile, 4 waves 2 x 2, Frame, LDS-DMA, one barrier per K-tile -- as a kernel of its
// own; gemm_tile_kernel and its instantiations are untouched.  Two LDS buffers of 32 KiB, each sized for an e4m3 K-tile (token half
// at byte 0, weight half at byte 16384 in BOTH phases), 64 KiB, two workgroups per CU.
//
// Phase 8, K-tiles 0 .. n8 / 128 - 1.  Both halves are what gemm_mx.hip's e4m3 halves are: 128 rows of 128 B, four LDS-DMA instructions
// per wave and half (dma_sources with the row pitch P = n8 + (K - n8) / 2), the 16-B chunk index XORed with (row >> 1) & 7, fragments
// read at chunks fq and 4 + fq (frag_addr, kk = 0 and 1).  Banks: gemm_mx.hip "LDS image", i.e. gemm_fp8.hip's derivation, unchanged.
// Phase 4, the remaining K-tiles.  Both halves are what gemm_mx.hip's W4A4 halves are: 128 rows of 64 B, two LDS-DMA instructions per
// wave and half (dma_sources4 on the row base + n8 bytes, the same pitch P), w4_swz, one ds_read_b128 of chunk fq per fragment,
// registers 4-7 zero.  Banks: gemm_mx.hip "LDS image" and "W4A4", unchanged -- the half's offset in the buffer (0 and 16 KiB) and the
// wave's 64-row offset (4 KiB) are multiples of 256 B and leave the banks alone.
//
// The phase boundary.  Tile t is copied into buffer t & 1 whatever its phase: the DMA of the first e2m1 tile is issued behind the
// barrier of the last e4m3 tile, into the other buffer, and runs under that tile's reads and MFMAs like every other copy.  One
// barrier per K-tile, no tile is waited for with nothing to hide it, and the buffer a copy overwrites was last read before every
// wave passed the barrier (the argument of gemm16_common.h; an e2m1 tile overwrites the first 8 KiB of each half of an e4m3 one).
//
// Scale operands: MxScales (gemm_mx_common.h), indexed by the running tile number across both phases -- the scale rows are in
// permuted order, block b of a row is its byte b whatever the block's format, so the scale path is phase-blind.
//
// Summation order of element (m, n): K-tiles ascending in permuted order, inside an MFMA the hardware's own.  It depends on (K, n8)
// only -- not on M, on the row's place in the launch or on the workgroup.  No split-K, one kernel form.
#include "gemm_mx_common.h"

namespace wanq {
namespace {

constexpr int MIXED_TILE = 2 * XTILE;  // one K-tile buffer: token half, weight half, each 16 KiB (an e2m1 half uses its first 8)

template <int OUT>
__global__ void __launch_bounds__(256, 2) gemm_mx_mixed_kernel(const Gemm16Params p, const int n8) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * MIXED_TILE];
  const Frame f(p.nt);
  const int nt8 = n8 / TKX, nk = nt8 + (p.K - n8) / TKX;
  const int pitch = n8 + (p.K - n8) / 2;  // bytes of a stored row, tokens and weights alike

  // ---- LDS-DMA sources: the e4m3 segment as 128-B rows, the e2m1 segment (n8 bytes into the row) as 64-B rows
  const char *xs8[4], *ws8[4], *xs4[4], *ws4[4];
  dma_sources(p.a, f.m0, p.M, pitch, f, xs8);
  dma_sources(p.w, f.n0, p.N, pitch, f, ws8);
  dma_sources4(static_cast<const char*>(p.a) + n8, f.m0, p.M, pitch, f, xs4);
  dma_sources4(static_cast<const char*>(p.w) + n8, f.n0, p.N, pitch, f, ws4);
  auto issue = [&](int t) {
    char* dst = smem + (t & 1) * MIXED_TILE + f.wave * 1024;
    if (t < nt8) {
      dma_issue<4>(xs8, (int64_t)t * TROW, dst);
      dma_issue<4>(ws8, (int64_t)t * TROW, dst + XTILE);
    } else {
      dma_issue<2>(xs4, (int64_t)(t - nt8) * W4ROW, dst);
      dma_issue<2>(ws4, (int64_t)(t - nt8) * W4ROW, dst + XTILE);
    }
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const uint32_t rd0 = frag_addr(lds0, f.fr, f.fq, 0), rd1 = frag_addr(lds0, f.fr, f.fq, 1);
  const uint32_t rdw4 = lds0 + f.fr * W4ROW + ((f.fq ^ w4_swz(f.fr)) << 4);
  MxScales side(p, f);

  v4f acc[4][4];
  zero_acc(acc);

  // wait for this wave's DMA of tile t | barrier | issue the DMA of tile t + 1, of either phase, into the other buffer
  auto step = [&](int t) {
    side.shift();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) {
      issue(t + 1);
      side.load(t + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  issue(0);
  side.load(0);
  int t = 0;
  for (; t < nt8; ++t) {  // ---- phase 8: e4m3 x e4m3
    step(t);
    const uint32_t xo = (t & 1) * MIXED_TILE + f.wm * 64 * TROW, wo = (t & 1) * MIXED_TILE + XTILE + f.wn * 64 * TROW;
    v4i xa[2][4], wb[2][4];
    dsr4<TROW>(wb[0], rd0 + wo);
    dsr4<TROW>(xa[0], rd0 + xo);
    dsr4<TROW>(wb[1], rd1 + wo);
    dsr4<TROW>(xa[1], rd1 + xo);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma_mx<false, false>(wb[0][j], wb[1][j], xa[0][i], xa[1][i], acc[i][j], side.sw_cur[j], side.sa_cur[i]);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (; t < nk; ++t) {  // ---- phase 4: e2m1 x e2m1
    step(t);
    const uint32_t xo = (t & 1) * MIXED_TILE + f.wm * 64 * W4ROW, wo = (t & 1) * MIXED_TILE + XTILE + f.wn * 64 * W4ROW;
    v4i xa[4], wb[4];
    dsr4<W4ROW>(wb, rdw4 + wo);
    dsr4<W4ROW>(xa, rdw4 + xo);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = mfma_mx<true, true>(wb[j], wb[j], xa[i], xa[i], acc[i][j], side.sw_cur[j], side.sa_cur[i]);
    __builtin_amdgcn_sched_barrier(0);
  }

  epilogue16<OUT, false, false>(acc, f, p);
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_gemm_mx_mixed(const uint8_t* a, const uint8_t* w, const uint8_t* sa_u8, const uint8_t* sw_u8, int n8, void* out,
                                  int out_dtype, const void* bias, int bias_dtype, const float* gate, const void* residual,
                                  int epi_flags, int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_mx_mixed";
  const auto rules = [&](MxRulesAt at) {
    if (at == MX_AFTER_SHAPES)
      WANQ_REQUIRE(n8 >= TKX && n8 % TKX == 0 && K - n8 >= TKX, WANQ_E_SHAPE,
                   "%s: n8=%d must be a multiple of 128 with 128 <= n8 <= K - 128 (K=%d)", what, n8, K);
    return WANQ_OK;
  };
  return mx_gemm_entry(what, a, w, sa_u8, sw_u8, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N, K, stream, rules,
                       [&](const Gemm16Params& p, hipStream_t st) {
                         return with_out_dtype(out_dtype, [&](auto o) {
                           const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
                           hipLaunchKernelGGL(gemm_mx_mixed_kernel<decltype(o)::value>, dim3((unsigned)tiles), dim3(256), 0, st, p, n8);
                           return check_launch(what);
                         });
                       });
}
