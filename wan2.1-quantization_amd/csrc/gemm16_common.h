// What the four tile GEMMs outside the int8 family share.  gemm_bf16.hip (bf16 / fp16 operands), gemm_fp8.hip (e4m3, fp32 row and
// channel scales) and gemm_mx.hip (OCP MX: e4m3 tokens against e4m3 or packed e2m1 weights, E8M0 block scales) copy BOTH halves of
// a K-tile into LDS and are one kernel, gemm_tile_kernel below, with a policy each (gemm_mx.hip's W4A4 form, packed e2m1 on both
// sides, and its W6A6 / W4A6 forms, packed e2m3 tokens, are further policies of it); gemm_wq16.hip (integer weight codes converted
// in registers, plain and group-wise) copies the token half only and has its own loop.  All four use the tile geometry, Frame, the
// LDS-DMA sources and issue, the fragment addresses and reads, epilogue16, the launch parameters and helpers and the argument rules
// of the extern "C" entries; gemm_tile_kernel is used by the first three.
//
// Structure.  One 128(M) x 128(N) output tile per 256-thread workgroup (4 waves, 2 x 2, 64 x 64 each = 4 x 4 MFMA tiles).  A K-tile
// is 128 bytes of every row: 64 16-bit or 128 8-bit elements (64 bytes of a packed e2m1 weight row).  A half of a K-tile (128 rows
// of 128 B) is copied global -> LDS by LDS-DMA (global_load_lds_dwordx4, 4 per wave) into one of two buffers; rows are 128 B with
// the 16-B chunk index XORed with (row >> 1) & 7, on the DMA source address and on the fragment reads (the LDS image of
// gemm_w8a8_pp.hip: a 16x16x32 bf16 fragment takes the same 16 bytes per lane as a 16x16x64 int8 one).  The MFMA takes the WEIGHT
// fragment as its A operand and the token fragment as B, so a lane's four accumulators are four consecutive channels of one token:
// bias / gate loads and the stores are 4-wide vectors.
//
// The two-sided loop (gemm_tile_kernel).  Token rows 0-127 and weight rows 128-255 of a K-tile share one buffer (32 KiB; 24 KiB with
// e2m1 weights, 16 KiB with e2m1 tokens too), two buffers, one barrier per K-tile:
//   wait for this wave's DMA of tile t | barrier | issue the DMA of tile t+1 into the other buffer | 16 fragment reads of tile t
//   | the policy's MFMA block
// so the copy of tile t+1 runs under the reads and MFMAs of tile t, and the buffer it overwrites was last read before every wave
// passed the barrier.  64 KiB (48 KiB) of LDS: two workgroups per CU, whose bursts interleave on the SIMDs.  A policy supplies
//   OUT, SCALED, TOKEN   the epilogue16 instantiation
//   TKE, KMUL            elements of a K-tile and the entry's K multiple; when KMUL is half of TKE a last tile may be half deep: its
//                        second 16-byte step is then read from the first step's addresses and `half` tells the MFMA block
//   WROW                 bytes of a weight row per K-tile: TROW, W4ROW for gemm_mx.hip's packed e2m1 rows (their own swizzle), or
//                        W6ROW (96 B) for its packed e2m3 rows: three DMA instructions per wave, w6_swz, three ds_read_b64 per
//                        fragment, and mma6 in place of mma (gemm_mx.hip has the derivation)
//   XROW                 bytes of a token row per K-tile, likewise: W4ROW (with WROW == W4ROW only) for gemm_mx.hip's e2m1 tokens, whose
//                        half is then the same 128 rows of 64 B, the same two DMA instructions per wave and the same swizzle and
//                        one-chunk fragment read as the packed weight half; W6ROW (with WROW == W6ROW or W4ROW) for its e2m3 tokens
//   Side                 per-tile values a lane loads itself, one tile ahead behind the DMA (gemm_mx.hip's scale dwords), or NoSide
//   mma                  the MFMA block of one K-tile
//
// Determinism.  Every output element is summed by one lane, over k in K-tile order and within a tile in the instruction's own
// order (16-bit: two 32-deep MFMA steps with the same k -> fragment-slot assignment in both 16-bit files): its fp32 summation order
// depends on K only -- not on M, on the row's place in the launch or on which workgroup ran it.  No split-K, one kernel form each.
// Rows past M are read from row M - 1 (computed, never stored); channels past N likewise.
#pragma once
#include <type_traits>

#include "gemm_params.h"

namespace wanq {
namespace {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

constexpr int TM = 128, TN = 128, TK = 64;
constexpr int TROW = TK * 2;      // bytes of one LDS row
constexpr int XTILE = TM * TROW;  // a half of a K-tile buffer (128 rows): 16 KiB
constexpr int W4ROW = TROW / 2;   // bytes of a packed e2m1 weight row of a K-tile
constexpr int W6ROW = 96;         // bytes of a packed e2m3 row of a K-tile: four blocks of 32 six-bit codes (gemm_mx.hip)

// launch parameters of all four files; sa / sw: fp32 (gemm_fp8.hip, and sw of gemm_wq16.hip), E8M0 bytes (gemm_mx.hip) or null
struct Gemm16Params {
  const void* a;
  const void* w;
  const void* sa;
  const void* sw;
  void* out;
  const void* bias;
  const float* gate;
  const void* residual;
  int bias_dtype, epi;
  int M, N, K, nt;
};

// this thread's place: its wave's 64 x 64 quarter (wm, wn) of the workgroup's tile at (m0, n0), its fragment row fr and lane group fq
struct Frame {
  int lane, wave, wm, wn, m0, n0, fr, fq;
  __device__ __forceinline__ explicit Frame(int nt) {
    const int tid = threadIdx.x, tm = blockIdx.x / nt, tn = blockIdx.x - tm * nt;
    lane = tid & 63; wave = tid >> 6; wm = wave >> 1; wn = wave & 1;
    m0 = tm * TM; n0 = tn * TN; fr = lane & 15; fq = lane >> 4;
  }
};

template <int OFF>
__device__ __forceinline__ void dsr(v4i& d, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

// one fragment of each of a wave's four 16-row blocks, ROW bytes per LDS row
template <int ROW>
__device__ __forceinline__ void dsr4(v4i (&d)[4], uint32_t addr) {
  dsr<0>(d[0], addr); dsr<16 * ROW>(d[1], addr); dsr<32 * ROW>(d[2], addr); dsr<48 * ROW>(d[3], addr);
}

// packed e2m3 rows (W6ROW): one 8-byte piece of a fragment (gemm_mx.hip: a 24-byte block is three of them, 8-byte aligned only)
template <int OFF>
__device__ __forceinline__ void dsr64(v2i& d, uint32_t addr) {
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

// piece p of the e2m3 fragment of each of a wave's four 16-row blocks, addr[p] as frag6_addr gives it
__device__ __forceinline__ void dsr4x6(v2i (&d)[3][4], const uint32_t (&addr)[3], uint32_t off) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    dsr64<0>(d[p][0], addr[p] + off); dsr64<16 * W6ROW>(d[p][1], addr[p] + off);
    dsr64<32 * W6ROW>(d[p][2], addr[p] + off); dsr64<48 * W6ROW>(d[p][3], addr[p] + off);
  }
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

// LDS-DMA sources of a half of 128 rows x 128 B (tokens, or weights): instruction q (0-3) of this wave fills LDS rows 8 g .. 8 g + 7,
// g = 4 q + wave; lane l writes row 8 g + (l >> 3), physical chunk l & 7 = logical chunk c ^ ((row >> 1) & 7).  src[q] points at
// byte 0 of that chunk in row row0 + r of `base` (`pitch` bytes per row; rows past `rows` read row rows - 1).  Returns c, the
// same for all four instructions (8 g is a multiple of 16 / 2).
__device__ __forceinline__ int dma_sources(const void* base, int row0, int rows, int64_t pitch, const Frame& f,
                                           const char* (&src)[4]) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + f.wave) + (f.lane >> 3);
    c = (f.lane & 7) ^ ((r >> 1) & 7);
    const int row = row0 + r < rows ? row0 + r : rows - 1;
    src[q] = static_cast<const char*>(base) + row * pitch + c * 16;
  }
  return c;
}

// NQ LDS-DMA instructions of this wave, 16 B per lane: 1 KiB each, 4 KiB apart (one per wave in between)
template <int NQ>
__device__ __forceinline__ void dma_issue(const char* const (&src)[4], int64_t off, char* dst) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) __builtin_amdgcn_global_load_lds((glb_void*)(src[q] + off), (lds_void*)(dst + q * 4096), 16, 0, 0);
}

// fragment reads: lane l reads row (16-row block) + fr, fr = l & 15, logical chunk 4 kk + fq, fq = l >> 4, of the 32-deep step kk
__device__ __forceinline__ uint32_t frag_addr(uint32_t lds0, int fr, int fq, int kk) {
  return lds0 + fr * TROW + (((4 * kk + fq) ^ ((fr >> 1) & 7)) << 4);
}

// acc[token block i][channel block j]: channel (lane >> 4) * 4 + e, token lane & 15
__device__ __forceinline__ void zero_acc(v4f (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
}

// epilogue, fp32: acc + bias, or with SCALED acc * sw + bias in one fma, or with TOKEN (gemm_fp8.hip) (acc * sa[m]) * sw + bias, the
// per-token factor first and then one fma; with LOWRANK (gemm_wq16.hip) + lr, a second accumulator set, one fp32 add behind the bias;
// GELU; residual + y * gate; one rounding to OUT
template <int OUT, bool SCALED, bool TOKEN, bool LOWRANK>
__device__ __forceinline__ void epilogue16(const v4f (&acc)[4][4], const v4f (&lr)[4][4], const Frame& f, const Gemm16Params& p) {
  static_assert(!TOKEN || SCALED, "the per-token factor comes with the per-channel one");
  const bool gelu = p.epi & WANQ_EPI_GELU, gres = p.epi & WANQ_EPI_GATE_RES;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = f.n0 + f.wn * 64 + j * 16 + f.fq * 4;
    if (n >= p.N) continue;
    float s4[4], b4[4] = {0.f, 0.f, 0.f, 0.f}, g4[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SCALED) load4_ch(p.sw, WANQ_F32, n, s4);
    if (p.bias) load4_any(p.bias, p.bias_dtype, n, b4);
    if (gres) load4_ch(p.gate, WANQ_F32, n, g4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = f.m0 + f.wm * 64 + i * 16 + f.fr;
      if (m >= p.M) continue;
      const int64_t o = (int64_t)m * p.N + n;
      float y[4];
      float sm = 1.f;
      if constexpr (TOKEN) sm = static_cast<const float*>(p.sa)[m];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (TOKEN) y[e] = __fmaf_rn(acc[i][j][e] * sm, s4[e], b4[e]);
        else if constexpr (SCALED) y[e] = __fmaf_rn(acc[i][j][e], s4[e], b4[e]);
        else y[e] = acc[i][j][e] + b4[e];
        if constexpr (LOWRANK) y[e] += lr[i][j][e];
      }
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

template <int OUT, bool SCALED, bool TOKEN = false>
__device__ __forceinline__ void epilogue16(const v4f (&acc)[4][4], const Frame& f, const Gemm16Params& p) {
  epilogue16<OUT, SCALED, TOKEN, false>(acc, acc, f, p);
}

// ---- the two-sided loop: policies in gemm_bf16.hip, gemm_fp8.hip and gemm_mx.hip (header comment: what a policy supplies) -----
struct NoSide {
  __device__ __forceinline__ NoSide(const Gemm16Params&, const Frame&) {}
  __device__ __forceinline__ void load(int) {}
  __device__ __forceinline__ void shift() {}
};

// packed e2m1 rows (64 B, four to a 256-B bank line): logical chunk c at physical chunk c ^ w4_swz(row); gemm_mx.hip
__device__ __forceinline__ int w4_swz(int r) {
  const int u = (r >> 2) & 3;
  return u ^ ((u & 1) << 1);
}

// LDS-DMA sources of a half of 128 packed e2m1 rows x 64 B: instruction q (0-1) of this wave fills rows 16 g .. 16 g + 15, g = 4 q +
// wave, lane l row 16 g + (l >> 2), physical chunk l & 3.  `pitch` bytes per row of `base`; rows past `rows` read row rows - 1.
__device__ __forceinline__ void dma_sources4(const void* base, int row0, int rows, int pitch, const Frame& f, const char* (&src)[4]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = 16 * (4 * q + f.wave) + (f.lane >> 2);
    const int c = (f.lane & 3) ^ w4_swz(r);
    const int row = row0 + r < rows ? row0 + r : rows - 1;
    src[q] = static_cast<const char*>(base) + (int64_t)row * pitch + c * 16;
  }
}

// packed e2m3 rows (96 B, the third geometry; gemm_mx.hip has the bank derivation): LDS 16-byte chunk g of a half is row g / 6,
// physical chunk g % 6 = logical chunk c ^ w6_swz(row).  c ^ 1 stays inside the row's six chunks.
__device__ __forceinline__ int w6_swz(int r) { return (r >> 3) & 1; }

// LDS-DMA sources of a half of 128 packed e2m3 rows x 96 B = 768 chunks: instruction q (0-2) of this wave fills chunks 64 g .. 64 g +
// 63, g = 4 q + wave, lane l chunk 64 g + l.  `pitch` bytes per row of `base`; rows past `rows` read row rows - 1.
__device__ __forceinline__ void dma_sources6(const void* base, int row0, int rows, int64_t pitch, const Frame& f, const char* (&src)[4]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int g = 64 * (4 * q + f.wave) + f.lane, r = g / 6;
    const int c = (g - 6 * r) ^ w6_swz(r);
    const int row = row0 + r < rows ? row0 + r : rows - 1;
    src[q] = static_cast<const char*>(base) + row * pitch + c * 16;
  }
}

// an e2m3 fragment: the 24 bytes of block fq of row fr, as the 8-byte pieces p = 0, 1, 2: bytes 8 (3 fq + p) of the row, i.e. half
// (3 fq + p) & 1 of logical chunk (3 fq + p) >> 1
__device__ __forceinline__ uint32_t frag6_addr(uint32_t lds0, int fr, int fq, int p) {
  const int s = 3 * fq + p;
  return lds0 + fr * W6ROW + (((s >> 1) ^ w6_swz(fr)) << 4) + ((s & 1) << 3);
}

template <class P>
__global__ void __launch_bounds__(256, 2) gemm_tile_kernel(Gemm16Params p) {
  constexpr bool W4 = P::WROW == W4ROW, X4 = P::XROW == W4ROW, W6 = P::WROW == W6ROW, X6 = P::XROW == W6ROW, SHORT = P::KMUL < P::TKE;
  constexpr int XT = TM * P::XROW, TILE = XT + TN * P::WROW;  // one K-tile buffer: token rows, then weight rows
  static_assert((W4 || W6 || P::WROW == TROW) && (X4 ? W4 : X6 ? (W4 || W6) : (P::XROW == TROW && !W6)) &&
                    (P::KMUL == P::TKE || (P::KMUL * 2 == P::TKE && !W4 && !W6)),
                "no such geometry");
  __shared__ __attribute__((aligned(1024))) char smem[2 * TILE];
  const Frame f(p.nt);
  const int K = p.K, nk = (K + P::TKE - P::KMUL) / P::TKE;  // K % KMUL == 0

  // ---- LDS-DMA sources: 128-B token and weight rows as dma_sources has them, packed e2m1 rows as dma_sources4
  const char *src[4], *wsrc[4];
  int kc = 0;  // (the token half's logical chunk: what a half-deep last tile asks about)
  if constexpr (X6) dma_sources6(p.a, f.m0, p.M, (int64_t)K * W6ROW / P::TKE, f, src);
  else if constexpr (X4) dma_sources4(p.a, f.m0, p.M, K / 2, f, src);
  else kc = dma_sources(p.a, f.m0, p.M, (int64_t)K * TROW / P::TKE, f, src);
  if constexpr (W6) {
    dma_sources6(p.w, f.n0, p.N, (int64_t)K * W6ROW / P::TKE, f, wsrc);
  } else if constexpr (W4 && !X4 && !X6) {  // (dma_sources4 written out: the form the W4A8 kernels were built and measured with)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = 16 * (4 * q + f.wave) + (f.lane >> 2);
      const int c = (f.lane & 3) ^ w4_swz(r);
      const int n = f.n0 + r < p.N ? f.n0 + r : p.N - 1;
      wsrc[q] = static_cast<const char*>(p.w) + (int64_t)n * (K / 2) + c * 16;
    }
  } else if constexpr (W4) {
    dma_sources4(p.w, f.n0, p.N, K / 2, f, wsrc);
  } else {
    dma_sources(p.w, f.n0, p.N, (int64_t)K * TROW / P::TKE, f, wsrc);
  }
  auto issue = [&](int t) {
    // the source offset in half rows of a K-tile.  k past K only in the second half of a half-deep last tile: re-read the first
    // half (never multiplied)
    int h = 2 * t;
    if constexpr (SHORT) h = t * P::TKE + kc * (P::TKE / 8) < K ? 2 * t : 2 * t - 1;
    char* dst = smem + (t & 1) * TILE + f.wave * 1024;
    dma_issue<XT / 4096>(src, (int64_t)h * (P::XROW / 2), dst);
    dma_issue<TN * P::WROW / 4096>(wsrc, (int64_t)h * (P::WROW / 2), dst + XT);
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const uint32_t rd0 = frag_addr(lds0, f.fr, f.fq, 0), rd1 = frag_addr(lds0, f.fr, f.fq, 1);
  const uint32_t rdw4 = lds0 + f.fr * W4ROW + ((f.fq ^ w4_swz(f.fr)) << 4);  // an e2m1 fragment: the one chunk fq of its row
  uint32_t rd6[3] = {0, 0, 0};  // an e2m3 fragment: three 8-byte pieces of block fq of its row
  if constexpr (W6 || X6) {
#pragma unroll
    for (int q = 0; q < 3; ++q) rd6[q] = frag6_addr(lds0, f.fr, f.fq, q);
  }
  typename P::Side side(p, f);

  v4f acc[4][4];
  zero_acc(acc);

  issue(0);
  side.load(0);
  for (int t = 0; t < nk; ++t) {
    side.shift();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) {
      issue(t + 1);
      side.load(t + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t xo = (t & 1) * TILE + f.wm * 64 * P::XROW, wo = (t & 1) * TILE + XT + f.wn * 64 * P::WROW;
    v4i xa[2][4], wb[2][4];  // [16-byte step][16-row block]; an e2m1 fragment is wb[0] / xa[0] alone
    if constexpr (W6 || X6) {
      v2i x6[3][4], w6[3][4];  // [8-byte piece][16-row block] of an e2m3 fragment
      if constexpr (W6) dsr4x6(w6, rd6, wo);
      else dsr4<W4ROW>(wb[0], rdw4 + wo);
      dsr4x6(x6, rd6, xo);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      P::mma6(acc, wb[0], w6, x6, side);
    } else {
      if constexpr (W4) dsr4<W4ROW>(wb[0], rdw4 + wo);
      else dsr4<TROW>(wb[0], rd0 + wo);
      if constexpr (X4) dsr4<W4ROW>(xa[0], rdw4 + xo);
      else dsr4<TROW>(xa[0], rd0 + xo);
      if constexpr (!W4) dsr4<TROW>(wb[1], rd1 + wo);
      if constexpr (!X4) dsr4<TROW>(xa[1], rd1 + xo);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      P::mma(acc, wb, xa, side, SHORT && t * P::TKE + P::KMUL >= K);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  epilogue16<P::OUT, P::SCALED, P::TOKEN>(acc, f, p);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
inline Gemm16Params gemm16_params(const void* a, const void* w, const void* sa, const void* sw, void* out, const void* bias,
                                  int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K) {
  const bool gres = epi_flags & WANQ_EPI_GATE_RES;
  return Gemm16Params{a, w, sa, sw, out, bias, gres ? gate : nullptr, gres ? residual : nullptr, bias_dtype, epi_flags,
                      (int)M, N, K, (N + TN - 1) / TN};
}

// one workgroup per output tile; KP: Gemm16Params, or a struct derived from it (gemm_wq16.hip)
template <class KP>
int launch_tiles(void (*kernel)(KP), const KP& p, hipStream_t st, const char* what) {
  const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * p.nt;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), 0, st, p);
  return check_launch(what);
}

// f(std::integral_constant<int, OUT>) for the output dtype (checked by check_gemm16_shapes)
template <class F>
int with_out_dtype(int out_dtype, F&& f) {
  switch (out_dtype) {
    case WANQ_F16: return f(std::integral_constant<int, WANQ_F16>{});
    case WANQ_BF16: return f(std::integral_constant<int, WANQ_BF16>{});
    default: return f(std::integral_constant<int, WANQ_F32>{});
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The argument rules both entries share, in the order they are refused, in two parts: an entry checks its non-NULL operands and the
// operand dtype itself, calls check_gemm16_shapes, and after any alignment rule of its own check_gemm16_tail.  `kmul`: the entry's
// K multiple.
inline int check_gemm16_shapes(const char* what, int kmul, const void* a, const void* w, const void* out, int out_dtype,
                               const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags, int64_t M,
                               int N, int K) {
  WANQ_REQUIRE(is_fp(out_dtype), WANQ_E_ARG, "%s: out dtype %d must be BF16, F16 or F32", what, out_dtype);
  WANQ_REQUIRE(!bias || is_fp(bias_dtype), WANQ_E_ARG, "%s: bias dtype %d must be BF16, F16 or F32", what, bias_dtype);
  WANQ_REQUIRE((epi_flags & ~(WANQ_EPI_GELU | WANQ_EPI_GATE_RES)) == 0, WANQ_E_ARG, "%s: unknown epilogue flag", what);
  WANQ_REQUIRE(!(epi_flags & WANQ_EPI_GATE_RES) || (gate && residual), WANQ_E_ARG, "%s: WANQ_EPI_GATE_RES needs gate and residual",
               what);
  WANQ_REQUIRE(M >= 0 && M < (1ll << 31) - TM, WANQ_E_SHAPE, "%s: M=%lld out of range", what, (long long)M);
  WANQ_REQUIRE(N >= 8 && N % 8 == 0, WANQ_E_SHAPE, "%s: N=%d must be a positive multiple of 8", what, N);
  WANQ_REQUIRE(K >= kmul && K % kmul == 0, WANQ_E_SHAPE, "%s: K=%d must be a positive multiple of %d", what, K, kmul);
  WANQ_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(out, 16) && aligned(residual, 16), WANQ_E_ARG,
               "%s: a, w, out and residual must be 16-byte aligned", what);
  return WANQ_OK;
}

// (the tile-count limit stands before the entries' M == 0 return here; no tiles pass it)
inline int check_gemm16_tail(const char* what, const void* bias, int bias_dtype, const float* gate, int64_t M, int N) {
  WANQ_REQUIRE(aligned(gate, 16) && (!bias || aligned(bias, bias_dtype == WANQ_F32 ? 16 : 8)), WANQ_E_ARG,
               "%s: gate and bias must be aligned to 4 elements", what);
  WANQ_REQUIRE(((M + TM - 1) / TM) * (((int64_t)N + TN - 1) / TN) < (1ll << 31), WANQ_E_SHAPE, "%s: too many tiles", what);
  return WANQ_OK;
}

}  // namespace
}  // namespace wanq
