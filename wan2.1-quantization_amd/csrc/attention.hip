// Flash-attention forward for gfx950, head_dim 128, non-causal, key-length masking, optional sliding window.
//
//   O[q, h, :] = softmax_k( Q[q,h,:] . K[k,h,:] / sqrt(d) ) V[k,h,:]
//
// One kernel template, attn_fwd16_kernel<SPLIT, QK8, NW, F16, WIN>, for every form: 16-bit or int8 Q.K^T (QK8), whole key range or
// one share of it (SPLIT, merged by attn_combine_kernel), 8 or 4 waves per workgroup (NW, plain 16-bit form only), bf16 or fp16
// elements (F16: the MFMA instruction, the conversions and the exponent headroom of P differ, see at_elem; the text below says bf16),
// all keys or a band of them per query (WIN, plain 16-bit form only).
//
// WIN (sliding-window local attention, wanq_attention_window_fwd; the `window_size=(left, right)` the reference's WanSelfAttention
// hands to flash_attn, ViDiT-Q/examples/Wan2.1/wan/modules/model.py:110-169).  flash_attn is not part of the reference tree, so
// the semantics are stated here, with Lk the number of valid keys (after k_len) and off = Lk - Lq:
//   * query i sees key j iff  i + off - left <= j <= i + off + right  and  0 <= j < Lk  (flash_attn's bottom-right alignment);
//   * a negative left or right means unbounded on that side;
//   * a query that sees no key gets an output row of exact zeros;
//   * the window runs over the flattened token sequence ((f, h, w) row-major in the model) and belongs to self-attention only:
//     cross-attention never gets one, as in the reference.
// A workgroup walks only the key tiles [jt0, jt1) that some query of its block sees (the mechanism of a split-KV share); a wave
// masks element-wise the tiles its 32 queries see partly, leaves the ones they all see whole untouched and skips the math of the
// ones none of them sees (it still issues its LDS-DMA pieces and meets every barrier).  A row's softmax reference is fixed by the
// first tile in which the ROW sees a key, not by the workgroup's first tile (see the softmax block).
//
// Layout: Q/K/V/O are token-major [tokens, heads*128] bf16 or fp16 (exactly what the q/k/v GEMMs write and what the
// o-projection's quantiser reads), so no head transposes exist anywhere.
//
// Structure: every wave owns 32 queries of one head for the whole kernel and holds their Q fragments in registers.  Per
// 64-key tile:
//   S^T = K . Q^T      A operand = K rows from LDS (ds_read_b128), B operand = Q in registers, on v_mfma_f32_16x16x32_bf16
//                      (QK8: v_mfma_i32_16x16x64_i8);
//   O^T += V^T . P^T   B operand = the S^T accumulators themselves, converted to bf16 in place (the accumulators' register ->
//                      key permutation is matched by the order in which the A operand V^T is gathered with
//                      ds_read_b64_tr_b16), so P never touches LDS.
// The 16x16 MFMA shapes hold a ~10 % higher clock on this part than the 32x32 ones (tools/probes/mfma_shape_clock.hip), and the
// softmax's exponentials fit one per MFMA.
//
// K and V tiles travel global -> LDS by LDS-DMA (global_load_lds_dwordx4) into a ring of three stages (two in the 4-wave
// form), two tiles (one) ahead of the math, published by a counted s_waitcnt vmcnt(N) (N = the LDS-DMA instructions this wave
// issued for the tiles still allowed in flight) + one bare s_barrier per tile.  V rows are 256 B with the 16-B chunk index
// XORed by ((row&3)<<2 | (row>>2)&3) (at_off): conflict-free for the transposed reads; the bf16 K image XORs by row & 15,
// conflict-free for the b128 lane groups of the K operand; the int8 K image has 128-B rows XORed by (row>>1)&7 (at_off8).  The
// DMA writes lane-linearly, so it applies the swizzle on the source side.
//
// QK8 (int8 Q.K^T, the reference's q / k fake-quant recipe run on the integer matrix cores: Q/base/quant_attn.py:168-174,
// W/models/quant_opensora.py:431-436): q and k arrive as per-(token, head) symmetric int8 codes with fp32 scales.  The int32
// accumulators of v_mfma_i32_16x16x64_i8 START at 0x4B400000, the bit pattern of 12582912.0f = 1.5 * 2^23: |dot| <= 128 * 127 *
// 127 < 2^22, so the accumulator's bits READ AS A FLOAT are exactly 12582912 + dot -- no int->float conversion -- and one fma per
// score, t = fma(f, delta_k, -12582912 * delta_k), applies the per-key scale (the constant comes precomputed beside the scale).
// The per-query scale delta_q is folded into the exp2 coefficient.  The K tile is 8 KiB instead of 16; P.V stays bf16.
#include "wanq_common.h"
#include <stdlib.h>

namespace wanq {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AttnParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  uint16_t* o;
  int64_t q_stride, k_stride, v_stride, o_stride;  // elements between consecutive tokens
  int Lq, Lk, H;
  float c;  // softmax scale * log2(e)
  // split-KV (gridDim.z > 1): workgroup z covers key tiles [z*tiles_per_split, ...) and writes unnormalised partials
  // sliding window (WIN; excludes split-KV, whose share size it shares a word with, and fills what was padding -- the layout
  // the other instantiations read is unchanged): query i sees keys [i + win_lo, i + win_hi] (and < Lk); the host clamps both so
  // that no 32-bit sum overflows
  union {
    int tiles_per_split;
    int win_hi;
  };
  int win_lo;
  float* part_o;   // [splits, Lq, H*128] fp32: O^T accumulators relative to the split's reference maximum
  float* part_ml;  // [splits, Lq, H, 2]  fp32: (reference maximum m, row sum l)
  // int8 Q.K^T (QK8): per-(token, head) symmetric int8 codes [tokens, H*128] and fp32 scale planes [H][stride]
  const int8_t* q8;
  const int8_t* k8;
  int64_t q8_stride, k8_stride;   // bytes between consecutive tokens
  const float* q_scale;           // delta_q[h][token]
  const float* k_scale;           // delta_k[h][token], followed by the plane -12582912 * delta_k at + H * ks_stride
  int64_t qs_stride, ks_stride;
};

constexpr int AT_D = 128, AT_QW = 32, AT_NW = 8, AT_QB = AT_QW * AT_NW, AT_KB = 64;
constexpr int AT_TILE = AT_KB * AT_D * 2;  // 16 KiB per K or V tile
constexpr int AT_STAGE = 2 * AT_TILE;
// QK8 stage: int8 K tile (64 x 128 B) | bf16 V tile | 64 key scales | 64 dequantisation constants
constexpr int AT_K8 = AT_KB * AT_D;               // 8 KiB
constexpr int AT_SC8 = AT_K8 + AT_TILE;           // scales at 24 KiB
constexpr int AT_STAGE8 = AT_SC8 + 2 * AT_KB * 4;  // 25088 B

__device__ __forceinline__ int at_off8(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ int at_off(int row, int ch) {
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

// The 16-bit element type of Q / K / V / P / O: bf16, or fp16 (F16).  The LDS images, the LDS-DMA and the transposed reads move
// 16-bit elements whatever they mean; the type shows in the MFMA instruction, in the conversions (hipcc emits round-to-nearest-even
// v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 or v_cvt_f16_f32 for the casts below, never the round-toward-zero cvt_pkrtz) and in the exponent
// headroom AT_F16_HEADROOM of P.
template <bool F16> struct at_elem { typedef __bf16 e; typedef bf16x8 x8; typedef __bf16 x4 __attribute__((ext_vector_type(4))); };
template <> struct at_elem<true> { typedef _Float16 e; typedef f16x8 x8; typedef _Float16 x4 __attribute__((ext_vector_type(4))); };

template <typename X8> __device__ __forceinline__ X8 at_join(s16x4 lo, s16x4 hi) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 vv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(X8, vv);
}

__device__ __forceinline__ f32x4 at_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 at_mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// fp16 P: P' = exp2(s - reference + 8).  bf16 keeps its 8 bits down to 2^-126; fp16 leaves its normal range at 2^-14, so the
// fp16 forms lift P by 2^8: the largest P of a row lies in [2^8, 2^14] (lazy reference) and a key keeps all 11 bits down to 22
// log2 units below the row maximum.  The factor runs through the row sum too and cancels in O / l.
constexpr float AT_F16_HEADROOM = 8.0f;

#ifndef WANQ_ATTN_NW4_KEYS_DEFAULT  // key count up to which the plain bf16 kernel runs in its 4-wave form
#define WANQ_ATTN_NW4_KEYS_DEFAULT 1024
#endif

// =====================================================================================================================
// MFMA fragments.  Per wave 32 queries = two blocks nq of 16; per 64-key tile four key blocks kb of 16.
//   S^T block (kb, nq) = K_kb . Q_nq^T : A = K rows (ds_read_b128: lane (r = lane & 15, g = lane >> 4) reads LDS row
//       16 kb + kappa(r), 16-B chunk 4 s + g of d-slice s), B = Q fragment in registers.  Accumulator element e of lane
//       (n, g) is query 16 nq + n against key 16 kb + 4 pi(g) + e, where kappa(4 t + e) = 4 pi(t) + e, pi = (0, 2, 1, 3):
//       the swap of the two middle row quads makes the transposed V reads below conflict-free.
//   O^T block (db, nq) += V^T_(db) . P^T_nq : B = two S blocks (2 ks, 2 ks + 1) of the lane converted in place (k index
//       8 g + j <-> key 32 ks + 16 (j >> 2) + 4 pi(g) + (j & 3)); A = V^T gathered by two ds_read_b64_tr_b16 whose 16-lane
//       group g reads rows 32 ks + 16 jh + 4 pi(g) + q: the two groups of a 32-lane half sit 8 rows apart (conflict-free).
//   A query's statistics live in four lanes (n, n + 16, n + 32, n + 48): the running maximum is only reduced across them
//   when the lazy rescale fires (wave vote on the lane-local maxima).
//
// The tile is bound by the SIMD's vector ISSUE port, not by the matrix pipe: a 16x16x32 MFMA holds the port for 8 of its 16
// cycles, and the two waves of a SIMD share it -- per wave and 64-key tile 64 MFMAs (512 issue cycles) + 32 v_exp (256) + the
// softmax bookkeeping.  So the row sums l = sum_k P are accumulated ON THE MATRIX CORES (LSUM): one MFMA per (key slice, query
// block) with an all-ones A operand and the same B operand (P as bf16) as the P.V MFMAs -- 4 MFMAs (32 issue cycles) replace 32
// dependent v_add_f32 (128) and the s_nop hipcc puts between a v_exp and the add that consumes it (16 per tile).  Every row of
// the 16x16 result is the row sum, so every lane holds its query's total (no cross-lane reduction in the epilogue), and l sums
// exactly the bf16-rounded P that P.V uses.  The bf16 split-KV form has no 8 registers to spare for it (it spills) and keeps
// per-lane v_add_f32 sums, reduced across the four lanes in the epilogue -- of the same ROUNDED P: with sums of the unrounded
// exponentials the rounding of a dominant key's P (up to 64 under the lazy reference, so not a power of two) does not cancel
// between O and l, and a row with all its mass on one key comes out 2^-8 away from that key's v instead of equal to it.
//
// The wave index is a SCALAR (readfirstlane of threadIdx.x >> 6): hipcc cannot prove it uniform, and carried in a vector register
// it made every LDS-DMA destination a v_readfirstlane + M0 write (8 per tile and DMA wave) and the dma_wave test an EXEC-mask
// branch; as a scalar the issue of a tile is s_add / s_mov m0 / global_load_lds only (1.012x, profiles/r05_uw_attn_uniform_wave_ab.txt).
//
// NW = waves per workgroup: 8 (256 queries, three ring stages, tiles requested two ahead), or 4 (128 queries per workgroup,
// two ring stages = 64 KiB, so that TWO workgroups share a CU: SIMD partners then belong to different workgroups and are not
// coupled by the per-tile barrier; one's prologue / epilogue runs under the other's tiles).
//
// WIN = sliding window: per workgroup the key tiles [jt0, jt1) that the band of its query block touches; per wave and tile one of
// three wave-uniform cases -- outside the band of all 32 queries (no math), inside the band of all 32 (the dense tile, no mask), or
// an edge (element-wise -inf mask, a branch like the ragged tile's).
template <bool SPLIT, bool QK8, int NW = 8, bool F16 = false, bool WIN = false>
__global__ __launch_bounds__(64 * NW, 2) void attn_fwd16_kernel(const AttnParams p) {
  typedef typename at_elem<F16>::e elem_t;
  typedef typename at_elem<F16>::x8 elem8_t;
  constexpr float HR = F16 ? AT_F16_HEADROOM : 0.f;  // exponent headroom of P (log2 units)
  constexpr bool LSUM = !(SPLIT && !QK8);  // row sums on the matrix cores (the 16-bit split-KV form has no 8 registers to spare: it spills)
  constexpr int STAGE = QK8 ? AT_STAGE8 : AT_STAGE;
  constexpr int NST = NW == 8 ? 3 : 2, AHEAD = NST - 1;  // ring stages, prefetch distance in tiles
  static_assert(NW == 8 || (NW == 4 && !SPLIT && !QK8), "the 4-wave form exists for the plain 16-bit kernel only");
  static_assert(!WIN || (!SPLIT && !QK8), "the sliding window exists for the plain 16-bit kernel only");
  constexpr int VOFF = QK8 ? AT_K8 : AT_TILE;  // byte offset of the V tile inside a stage
  typedef int v4i __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, g4 = lane >> 4;
  int head = blockIdx.y, qblk = blockIdx.x;
  // Workgroup -> (head, query block).  The dispatcher hands workgroup L = x + gridDim.x * y to XCD L % 8, so with the plain
  // (x, y) = (query block, head) reading every XCD works on every head at once and each of the eight L2s streams every K / V
  // tile.  The remap gives XCD k the k-th contiguous eighth of the head-major sequence (bijective for any grid): the workgroups
  // an XCD runs at a time share ONE head, whose K / V tiles are then fetched by one L2 per pass instead of by all eight.
  if (!SPLIT) {
    const int nqb = gridDim.x, T = nqb * (int)gridDim.y, L = (int)blockIdx.x + nqb * (int)blockIdx.y;
    const int xq = T >> 3, xr = T & 7, xcd = L & 7;
    const int i = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (L >> 3);
    head = i / nqb;
    qblk = i - head * nqb;
  }
  const int q0 = qblk * (AT_QW * NW) + wave * AT_QW;
  const int nt = (p.Lk + AT_KB - 1) / AT_KB;
  // key tiles of this workgroup: all of them, or one contiguous share under split-KV (the host makes every share non-empty)
  // WIN: the tiles between the first key the block's first query sees and the last key its last query sees
  int wjt0 = 0, wjt1 = nt;
  if (WIN) {
    const int qa = qblk * (AT_QW * NW), qb = (qa + AT_QW * NW < p.Lq ? qa + AT_QW * NW : p.Lq) - 1;
    const int lo = qa + p.win_lo > 0 ? qa + p.win_lo : 0, hi = qb + p.win_hi < p.Lk - 1 ? qb + p.win_hi : p.Lk - 1;
    if (lo > hi) {  // no query of this block sees a key: rows of zeros (workgroup-uniform, before any barrier)
#pragma unroll
      for (int nq = 0; nq < 2; ++nq) {
        const int qr = q0 + 16 * nq + n16;
        if (qr < p.Lq) {
          uint16_t* op = p.o + (int64_t)qr * p.o_stride + head * AT_D + 4 * g4;
#pragma unroll
          for (int db = 0; db < 8; ++db) *reinterpret_cast<uint2*>(op + 16 * db) = make_uint2(0u, 0u);
        }
      }
      return;
    }
    wjt0 = lo / AT_KB;
    wjt1 = hi / AT_KB + 1;
  }
  const int jt0 = SPLIT ? (int)blockIdx.z * p.tiles_per_split : (WIN ? wjt0 : 0);
  const int jt1 = SPLIT ? (jt0 + p.tiles_per_split < nt ? jt0 + p.tiles_per_split : nt) : (WIN ? wjt1 : nt);
  // WIN: the wave's first and last query (clamped like the Q loads below, so rows past Lq repeat the last one) -- scalars
  int wqa = 0, wqb = 0;
  if (WIN) {
    wqa = q0 < p.Lq - 1 ? q0 : p.Lq - 1;
    wqb = q0 + AT_QW - 1 < p.Lq - 1 ? q0 + AT_QW - 1 : p.Lq - 1;
  }
  bool allseen = false;  // WIN: every row of the wave has had a visible key, i.e. has its reference (wave-uniform)
  const float c = p.c;

  // ---- Q fragments: query q0 + 16 nq + n16, d = 32 s + 8 g4 + [0, 8), pre-scaled by softmax scale * log2(e)
  // QK8: int8 codes, d = 64 s + 16 g4 + [0, 16); the query's scale delta_q rides in the exp2 coefficient c2[nq]
  elem8_t qf[QK8 ? 1 : 2][QK8 ? 1 : 4];
  v4i qf8[QK8 ? 2 : 1][QK8 ? 2 : 1];
  float c2[2] = {c, c};
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    int qr = q0 + 16 * nq + n16;
    if (qr >= p.Lq) qr = p.Lq - 1;
    if (QK8) {
      const int8_t* qp8 = p.q8 + (int64_t)qr * p.q8_stride + head * AT_D + 16 * g4;
#pragma unroll
      for (int s = 0; s < 2; ++s) qf8[QK8 ? nq : 0][QK8 ? s : 0] = *reinterpret_cast<const v4i*>(qp8 + 64 * s);
      c2[nq] = c * p.q_scale[(int64_t)head * p.qs_stride + qr];  // score = dot * delta_k * delta_q * softmax scale
    } else {
      const uint16_t* qp = p.q + (int64_t)qr * p.q_stride + head * AT_D + 8 * g4;
#pragma unroll
      for (int s = 0; s < 4; ++s) qf[QK8 ? 0 : nq][QK8 ? 0 : s] = *reinterpret_cast<const elem8_t*>(qp + 32 * s);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[QK8 ? 0 : nq][QK8 ? 0 : s][e] = (elem_t)((float)qf[QK8 ? 0 : nq][QK8 ? 0 : s][e] * c);
    }
  }

  // ---- LDS-DMA: waves 0-3 issue the whole tile, 8 pieces each (rows 16 w + 4 i + d_r of the K tile and of the V tile).  The
  // FIRST-dispatched half of the workgroup issues: those waves win the issue arbitration against their SIMD partners and would
  // otherwise wait at the barrier, and a piece costs less when only four waves issue (K on waves 0-3 and V on 4-7 measured
  // 0.974x, everything on 4-7 0.969x).  Per-lane byte offsets inside a tile are constants and a tile's base address is
  // wave-uniform, so a DMA costs no vector arithmetic: `base + zero-extended 32-bit lane offset` is the instruction's own
  // sgpr + vgpr addressing.  Only a ragged last tile clamps rows, on the slow path.
  typedef __attribute__((address_space(3))) void lds_void;
  typedef __attribute__((address_space(1))) const void glb_void;
  const bool dma_wave = wave < 4;
  const int d_r = lane >> 4;
#define A16_DOFF_V(stride, i) ((uint32_t)((16 * (wave & 3) + 4 * (i) + d_r) * (int)(stride) + head * AT_D + ((((lane & 15) ^ (d_r << 2)) ^ (i)) << 3)) * 2u)
#define A16_DOFF_K(stride, i) ((uint32_t)((16 * (wave & 3) + 4 * (i) + d_r) * (int)(stride) + head * AT_D + (((lane & 15) ^ (4 * (i) + d_r)) << 3)) * 2u)
  uint32_t d_k0 = QK8 ? 0u : A16_DOFF_K(p.k_stride, 0), d_k1 = QK8 ? 0u : A16_DOFF_K(p.k_stride, 1), d_k2 = QK8 ? 0u : A16_DOFF_K(p.k_stride, 2),
           d_k3 = QK8 ? 0u : A16_DOFF_K(p.k_stride, 3);
  // QK8: the K tile is int8 (8 rows x 128 B per 1-KiB piece, 2 pieces per DMA wave: rows 16 w + 8 i + (lane >> 3), physical chunk
  // lane & 7 holds logical chunk (lane & 7) ^ ((row >> 1) & 7)); waves 4 and 5 fetch the tile's 64 key scales / constants
  const int d8_r = lane >> 3;
#define A16_D8OFF(i) ((uint32_t)((16 * (wave & 3) + 8 * (i) + d8_r) * (int)p.k8_stride + head * AT_D + ((((lane & 7) ^ (((8 * (i) + d8_r) >> 1) & 7))) << 4)))
  const uint32_t d8_k0 = QK8 ? A16_D8OFF(0) : 0u, d8_k1 = QK8 ? A16_D8OFF(1) : 0u;
#undef A16_D8OFF
  uint32_t d_v0 = A16_DOFF_V(p.v_stride, 0), d_v1 = A16_DOFF_V(p.v_stride, 1), d_v2 = A16_DOFF_V(p.v_stride, 2), d_v3 = A16_DOFF_V(p.v_stride, 3);
#undef A16_DOFF_V
#undef A16_DOFF_K
#define A16_DMA_F(base, off, tilebyte, i) \
  __builtin_amdgcn_global_load_lds((glb_void*)((base) + (off)), (lds_void*)(sK_ + (tilebyte) + 1024 * (i)), 16, 0, 0);
#define A16_DMA_S(base, stride, tilebyte, i, j, kswz)                                                           \
  {                                                                                                             \
    int kr_ = (j) * AT_KB + 16 * (wave & 3) + 4 * (i) + d_r;                                                    \
    kr_ = kr_ < p.Lk ? kr_ : p.Lk - 1;                                                                          \
    const int col_ = head * AT_D + ((kswz ? ((lane & 15) ^ (4 * (i) + d_r)) : (((lane & 15) ^ (d_r << 2)) ^ (i))) << 3); \
    __builtin_amdgcn_global_load_lds((glb_void*)((base) + (int64_t)kr_ * (stride) + col_), (lds_void*)(sK_ + (tilebyte) + 1024 * (i)), 16, 0, 0); \
  }
#define A16_DMA8(j, stage)                                                                                      \
  do {                                                                                                          \
    char* st_ = smem + (stage) * STAGE;                                                                         \
    if (dma_wave) {                                                                                             \
      char* sK8_ = st_ + (wave & 3) * 2048;                                                                     \
      char* sK_ = st_ + (wave & 3) * 4096;                                                                      \
      if (((j) + 1) * AT_KB <= p.Lk) {                                                                          \
        const char* kt_ = reinterpret_cast<const char*>(p.k8) + (int64_t)(j) * AT_KB * p.k8_stride;             \
        const char* vt_ = reinterpret_cast<const char*>(p.v) + (int64_t)(j) * (AT_KB * 2) * p.v_stride;         \
        __builtin_amdgcn_global_load_lds((glb_void*)(kt_ + d8_k0), (lds_void*)(sK8_), 16, 0, 0);                \
        __builtin_amdgcn_global_load_lds((glb_void*)(kt_ + d8_k1), (lds_void*)(sK8_ + 1024), 16, 0, 0);         \
        A16_DMA_F(vt_, d_v0, AT_K8, 0) A16_DMA_F(vt_, d_v1, AT_K8, 1) A16_DMA_F(vt_, d_v2, AT_K8, 2) A16_DMA_F(vt_, d_v3, AT_K8, 3) \
      } else {                                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                      \
          int kr_ = (j) * AT_KB + 16 * (wave & 3) + 8 * i_ + d8_r;                                              \
          kr_ = kr_ < p.Lk ? kr_ : p.Lk - 1;                                                                    \
          const int col_ = head * AT_D + ((((lane & 7) ^ (((8 * i_ + d8_r) >> 1) & 7))) << 4);                  \
          __builtin_amdgcn_global_load_lds((glb_void*)(p.k8 + (int64_t)kr_ * p.k8_stride + col_), (lds_void*)(sK8_ + 1024 * i_), 16, 0, 0); \
        }                                                                                                       \
        A16_DMA_S(p.v, p.v_stride, AT_K8, 0, j, false) A16_DMA_S(p.v, p.v_stride, AT_K8, 1, j, false) A16_DMA_S(p.v, p.v_stride, AT_K8, 2, j, false) A16_DMA_S(p.v, p.v_stride, AT_K8, 3, j, false) \
      }                                                                                                         \
    } else if (wave < 6) { /* scale plane (wave 4) / constant plane (wave 5): 64 floats, one dword per lane */  \
      const float* sp_ = p.k_scale + (int64_t)(wave - 4) * p.H * p.ks_stride + (int64_t)head * p.ks_stride + (int64_t)(j) * AT_KB + lane; \
      __builtin_amdgcn_global_load_lds((glb_void*)sp_, (lds_void*)(st_ + AT_SC8 + (wave - 4) * 256), 4, 0, 0);  \
    }                                                                                                           \
  } while (0)
#define A16_DMA(j, stage)                                                                                       \
  do {                                                                                                          \
    if (QK8) { A16_DMA8(j, stage); break; }                                                                     \
    if (dma_wave) {                                                                                             \
      char* sK_ = smem + (stage) * AT_STAGE + (wave & 3) * 4096;                                                \
      if (((j) + 1) * AT_KB <= p.Lk) {                                                                          \
        const char* kt_ = reinterpret_cast<const char*>(p.k) + (int64_t)(j) * (AT_KB * 2) * p.k_stride;         \
        const char* vt_ = reinterpret_cast<const char*>(p.v) + (int64_t)(j) * (AT_KB * 2) * p.v_stride;         \
        A16_DMA_F(kt_, d_k0, 0, 0) A16_DMA_F(kt_, d_k1, 0, 1) A16_DMA_F(kt_, d_k2, 0, 2) A16_DMA_F(kt_, d_k3, 0, 3) \
        A16_DMA_F(vt_, d_v0, AT_TILE, 0) A16_DMA_F(vt_, d_v1, AT_TILE, 1) A16_DMA_F(vt_, d_v2, AT_TILE, 2) A16_DMA_F(vt_, d_v3, AT_TILE, 3) \
      } else {                                                                                                  \
        A16_DMA_S(p.k, p.k_stride, 0, 0, j, true) A16_DMA_S(p.k, p.k_stride, 0, 1, j, true) A16_DMA_S(p.k, p.k_stride, 0, 2, j, true) A16_DMA_S(p.k, p.k_stride, 0, 3, j, true) \
        A16_DMA_S(p.v, p.v_stride, AT_TILE, 0, j, false) A16_DMA_S(p.v, p.v_stride, AT_TILE, 1, j, false) A16_DMA_S(p.v, p.v_stride, AT_TILE, 2, j, false) A16_DMA_S(p.v, p.v_stride, AT_TILE, 3, j, false) \
      }                                                                                                         \
    }                                                                                                           \
  } while (0)

  // ---- fragment read offsets
  const int kap = 4 * (2 * ((n16 >> 2) & 1) + ((n16 >> 3) & 1)) + (n16 & 3);  // kappa(n16)
  uint32_t koff0 = kap * 256 + (((0 + g4) ^ kap) << 4), koff1 = kap * 256 + (((4 + g4) ^ kap) << 4);
  uint32_t koff2 = kap * 256 + (((8 + g4) ^ kap) << 4), koff3 = kap * 256 + (((12 + g4) ^ kap) << 4);
  // QK8: 128-B rows, chunk swizzle (row >> 1) & 7 (at_off8): row 16 kb + kappa, chunk 4 s + g4
  const uint32_t k8off0 = kap * 128 + (((0 + g4) ^ ((kap >> 1) & 7)) << 4), k8off1 = kap * 128 + (((4 + g4) ^ ((kap >> 1) & 7)) << 4);
  const int pg = 2 * (g4 & 1) + (g4 >> 1), tq = (lane >> 2) & 3, tp = lane & 3;
  const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)smem;
#define A16_VA(db) (uint32_t)(at_off(4 * pg + tq, 2 * (db) + (tp >> 1)) + 8 * (tp & 1))
  const uint32_t va0 = A16_VA(0), va1 = A16_VA(1), va2 = A16_VA(2), va3 = A16_VA(3);
  const uint32_t va4 = A16_VA(4), va5 = A16_VA(5), va6 = A16_VA(6), va7 = A16_VA(7);
#undef A16_VA

  f32x4 o[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int nq = 0; nq < 2; ++nq)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[i][nq][r] = 0.f;
  float m_run[2] = {QK8 ? -INFINITY : 0.f, QK8 ? -INFINITY : 0.f}, l_run[2] = {0.f, 0.f};
  f32x4 lacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // LSUM: row sums as MFMA accumulators (all four elements equal)
  elem8_t ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (elem_t)1.0f;
  asm volatile("" : "+v"(ones));  // one register quad for the whole kernel, not rematerialised per use
  // bf16 form: -m_run (log2 domain) in all four registers: the initial accumulator of the S chains of query block nq, rewritten
  // only when the running maximum moves (the first tile and lazy-rescale events)
  f32x4 sinit[2];
#pragma unroll
  for (int nq = 0; nq < 2; ++nq)
#pragma unroll
    for (int r = 0; r < 4; ++r) sinit[nq][r] = 0.f;

  // LDS-DMA instructions a wave issues per tile (= what may stay in flight behind a counted wait): 8 for the DMA waves of the
  // bf16 form (waves 4-7 issue none: any count passes); QK8: 6 for waves 0-3 (2 K + 4 V pieces), 1 for waves 4-5 (scales)
#define A16_WAIT_TILE_AHEAD()                                                               \
  do {                                                                                      \
    if (!QK8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                              \
    else if (wave < 4) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                     \
    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");                                   \
  } while (0)
  A16_DMA(jt0, 0);
  if (AHEAD == 2 && jt0 + 1 < jt1) {
    A16_DMA(jt0 + 1, 1);
    A16_WAIT_TILE_AHEAD();
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  // Static priority for the second-dispatched half of the workgroup: waves 4-7 lose every VALU / MFMA arbitration against their
  // SIMD partners (priority, then age) and are the critical path of a tile; one s_setprio for the whole kernel, no per-phase flips.
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(1);

  // The ring position (j - jt0) % NST is made a compile-time constant by unrolling the tile loop over the stages: every LDS
  // address of a tile is then `per-lane constant + immediate`.  Every wave is past the barrier that ended tile j-1, so the stage
  // that held it is free: tile j + AHEAD goes there.
  for (int j0 = jt0; j0 < jt1; j0 += NST) {
#pragma unroll
  for (int u = 0; u < NST; ++u) {
    const int j = j0 + u;
    if (j >= jt1) break;
    const char* sK = smem + u * STAGE;
    // (opaque to the optimiser on purpose: otherwise it keeps the eight lane offsets zero-extended to 64 bits -- sixteen
    // registers -- live across the whole loop and spills)
    asm volatile("" : "+v"(d_k0), "+v"(d_k1), "+v"(d_k2), "+v"(d_k3), "+v"(d_v0), "+v"(d_v1), "+v"(d_v2), "+v"(d_v3));
    if (j + AHEAD < jt1) A16_DMA(j + AHEAD, (u + AHEAD) % NST);
    // WIN: a tile none of the wave's 32 queries sees costs it the DMA issue above and the barrier below, nothing else
    if (!(WIN && (j * AT_KB + AT_KB - 1 < wqa + p.win_lo || j * AT_KB > wqb + p.win_hi))) {

    // ---------------- S^T blocks: fragment i = 4 kb + s read four ahead of its two MFMAs
    f32x4 sacc[4][2];
    if (!QK8) {
      // K fragments by asm reads with COUNTED waits: fragment i is waited for with the KA-1 younger reads still in flight
      // (hipcc merges the waits of the builtin form into three s_waitcnt lgkmcnt(0) per tile, each of which drains the
      // lookahead it was given; 2 and 6 in flight measured within 1 % of 4)
      constexpr int KA = 4;  // fragments in flight
      elem8_t kf[16];
      const uint32_t kbase = lds_base + u * STAGE;
      const uint32_t ka0 = kbase + koff0, ka1 = kbase + koff1, ka2 = kbase + koff2, ka3 = kbase + koff3;
#define A16_KR(i) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(kf[i]) : "v"(((i) & 3) == 0 ? ka0 : ((i) & 3) == 1 ? ka1 : ((i) & 3) == 2 ? ka2 : ka3), "n"(((i) >> 2) * 4096))
#pragma unroll
      for (int i = 0; i < KA; ++i) { A16_KR(i); }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i + KA < 16) { A16_KR(i + KA); }
        const int left = 15 - i < KA ? 15 - i : KA;  // reads younger than fragment i
        if (left == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(kf[i]));
        else if (left == 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(kf[i]));
        else if (left == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(kf[i]));
        else if (left == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(kf[i]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kf[i]));
        __builtin_amdgcn_sched_barrier(0);
        const int kb = i >> 2, s = i & 3;
        sacc[kb][0] = at_mfma(kf[i], qf[0][QK8 ? 0 : s], s == 0 ? sinit[0] : sacc[kb][0]);
        sacc[kb][1] = at_mfma(kf[i], qf[QK8 ? 0 : 1][QK8 ? 0 : s], s == 0 ? sinit[1] : sacc[kb][1]);
      }
#undef A16_KR
    } else {
      // int8: fragment i = 2 kb + s (d-slices of 64) on v_mfma_i32_16x16x64_i8; the accumulators START at the bit pattern of
      // 12582912.0f (file header), so their bits read as a float are 12582912 + dot, and one fma per score with the
      // key's scale and its precomputed constant gives t = dot * delta_k
      v4i ia[4][2], kf8[8];
      const v4i mg = {0x4B400000, 0x4B400000, 0x4B400000, 0x4B400000};
      f32x4 sk[4], sb[4];  // key scales / constants of the lane's four keys per key block: keys 16 kb + 4 pi(g) + e
      const uint32_t sa = lds_base + u * STAGE + AT_SC8 + 16 * pg;
#define A16_SC(dst, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(sa), "n"(off))
      A16_SC(sk[0], 0); A16_SC(sk[1], 64); A16_SC(sk[2], 128); A16_SC(sk[3], 192);
      A16_SC(sb[0], 256); A16_SC(sb[1], 320); A16_SC(sb[2], 384); A16_SC(sb[3], 448);
#define A16_KF8(i) kf8[i] = *reinterpret_cast<const v4i*>(sK + (((i) & 1) == 0 ? k8off0 : k8off1) + ((i) >> 1) * 2048)
      A16_KF8(0); A16_KF8(1); A16_KF8(2); A16_KF8(3);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i + 4 < 8) { A16_KF8(i + 4); }
        __builtin_amdgcn_sched_barrier(0);
        const int kb = i >> 1, s = i & 1;
        ia[kb][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf8[i], qf8[0][QK8 ? s : 0], s == 0 ? mg : ia[kb][0], 0, 0, 0);
        ia[kb][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf8[i], qf8[QK8 ? 1 : 0][QK8 ? s : 0], s == 0 ? mg : ia[kb][1], 0, 0, 0);
      }
#undef A16_KF8
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sk[0]), "+v"(sk[1]), "+v"(sk[2]), "+v"(sk[3]), "+v"(sb[0]), "+v"(sb[1]), "+v"(sb[2]), "+v"(sb[3]));
#undef A16_SC
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int nq = 0; nq < 2; ++nq)
#pragma unroll
          for (int e = 0; e < 4; ++e) sacc[kb][nq][e] = fmaf(__int_as_float(ia[kb][nq][e]), sk[kb][e], sb[kb][e]);
    }
    if (j == nt - 1 && (p.Lk & (AT_KB - 1))) {  // ragged last tile: keys >= Lk get -inf
      asm volatile("" ::: "memory");  // keeps this a branch: if-converted, it costs selects on EVERY tile
      const int kbase = j * AT_KB + 4 * pg;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (kbase + 16 * kb + e >= p.Lk) { sacc[kb][0][e] = -INFINITY; sacc[kb][1][e] = -INFINITY; }
    }
    // WIN: unless all 32 queries see the whole tile, keys outside a query's band get -inf.  Lane (n16, g4), element e of block
    // (kb, nq) is query 16 nq + n16 against key 64 j + 16 kb + 4 pi(g4) + e (layout above).
    if (WIN && (j * AT_KB < wqb + p.win_lo || j * AT_KB + AT_KB - 1 > wqa + p.win_hi)) {
      asm volatile("" ::: "memory");  // a branch, as above
#pragma unroll
      for (int nq = 0; nq < 2; ++nq) {
        int qi = q0 + 16 * nq + n16;
        qi = qi < p.Lq ? qi : p.Lq - 1;
        const int klo = qi + p.win_lo - (j * AT_KB + 4 * pg), khi = qi + p.win_hi - (j * AT_KB + 4 * pg);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * kb + e < klo || 16 * kb + e > khi) sacc[kb][nq][e] = -INFINITY;
      }
    }

    // ---------------- online softmax: lane-local maxima, cross-lane only when the reference moves
    // lane-local maxima of the tile's scores for the lazy-rescale vote
    float mx0 = sacc[0][0][0], mx1 = sacc[0][1][0];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 4; ++e) { mx0 = fmaxf(mx0, sacc[kb][0][e]); mx1 = fmaxf(mx1, sacc[kb][1][e]); }
    const bool first = (j == jt0);
    if (QK8) {
      // scores are dot * delta_k here; c2 = delta_q * scale * log2(e) is per lane and query block.  Running maximum in score
      // units, rescaled lazily (first tile: m_run = -inf, so the vote fires and alpha = 0 on the zero accumulators)
      if (__any(fmaxf((mx0 - m_run[0]) * c2[0], (mx1 - m_run[1]) * c2[1]) > 6.0f)) {
        asm volatile("" ::: "memory");
        float mx[2] = {mx0, mx1};
#pragma unroll
        for (int nq = 0; nq < 2; ++nq) {
          float m = mx[nq];
          m = fmaxf(m, __shfl_xor(m, 16, 64));
          m = fmaxf(m, __shfl_xor(m, 32, 64));
          const float m_new = fmaxf(m_run[nq], m);
          const float alpha = __builtin_amdgcn_exp2f((m_run[nq] - m_new) * c2[nq]);
          m_run[nq] = m_new;
          l_run[nq] *= alpha;
#pragma unroll
          for (int r = 0; r < 4; ++r) lacc[nq][r] *= alpha;
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][nq][r] *= alpha;
        }
      }
    } else if ((WIN ? !allseen : first) || __any(fmaxf(mx0, mx1) > 6.0f + HR)) {
      // The accumulators hold s * scale * log2(e) - m_run already (Q carries the scale, the MFMA chains started from -m_run), so
      // the maxima are the growth of the row maximum over the reference and p = exp2(acc) with no further arithmetic.  The first
      // tile fixes the reference at its own maximum (whatever its sign); later the reference only grows, lazily: when some
      // query's maximum exceeds it by more than 2^6 (wave-uniform vote) -- P stays <= 64 instead of <= 1, the same 8 significant
      // bits in bf16 -- and then O, l and this tile's scores are brought to the new reference.  fp16: the reference sits HR below
      // that (the chains start from HR - m_run, at no instruction in the loop), so the accumulators are HR larger throughout.
      //
      // WIN: the band starts at a different tile for every row, and the leading tiles of a later row are wholly masked: there
      // m = -inf, and taken as the reference it would make every score of the row NaN.  So a row's reference is fixed by the first
      // tile in which the ROW sees a key.  A row has its reference exactly when its sum l is positive (the key that fixed the
      // reference, and after every rescale the key that caused it, has P = 2^HR), and the MFMA row sums keep l in every lane of
      // the row, so that state costs no register.  A row without one: nothing visible in this tile -> delta = 0, its -inf scores
      // stay -inf and add P = 0; something visible -> delta = m whatever its sign, and O = l = 0 are left alone (alpha = 1, never
      // 0 * 2^-m).  A row with one treats a wholly masked tile as growth 0.  Until every row of the wave has its reference the
      // block runs on every tile (a few tiles at the head of the wave's band); from then on the vote alone decides, as without
      // a window.  A row that never sees a key keeps O = l = 0 and is written as zeros.
      asm volatile("" ::: "memory");  // keep this a branch
      float mx[2] = {mx0, mx1};
      bool rows_seen = true;
#pragma unroll
      for (int nq = 0; nq < 2; ++nq) {
        float m = mx[nq];
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (F16) m -= HR;
        const bool seen = WIN && lacc[nq][0] > 0.f, visible = m > -INFINITY;
        if (WIN) rows_seen = rows_seen && (seen || visible);
        const float delta = WIN ? (seen ? fmaxf(m, 0.f) : visible ? m : 0.f) : first ? m : fmaxf(m, 0.f);
        if (WIN || !first) {
          const float alpha = WIN && !seen ? 1.0f : __builtin_amdgcn_exp2f(-delta);
          l_run[nq] *= alpha;
#pragma unroll
          for (int r = 0; r < 4; ++r) lacc[nq][r] *= alpha;
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][nq][r] *= alpha;
        }
        m_run[nq] = !WIN && first ? delta : m_run[nq] + delta;  // (WIN: 0 until the row has its reference)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int e = 0; e < 4; ++e) sacc[kb][nq][e] -= delta;
#pragma unroll
        for (int r = 0; r < 4; ++r) sinit[nq][r] = -m_run[nq];
      }
      if (WIN) allseen = __all(rows_seen);
    }
    // P of key slice ks (32 keys) for query block nq: element j = 4 (kb & 1) + e of S block kb = 2 ks + (j >> 2)
    float ls0 = 0.f, ls1 = 0.f;
    // (fp16: the headroom rides in the constant of the exponent's fma)
    const float mc[2] = {QK8 ? (F16 ? fmaf(m_run[0], c2[0], -HR) : m_run[0] * c2[0]) : 0.f, QK8 ? (F16 ? fmaf(m_run[1], c2[1], -HR) : m_run[1] * c2[1]) : 0.f};
    elem8_t pf[2][2];
#define A16_EXP(kb, nq, e)                                                     \
  {                                                                            \
    const float x_ = __builtin_amdgcn_exp2f(QK8 ? fmaf(sacc[kb][nq][e], c2[nq], -mc[nq]) : sacc[kb][nq][e]); \
    const elem_t b_ = (elem_t)x_;                                              \
    if (!LSUM) { /* the sum of the ROUNDED P, as the MFMA form has it */        \
      if (nq == 0) { ls0 += (float)b_; asm volatile("" : "+v"(ls0)); }         \
      else { ls1 += (float)b_; asm volatile("" : "+v"(ls1)); }                 \
    }                                                                          \
    pf[(kb) >> 1][nq][4 * ((kb) & 1) + (e)] = b_;                              \
  }
#define A16_EXP4(kb, nq) A16_EXP(kb, nq, 0) A16_EXP(kb, nq, 1) A16_EXP(kb, nq, 2) A16_EXP(kb, nq, 3)

    // ---------------- O^T += V^T . P^T
    // The transposed reads go through inline asm: hipcc puts s_waitcnt vmcnt(0) in front of the builtin form whenever an LDS-DMA
    // is in flight (it cannot tell the stages apart), which would serialise the prefetch.  Reads of the next eight fragments are
    // issued before the MFMAs of the current ones; the counted lgkmcnt wait carries the eight registers it publishes as
    // operands so that the MFMAs cannot be scheduled above it.  The exponentials of key slice 1 are placed one behind each MFMA
    // of slice 0: an MFMA holds the issue port for 8 of its 16 cycles, so the wave's own softmax overlaps its own matrix work.
    const uint32_t vb = lds_base + u * STAGE;
    s16x4 ta0, ta1, ta2, ta3, ta4, ta5, ta6, ta7, tb0, tb1, tb2, tb3, tb4, tb5, tb6, tb7;
#define A16_TR(dst, areg, ks, jh) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(vb + areg), "n"(VOFF + 8192 * (ks) + 4096 * (jh)))
#define A16_TR8(P, ks, a0_, a1_, a2_, a3_)                                                                      \
  A16_TR(P##0, a0_, ks, 0); A16_TR(P##1, a0_, ks, 1); A16_TR(P##2, a1_, ks, 0); A16_TR(P##3, a1_, ks, 1);     \
  A16_TR(P##4, a2_, ks, 0); A16_TR(P##5, a2_, ks, 1); A16_TR(P##6, a3_, ks, 0); A16_TR(P##7, a3_, ks, 1)
#define A16_WAIT8(P, n)                                                                                    \
  asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(P##0), "+v"(P##1), "+v"(P##2), "+v"(P##3), "+v"(P##4), "+v"(P##5), "+v"(P##6), "+v"(P##7))
#define A16_PV(P, a, b, ks, db, nq) o[db][nq] = at_mfma(at_join<elem8_t>(P##a, P##b), pf[ks][nq], o[db][nq])
#define A16_F() __builtin_amdgcn_sched_barrier(0)
#define A16_LS(ks, nq) if (LSUM) lacc[nq] = at_mfma(ones, pf[ks][nq], lacc[nq])
    A16_TR8(ta, 0, va0, va1, va2, va3);
    A16_TR8(tb, 0, va4, va5, va6, va7);
    A16_EXP4(0, 0) A16_EXP4(1, 0) A16_EXP4(0, 1) A16_EXP4(1, 1)
    A16_F();
    A16_WAIT8(ta, 8);
    // slice 0, d blocks 0-3: one exponential of slice 1 behind every MFMA
    A16_PV(ta, 0, 1, 0, 0, 0); A16_F(); A16_EXP(2, 0, 0) A16_F(); A16_PV(ta, 0, 1, 0, 0, 1); A16_F(); A16_EXP(2, 0, 1) A16_F();
    A16_PV(ta, 2, 3, 0, 1, 0); A16_F(); A16_EXP(2, 0, 2) A16_F(); A16_PV(ta, 2, 3, 0, 1, 1); A16_F(); A16_EXP(2, 0, 3) A16_F();
    A16_PV(ta, 4, 5, 0, 2, 0); A16_F(); A16_EXP(3, 0, 0) A16_F(); A16_PV(ta, 4, 5, 0, 2, 1); A16_F(); A16_EXP(3, 0, 1) A16_F();
    A16_PV(ta, 6, 7, 0, 3, 0); A16_F(); A16_EXP(3, 0, 2) A16_F(); A16_PV(ta, 6, 7, 0, 3, 1); A16_F(); A16_EXP(3, 0, 3) A16_F();
    A16_LS(0, 0); A16_LS(0, 1);
    A16_TR8(ta, 1, va0, va1, va2, va3);
    A16_WAIT8(tb, 8);
    A16_PV(tb, 0, 1, 0, 4, 0); A16_F(); A16_EXP(2, 1, 0) A16_F(); A16_PV(tb, 0, 1, 0, 4, 1); A16_F(); A16_EXP(2, 1, 1) A16_F();
    A16_PV(tb, 2, 3, 0, 5, 0); A16_F(); A16_EXP(2, 1, 2) A16_F(); A16_PV(tb, 2, 3, 0, 5, 1); A16_F(); A16_EXP(2, 1, 3) A16_F();
    A16_PV(tb, 4, 5, 0, 6, 0); A16_F(); A16_EXP(3, 1, 0) A16_F(); A16_PV(tb, 4, 5, 0, 6, 1); A16_F(); A16_EXP(3, 1, 1) A16_F();
    A16_PV(tb, 6, 7, 0, 7, 0); A16_F(); A16_EXP(3, 1, 2) A16_F(); A16_PV(tb, 6, 7, 0, 7, 1); A16_F(); A16_EXP(3, 1, 3) A16_F();
    A16_TR8(tb, 1, va4, va5, va6, va7);
    A16_WAIT8(ta, 8);
    A16_PV(ta, 0, 1, 1, 0, 0); A16_PV(ta, 0, 1, 1, 0, 1); A16_PV(ta, 2, 3, 1, 1, 0); A16_PV(ta, 2, 3, 1, 1, 1);
    A16_PV(ta, 4, 5, 1, 2, 0); A16_PV(ta, 4, 5, 1, 2, 1); A16_PV(ta, 6, 7, 1, 3, 0); A16_PV(ta, 6, 7, 1, 3, 1);
    A16_LS(1, 0); A16_LS(1, 1);
    A16_WAIT8(tb, 0);
    A16_PV(tb, 0, 1, 1, 4, 0); A16_PV(tb, 0, 1, 1, 4, 1); A16_PV(tb, 2, 3, 1, 5, 0); A16_PV(tb, 2, 3, 1, 5, 1);
    A16_PV(tb, 4, 5, 1, 6, 0); A16_PV(tb, 4, 5, 1, 6, 1); A16_PV(tb, 6, 7, 1, 7, 0); A16_PV(tb, 6, 7, 1, 7, 1);
    if (!LSUM) {
      l_run[0] += ls0;
      l_run[1] += ls1;
    }
#undef A16_LS
#undef A16_EXP
#undef A16_EXP4
#undef A16_TR
#undef A16_TR8
#undef A16_WAIT8
#undef A16_PV
#undef A16_F
    }  // (WIN: the tile lies in the wave's band)
    // tile j+1 must have landed; the eight instructions of tile j+2 (if issued; waves 4-7 issue none) may stay in flight
    if (AHEAD == 2 && j + 2 < jt1) A16_WAIT_TILE_AHEAD();
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (two stages: the tile requested at the top of this one is the next)
    __builtin_amdgcn_s_barrier();  // bare: __syncthreads() would drain vmcnt to 0 and with it the prefetch
  }
  }
#undef A16_DMA
#undef A16_DMA8
#undef A16_WAIT_TILE_AHEAD
#undef A16_DMA_F
#undef A16_DMA_S

  // ---- epilogue: O[q, d] = O^T[d, q] / l ; lane holds d = 16 db + 4 g4 + e of query 16 nq + n16
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    float l;
    if (LSUM) {
      l = lacc[nq][0];  // row (any) x column n16 of the ones . P^T product: the whole row sum of query 16 nq + n16
    } else {
      l = l_run[nq];
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
    }
    if (SPLIT) {  // unnormalised partials; attn_combine_kernel merges the splits
      const int qs = q0 + 16 * nq + n16;
      if (qs < p.Lq) {
        float* po = p.part_o + ((int64_t)blockIdx.z * p.Lq + qs) * (p.H * AT_D) + head * AT_D + 4 * g4;
#pragma unroll
        for (int db = 0; db < 8; ++db)
          *reinterpret_cast<float4*>(po + 16 * db) = make_float4(o[db][nq][0], o[db][nq][1], o[db][nq][2], o[db][nq][3]);
        if (g4 == 0) {
          float* pm = p.part_ml + (((int64_t)blockIdx.z * p.Lq + qs) * p.H + head) * 2;
          // the merge kernel computes exp2((m - M) * p.c): hand it m in raw-score units (QK8: fold this query's delta_q in;
          // bf16 form: m_run already carries scale * log2(e))
          pm[0] = QK8 ? m_run[nq] * (c2[nq] / p.c) : m_run[nq] / p.c;
          pm[1] = l;
        }
      }
      continue;
    }
    const float inv = WIN ? (l > 0.f ? 1.0f / l : 0.f) : 1.0f / l;  // WIN: a row that saw no key is a row of zeros
    const int qr = q0 + 16 * nq + n16;
    if (qr < p.Lq) {
      uint16_t* op = p.o + (int64_t)qr * p.o_stride + head * AT_D + 4 * g4;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        typename at_elem<F16>::x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (elem_t)(o[db][nq][e] * inv);
        *reinterpret_cast<typename at_elem<F16>::x4*>(op + 16 * db) = b;
      }
    }
  }
}

// Split-KV merge: out[q, h, :] = sum_z w_z O_z / sum_z w_z l_z,  w_z = 2^{(m_z - max_z m_z) c}.  One thread per 4 channels.
template <bool F16>
__global__ __launch_bounds__(256) void attn_combine_kernel(const AttnParams p, int splits) {
  typedef typename at_elem<F16>::e elem_t;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_q = p.H * (AT_D / 4);
  const int64_t q = t / per_q;
  if (q >= p.Lq) return;
  const int r = (int)(t - q * per_q), h = r / (AT_D / 4), d4 = r % (AT_D / 4);
  float M = -INFINITY;
  for (int z = 0; z < splits; ++z) M = fmaxf(M, p.part_ml[(((int64_t)z * p.Lq + q) * p.H + h) * 2]);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float l = 0.f;
  for (int z = 0; z < splits; ++z) {
    const float* ml = p.part_ml + (((int64_t)z * p.Lq + q) * p.H + h) * 2;
    const float w = __builtin_amdgcn_exp2f((ml[0] - M) * p.c);
    const float4 v = *reinterpret_cast<const float4*>(p.part_o + ((int64_t)z * p.Lq + q) * (p.H * AT_D) + h * AT_D + 4 * d4);
    acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
    l += w * ml[1];
  }
  const float inv = 1.0f / l;
  typename at_elem<F16>::x4 b;
  b[0] = (elem_t)(acc.x * inv); b[1] = (elem_t)(acc.y * inv); b[2] = (elem_t)(acc.z * inv); b[3] = (elem_t)(acc.w * inv);
  *reinterpret_cast<typename at_elem<F16>::x4*>(p.o + q * p.o_stride + h * AT_D + 4 * d4) = b;
}

}  // namespace wanq

using namespace wanq;

extern "C" int64_t wanq_attention_split_workspace(int64_t Lq, int heads, int head_dim, int splits);

struct Qk8Args {  // int8 Q.K^T operands (NULL q8 = the bf16 form)
  const int8_t* q8;
  const int8_t* k8;
  const float* q_scale;
  const float* k_scale;
  int64_t q8_stride, k8_stride, qs_stride, ks_stride;
};

static volatile int64_t g_nw4_keys = -1;  // wanq_attention_select_form

// Dynamic LDS beyond the 64-KiB default for every instantiation: set once per process (thread-safe static initialiser).
static void allow_attn_dynamic_lds() {
  static const bool done = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE8);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE8);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<true, false, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, true, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE8);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<true, true, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE8);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 8, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 4, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 8, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * AT_STAGE);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd16_kernel<false, false, 4, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * AT_STAGE);
    return true;
  }();
  (void)done;
}

static int attention_impl(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq, int64_t Lk, int heads,
                          int head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, float scale,
                          int splits, void* workspace, int64_t workspace_bytes, void* stream, const Qk8Args* q8 = nullptr,
                          const int64_t* window = nullptr) {
  const char* what = q8 ? "wanq_attention_qk8_fwd" : window ? "wanq_attention_window_fwd" : "wanq_attention_fwd";
  WANQ_REQUIRE((q8 || (q && k)) && v && o, WANQ_E_ARG, "%s: NULL pointer", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: dtype must be WANQ_BF16 or WANQ_F16 (dtype code %d)", what, dtype);
  const bool f16 = dtype == WANQ_F16;
  WANQ_REQUIRE(head_dim == AT_D, WANQ_E_SHAPE, "%s: head_dim=%d, only 128 is implemented", what, head_dim);
  WANQ_REQUIRE(heads >= 1 && heads <= 65535, WANQ_E_SHAPE, "%s: heads=%d out of range", what, heads);
  WANQ_REQUIRE(Lq >= 0 && Lk >= 1 && Lq < (1ll << 30) && Lk < (1ll << 30), WANQ_E_SHAPE, "%s: bad lengths", what);
  const int64_t need = (int64_t)heads * head_dim;
  WANQ_REQUIRE(v_stride >= need && o_stride >= need && (q8 || (q_stride >= need && k_stride >= need)), WANQ_E_SHAPE,
               "%s: token stride smaller than heads*head_dim", what);
  WANQ_REQUIRE((v_stride | o_stride) % 8 == 0 && (q8 || (q_stride | k_stride) % 8 == 0), WANQ_E_SHAPE,
               "%s: strides must be multiples of 8 elements", what);
  WANQ_REQUIRE(v_stride < (1ll << 24) && (q8 || k_stride < (1ll << 24)), WANQ_E_SHAPE,
               "%s: k / v token stride must be below 2^24 elements (32-bit lane offsets inside a 64-key tile)", what);
  if (q8) {
    WANQ_REQUIRE(q8->q8 && q8->k8 && q8->q_scale && q8->k_scale, WANQ_E_ARG, "%s: NULL pointer", what);
    WANQ_REQUIRE(q8->q8_stride >= need && q8->k8_stride >= need && q8->q8_stride % 16 == 0 && q8->k8_stride % 16 == 0 &&
                     q8->k8_stride < (1ll << 24),
                 WANQ_E_SHAPE, "%s: int8 token strides must be multiples of 16 bytes, >= heads*128 and below 2^24", what);
    WANQ_REQUIRE(q8->qs_stride >= Lq && q8->ks_stride >= ((Lk + AT_KB - 1) / AT_KB) * AT_KB, WANQ_E_SHAPE,
                 "%s: scale planes are [heads][stride] with q stride >= Lq and k stride >= Lk rounded up to 64", what);
  }
  if (Lq == 0) return WANQ_OK;
  AttnParams p{(const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, (uint16_t*)o, q_stride, k_stride, v_stride, o_stride,
               (int)Lq, (int)Lk, heads, scale * 1.4426950408889634f};
  if (q8) {
    p.q8 = q8->q8; p.k8 = q8->k8; p.q_scale = q8->q_scale; p.k_scale = q8->k_scale;
    p.q8_stride = q8->q8_stride; p.k8_stride = q8->k8_stride; p.qs_stride = q8->qs_stride; p.ks_stride = q8->ks_stride;
  }
  dim3 grid((unsigned)((Lq + AT_QB - 1) / AT_QB), (unsigned)heads);
  const int nt = (int)((Lk + AT_KB - 1) / AT_KB);
  if (splits > nt) splits = nt;
  if (splits > 1) {
    p.tiles_per_split = (nt + splits - 1) / splits;
    splits = (nt + p.tiles_per_split - 1) / p.tiles_per_split;  // no empty share
  }
  hipStream_t st = (hipStream_t)stream;
  allow_attn_dynamic_lds();
  if (splits <= 1) {
    if (q8) {
      if (f16) hipLaunchKernelGGL((attn_fwd16_kernel<false, true, 8, true>), grid, dim3(512), 3 * AT_STAGE8, st, p);
      else hipLaunchKernelGGL((attn_fwd16_kernel<false, true>), grid, dim3(512), 3 * AT_STAGE8, st, p);
    } else {
      // 4-wave workgroups of 128 queries, two per CU (see attn_fwd16_kernel), up to WANQ_ATTN_NW4_KEYS keys (0 = never)
      static const int64_t nw4_env = [] { const char* e = getenv("WANQ_ATTN_NW4_KEYS"); return e ? atoll(e) : (int64_t)WANQ_ATTN_NW4_KEYS_DEFAULT; }();
      const int64_t nw4_sel = g_nw4_keys;  // wanq_attention_select_form: -1 = the start-up value
      const int64_t nw4_keys = nw4_sel >= 0 ? nw4_sel : nw4_env;
      const dim3 grid4((unsigned)((Lq + 4 * AT_QW - 1) / (4 * AT_QW)), (unsigned)heads);
      if (window && (window[0] >= 0 || window[1] >= 0)) {
        // Bounded on a side: the banded instantiations.  Query i sees keys [i + win_lo, i + win_hi]; an unbounded side and
        // anything wider than the problem is cut to where it changes nothing, so that the kernel's 32-bit sums cannot overflow
        // (Lq, Lk < 2^30).  The form is chosen as for the dense call, by the keys a 256-query block walks in place of Lk.
        const int64_t off = Lk - Lq, span = Lq > Lk ? Lq : Lk;
        const int64_t left = window[0] < 0 || window[0] > span ? span : window[0], right = window[1] < 0 || window[1] > span ? span : window[1];
        p.win_lo = (int)(off - left > -Lq ? off - left : -Lq);
        p.win_hi = (int)(off + right < Lk ? off + right : Lk);
        const int64_t band = left + right + AT_QB < Lk ? left + right + AT_QB : Lk;
        if (band <= nw4_keys) {
          if (f16) hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 4, true, true>), grid4, dim3(256), 2 * AT_STAGE, st, p);
          else hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 4, false, true>), grid4, dim3(256), 2 * AT_STAGE, st, p);
        } else if (f16) {
          hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 8, true, true>), grid, dim3(512), 3 * AT_STAGE, st, p);
        } else {
          hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 8, false, true>), grid, dim3(512), 3 * AT_STAGE, st, p);
        }
      } else if (Lk <= nw4_keys) {
        if (f16) hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 4, true>), grid4, dim3(256), 2 * AT_STAGE, st, p);
        else hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 4>), grid4, dim3(256), 2 * AT_STAGE, st, p);
      } else if (f16) {
        hipLaunchKernelGGL((attn_fwd16_kernel<false, false, 8, true>), grid, dim3(512), 3 * AT_STAGE, st, p);
      } else {
        hipLaunchKernelGGL((attn_fwd16_kernel<false, false>), grid, dim3(512), 3 * AT_STAGE, st, p);
      }
    }
    return check_launch(what);
  }
  const int64_t need_ws = wanq_attention_split_workspace(Lq, heads, head_dim, splits);
  WANQ_REQUIRE(workspace && workspace_bytes >= need_ws, WANQ_E_ARG,
               "%s: split-KV workspace of %lld bytes needed, %lld given", what, (long long)need_ws, (long long)workspace_bytes);
  WANQ_REQUIRE(((uintptr_t)workspace & 15) == 0, WANQ_E_ARG, "%s: workspace must be 16-byte aligned", what);
  p.part_o = static_cast<float*>(workspace);
  p.part_ml = p.part_o + (int64_t)splits * Lq * heads * AT_D;
  grid.z = (unsigned)splits;
  if (q8 && f16) hipLaunchKernelGGL((attn_fwd16_kernel<true, true, 8, true>), grid, dim3(512), 3 * AT_STAGE8, st, p);
  else if (q8) hipLaunchKernelGGL((attn_fwd16_kernel<true, true>), grid, dim3(512), 3 * AT_STAGE8, st, p);
  else if (f16) hipLaunchKernelGGL((attn_fwd16_kernel<true, false, 8, true>), grid, dim3(512), 3 * AT_STAGE, st, p);
  else hipLaunchKernelGGL((attn_fwd16_kernel<true, false>), grid, dim3(512), 3 * AT_STAGE, st, p);
  const int64_t threads = Lq * heads * (AT_D / 4);
  if (f16) hipLaunchKernelGGL(attn_combine_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p, splits);
  else hipLaunchKernelGGL(attn_combine_kernel<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p, splits);
  return check_launch(what);
}

extern "C" int64_t wanq_attention_split_workspace(int64_t Lq, int heads, int head_dim, int splits) {
  if (splits <= 1) return 0;
  return (int64_t)splits * Lq * heads * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int64_t wanq_attention_select_form(int64_t nw4_keys) {
  const int64_t prev = g_nw4_keys;
  g_nw4_keys = nw4_keys < -1 ? -1 : nw4_keys;
  return prev;
}

extern "C" int wanq_attention_fwd(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq,
                                  int64_t Lk, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, int64_t o_stride, float scale, void* stream) {
  return attention_impl(q, k, v, o, dtype, Lq, Lk, heads, head_dim, q_stride, k_stride, v_stride, o_stride, scale, 1, nullptr, 0, stream);
}

extern "C" int wanq_attention_window_fwd(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq, int64_t Lk,
                                         int heads, int head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                         int64_t o_stride, float scale, int64_t window_left, int64_t window_right, void* stream) {
  const int64_t window[2] = {window_left, window_right};
  return attention_impl(q, k, v, o, dtype, Lq, Lk, heads, head_dim, q_stride, k_stride, v_stride, o_stride, scale, 1, nullptr, 0, stream,
                        nullptr, window);
}

extern "C" int wanq_attention_fwd_split(const void* q, const void* k, const void* v, void* o, int dtype, int64_t Lq,
                                        int64_t Lk, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                                        int64_t v_stride, int64_t o_stride, float scale, int splits, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  WANQ_REQUIRE(splits >= 1 && splits <= 64, WANQ_E_ARG, "wanq_attention_fwd_split: splits=%d must be 1..64", splits);
  return attention_impl(q, k, v, o, dtype, Lq, Lk, heads, head_dim, q_stride, k_stride, v_stride, o_stride, scale, splits, workspace,
                        workspace_bytes, stream);
}

extern "C" int wanq_attention_qk8_fwd(const int8_t* q8, const float* q_scale, int64_t qs_stride, const int8_t* k8,
                                      const float* k_scale, int64_t ks_stride, const void* v, void* o, int dtype, int64_t Lq,
                                      int64_t Lk, int heads, int head_dim, int64_t q8_stride, int64_t k8_stride,
                                      int64_t v_stride, int64_t o_stride, float scale, int splits, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  WANQ_REQUIRE(splits >= 1 && splits <= 64, WANQ_E_ARG, "wanq_attention_qk8_fwd: splits=%d must be 1..64", splits);
  const Qk8Args a{q8, k8, q_scale, k_scale, q8_stride, k8_stride, qs_stride, ks_stride};
  return attention_impl(nullptr, nullptr, v, o, dtype, Lq, Lk, heads, head_dim, 0, 0, v_stride, o_stride, scale, splits, workspace,
                        workspace_bytes, stream, &a);
}
