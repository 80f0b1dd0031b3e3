// The transforms whose block mix is a Paley-I matrix:  y = hadU(x * premul),  hadU = (P_K (x) H_M) / fp32-sqrt(n),  n = K x M.
//   n =  8960 = 140 x  64  (Wan2.1-1.3B ffn.2 input): get_hadK picks K = 140 (quarot_utils.py:100-155; matmul_hadU :158-179; the
//                           reference multiplies by the dense 8960 x 8960 fp64 matrix, viditq_quant_layer.py:62-63).
//   n = 13824 = 108 x 128  (Wan2.1-14B ffn.2 input): REPO-DEFINED behaviour: the reference cannot rotate 13824
//                           columns at all -- get_hadK reaches `n % 144 == 0` first and asserts is_pow2(96) (quarot_utils.py:110-112)
//                           before its K = 108 branch (:118-121), which would fit.  This is that branch: the reference's
//                           own get_had108 table (= the Paley-I matrix of order 108, quadratic character mod 107), its butterfly over
//                           the 128 columns of every block and its fp32 sqrt (matmul_hadU, :158-179).  Pinned by
//                           tests/golden/a5_hadamard_13824.npz, which is made from the reference's table and loop.
// P_K is no butterfly: a dense +-1 mix of K x K per column (64 x 140 x 140 = 1.25 M adds per row of 8960, 4.1e10 per [32760, 8960]
// call), too many for the vector ALUs (> 0.5 ms at their peak).  So the mix runs on the matrix cores, exactly:
//   * the M-point Walsh-Hadamard transform of every block and the 1/sqrt(n) run on the vector ALUs in fp32 (M / 8 lanes x 8 elements
//     hold a block: 3 in-register + log2(M / 8) lane-exchange stages), in the natural layout the row is loaded in;
//   * every fp32 value is then split into three bf16 terms  v = hi + mid + lo  (each the RNE bf16 of the remainder: 3 x 8
//     significand bits = all 24), stored as three [KP][64] bf16 planes in LDS (KP = K padded to the MFMA's k-steps of 16);
//   * Y = P_K . V as v_mfma_f32_32x32x16_bf16 with A = P_K (entries +-1, exact in bf16, held in REGISTERS for the whole kernel:
//     generated from the quadratic character mod K - 1, never loaded) and B = the three planes accumulated into the same fp32
//     accumulator (read with ds_read_b64_tr_b16: the planes are row-major [k'][j] as written, the B operand wants k' along the
//     lane's elements).  Products are exact, sums are fp32: the result is an fp32 evaluation of the transform;
//   * Y goes back to the natural layout through LDS (fp32, over the plane area) for the optional fp output and the per-token quantiser.
// One workgroup (4 waves) per row at a time, rows round-robin, 2 workgroups per CU (54 / 42 KiB of LDS each) so that one's load /
// transform phase overlaps the other's MFMA phase.  The planes hold 64 columns: a 128-wide block goes through the matrix cores in
// two sequential halves.  The two orders are two parameter sets (PaleyOrder below); what they choose is which tiles of Y a wave owns:
//   140: a wave owns one 32-column half and 3 or 2 of the 5 row tiles of Y (140 -> 160), the 3 : 2 split alternating with the
//        workgroup's parity so that the two waves a SIMD hosts add up to 5;
//   108: wave w owns row tile w (of the 108 -> 128 rows of Y) for both 32-column sub-tiles of the half.
#include "row_frame.h"

namespace wanq {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct RotPaleyParams {
  const void* x;
  int x_dtype;
  const float* premul;
  void* out_fp;
  int out_dtype;
  int8_t* q;
  void* scale;
  void* sum;
  int vec_dtype;
  int64_t rows;
  float inv_div;
};

// One order: K blocks of M columns; a wave owns RT_ row tiles x CT_ column sub-tiles (32 x 32 each) of a half's Y.
template <int K_, int M_, int RT_, int CT_, bool RAW16_, bool B_ONE_STEP_, bool FMA_R_>
struct PaleyOrder {
  static constexpr int K = K_;                           // blocks per row = order of the Paley matrix
  static constexpr int Q = K - 1;                        // its prime
  static constexpr int M = M_;                           // columns per block
  static constexpr int N = K * M;
  static constexpr int LPB = M / 8;                      // lanes per block
  static constexpr int SLOTS = 256 / LPB;                // block slots per pass
  static constexpr int PASSES = (K + SLOTS - 1) / SLOTS;
  static constexpr int KSTEPS = (K + 15) / 16;           // the MFMA's k-steps
  static constexpr int KP = 16 * KSTEPS;                 // K padded to them
  static constexpr int PLANE = KP * 128;                 // one bf16 plane: KP rows of 64 columns
  static constexpr int HALVES = M / 64;
  static constexpr int TILES = (K + 31) / 32;            // row tiles of Y
  static constexpr int RT = RT_, CT = CT_;
  static constexpr int WC = 2 / CT, WR = 4 / WC;         // the 4 waves over a half's 2 column sub-tiles x the row tiles
  static constexpr bool LIGHT = WR * RT > TILES;         // 2 x 3 > 5: every other wave has no last row tile
  static constexpr bool PAD_SLOTS = SLOTS * PASSES == KP;  // the block slots K..KP-1 exist (loaded as zeros) and write the planes' padding rows
  static constexpr bool RAW16 = RAW16_;                  // 16-bit inputs are loaded as raw 16-B chunks, unpacked after the last request
  static constexpr bool B_ONE_STEP = B_ONE_STEP_;        // A fills the register file: one k-step of B fragments in flight at a time
  static constexpr bool FMA_R = FMA_R_;                  // the split's first remainder: see split3_store
  static constexpr int LDS = 3 * PLANE + 64;             // + [4] wave absmax, [4] wave code sums
  static_assert(M == 64 || M == 128, "8 or 16 lanes per block");
  static_assert(PAD_SLOTS || SLOTS * PASSES > KP, "every plane row has a block slot");
  static_assert(WR * RT == TILES || (LIGHT && WR == 2 && WR * RT == TILES + 1), "row tiles over the waves");
  static_assert((LIGHT ? K : 32 * TILES) * 64 * 4 <= 3 * PLANE, "Y (fp32, every row written) fits over the planes");
};
using Paley140 = PaleyOrder<140, 64, 3, 1, true, true, true>;
using Paley108 = PaleyOrder<108, 128, 1, 2, false, false, false>;

// byte offset of (row k', column j) in a plane: the row's two 64-B halves swap on rows 2, 3 (mod 4), so that the four rows a
// half-wave gathers with one transposed read cover all 64 banks (rows are 128 B = 32 banks: rows q and q + 2 would collide)
__device__ __forceinline__ int plane_off(int row, int col) { return row * 128 + ((col * 2) ^ (((row >> 1) & 1) << 6)); }

__device__ __forceinline__ uint32_t bf16_pair_bits(float a, float b) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 t;
  t[0] = (__bf16)a;
  t[1] = (__bf16)b;
  return __builtin_bit_cast(uint32_t, t);
}

// v = hi + mid + lo of the 8 values x = fl(v * c): 16 B at `off` of each plane.  The first remainder is x - hi (exact), or, FMA_R,
// fma(v, c, -hi): the product's own rounding error goes into mid / lo as well.  Both are pinned here and not left to -ffp-contract,
// which had picked the second at order 140 (scale and split in one basic block) and the first at 108: outputs are bit-exact to that.
template <bool FMA_R>
__device__ __forceinline__ void split3_store(char* smem, int plane, int off, const float (&v)[8], float c) {
#pragma clang fp contract(off)
  typedef float v2f __attribute__((ext_vector_type(2)));  // on element pairs (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32)
  const v2f c2 = {c, c};
  uint32_t hi[4], mid[4], lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v2f v2 = {v[2 * j], v[2 * j + 1]};
    const v2f x = v2 * c2;
    hi[j] = bf16_pair_bits(x.x, x.y);
    const v2f h = {__uint_as_float(hi[j] << 16), __uint_as_float(hi[j] & 0xffff0000u)};
    const v2f r = FMA_R ? __builtin_elementwise_fma(v2, c2, -h) : x - h;
    mid[j] = bf16_pair_bits(r.x, r.y);
    const v2f m = {__uint_as_float(mid[j] << 16), __uint_as_float(mid[j] & 0xffff0000u)};
    const v2f t = r - m;
    lo[j] = bf16_pair_bits(t.x, t.y);
  }
  *reinterpret_cast<uint4*>(smem + off) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  *reinterpret_cast<uint4*>(smem + plane + off) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
  *reinterpret_cast<uint4*>(smem + 2 * plane + off) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// A operand: row tiles mt0 .. mt0 + RT - 1 of P_K (first column +1, first row -1, diagonal +1, chi(m - k) elsewhere, zero padding),
// generated once from the quadratic character mod Q, which is tabulated in LDS (start-up only: it shares the plane area)
template <typename D>
__device__ __forceinline__ void paley_a_frags(int8_t* chi, int tid, int lane, int mt0, bf16x8 (&af)[D::RT][D::KSTEPS]) {
  if (tid < D::Q) chi[tid] = -1;
  __syncthreads();
  if (tid >= 1 && tid < D::Q) chi[(tid * tid) % D::Q] = 1;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < D::RT; ++t)
#pragma unroll
    for (int s = 0; s < D::KSTEPS; ++s) {
      const int m = 32 * (mt0 + t) + (lane & 31), k0 = 16 * s + 8 * (lane >> 5);
      const int idx0 = (m - k0 + 2 * D::Q) % D::Q;  // chi index of element 0; one step down per element
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        int idx = idx0 - i;
        idx += idx < 0 ? D::Q : 0;
        float e = (float)chi[idx];
        e = (m == k) ? 1.f : e;
        e = (m == 0) ? -1.f : e;
        e = (k == 0) ? 1.f : e;
        e = (m >= D::K || k >= D::K) ? 0.f : e;
        af[t][s][i] = (__bf16)e;
      }
    }
  __syncthreads();
}

// A row in the natural layout: pass ps of a thread is 8 columns at c8 of block bgrp + SLOTS * ps.
// (one dtype branch per ROW, not per chunk: with a branch per chunk hipcc waits for each load before it issues the next one)
template <typename D, typename T>
__device__ __forceinline__ void load_row(const void* x, int64_t rbase, int bgrp, int c8, float (&v)[D::PASSES][8]) {
#pragma unroll
  for (int ps = 0; ps < D::PASSES; ++ps) {
    const int b = bgrp + D::SLOTS * ps;
    if (b < D::K) Io<T>::load8(x, rbase + b * D::M + c8, v[ps]);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[ps][j] = 0.f;
    }
  }
}
template <typename D, typename T>
__device__ __forceinline__ void store_row(void* out, int64_t rbase, int bgrp, int c8, const float (&v)[D::PASSES][8]) {
#pragma unroll
  for (int ps = 0; ps < D::PASSES; ++ps) {
    const int b = bgrp + D::SLOTS * ps;
    if (b < D::K) Io<T>::store8(out, rbase + b * D::M + c8, v[ps]);
  }
}
// 16-bit inputs at 8960: the row's raw 16-B chunks.  (Requesting the NEXT row's chunks a row ahead was tried: the 20 registers they pin
// beside the 108 of A make hipcc spill, and a spill reload waits vmcnt(0), i.e. for that very prefetch -- 717 us with it, 664 us without.)
template <typename D>
__device__ __forceinline__ void load_raw16(const void* x, int64_t rbase, int bgrp, int c8, uint4 (&raw)[D::PASSES]) {
#pragma unroll
  for (int ps = 0; ps < D::PASSES; ++ps) {
    const int b = bgrp + D::SLOTS * ps;
    raw[ps] = b < D::K ? *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(x) + rbase + b * D::M + c8) : make_uint4(0, 0, 0, 0);
  }
}
template <bool BF, int P>
__device__ __forceinline__ void unpack16(const uint4 (&raw)[P], float (&v)[P][8]) {
#pragma unroll
  for (int ps = 0; ps < P; ++ps) {
    const uint32_t w[4] = {raw[ps].x, raw[ps].y, raw[ps].z, raw[ps].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (BF) {
        v[ps][2 * i] = __uint_as_float(w[i] << 16);
        v[ps][2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
      } else {
        const float2 f = __half22float2(*reinterpret_cast<const __half2*>(&w[i]));
        v[ps][2 * i] = f.x;
        v[ps][2 * i + 1] = f.y;
      }
    }
  }
}

// The butterfly stages between lanes MASK, 2 MASK, .. < LPB
template <int MASK, int LPB, int P>
__device__ __forceinline__ void lane_stages(float (&v)[P][8], int lane) {
  if constexpr (MASK < LPB) {
    const float sgn = (lane & MASK) ? -1.f : 1.f;
#pragma unroll
    for (int ps = 0; ps < P; ++ps)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[ps][j] = fmaf(sgn, v[ps][j], __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v[ps][j]), (MASK << 10) | 0x1f)));
    lane_stages<2 * MASK, LPB>(v, lane);
  }
}

template <typename D>
__device__ __forceinline__ void rotate_paley_body(const RotPaleyParams& p, char* smem) {
  constexpr int K = D::K, M = D::M, PASSES = D::PASSES, PLANE = D::PLANE, RT = D::RT, CT = D::CT, HALVES = D::HALVES;
  float* red = reinterpret_cast<float*>(smem + 3 * PLANE);     // [4] wave absmax
  int* red_i = reinterpret_cast<int*>(smem + 3 * PLANE + 32);  // [4] wave code sums
  float* ylds = reinterpret_cast<float*>(smem);                // Y of a half back in the natural layout: fp32 [32 TILES][64]
  const int tid_k = threadIdx.x, lane = tid_k & 63, wave = __builtin_amdgcn_readfirstlane(tid_k >> 6);

  // ---- this wave's tiles: column sub-tiles ct0 .. ct0 + CT - 1, row tiles mt0 .. mt0 + RT - 1 (a light wave: without the last)
  const int ct0 = (wave % D::WC) * CT;
  const bool heavy = !D::LIGHT || (((wave / D::WC) ^ (int)(blockIdx.x & 1)) == 0);
  const int mt0 = D::LIGHT ? (heavy ? 0 : RT) : (wave / D::WC) * RT;
  bf16x8 af[RT][D::KSTEPS];
  paley_a_frags<D>(reinterpret_cast<int8_t*>(smem), tid_k, lane, mt0, af);

  // transposed-read addresses (bytes within a plane, k-step 0): lane 4q+p of a 16-lane group gives row q, columns 4p..4p+3
  const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  const int trow = 8 * (grp >> 1) + tq, tcol = 32 * ct0 + 16 * (grp & 1) + 4 * tp;
  int a_lo[CT], a_hi[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    a_lo[c] = plane_off(trow, tcol + 32 * c);
    a_hi[c] = plane_off(trow + 4, tcol + 32 * c);
  }

  for (int64_t row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int64_t rbase = row * (int64_t)D::N;
    // keep the per-pass addresses of x / premul / out / q out of loop-invariant motion: hoisted, their 64-bit copies for every
    // pass and pointer stay live through the MFMA phase, next to the registers of A (108 at order 140), and spill
    int tid = tid_k;
    asm volatile("" : "+v"(tid));
    const int li = tid % D::LPB, bgrp = tid / D::LPB;  // lane within its block, block slot within a pass
    const int c8 = li * 8, pc8 = (li & 7) * 8;        // this lane's 8 columns: within the block, within a plane
    // ---- phase 1: load, premultiply, H_M per block
    if constexpr (!D::PAD_SLOTS) {  // no block slot writes the planes' padding rows K..KP-1, and Y overwrote them: zero them
      constexpr int CH = (D::KP - K) * 8;
      if (tid < 3 * CH) *reinterpret_cast<uint4*>(smem + (tid / CH) * PLANE + K * 128 + (tid % CH) * 16) = make_uint4(0, 0, 0, 0);
    }
    float v[PASSES][8];
    if (D::RAW16 && p.x_dtype != WANQ_F32) {
      uint4 raw[PASSES];
      load_raw16<D>(p.x, rbase, bgrp, c8, raw);
      if (p.x_dtype == WANQ_BF16) unpack16<true>(raw, v);
      else unpack16<false>(raw, v);
    } else if (!D::RAW16 && p.x_dtype == WANQ_BF16) load_row<D, BF16>(p.x, rbase, bgrp, c8, v);
    else if (!D::RAW16 && p.x_dtype == WANQ_F16) load_row<D, F16>(p.x, rbase, bgrp, c8, v);
    else load_row<D, F32>(p.x, rbase, bgrp, c8, v);
    if (p.premul) {
#pragma unroll
      for (int ps = 0; ps < PASSES; ++ps) {
        const int b = bgrp + D::SLOTS * ps;
        if (b < K) {
          float pm[8];
          Io<F32>::load8(p.premul, b * M + c8, pm);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[ps][j] *= pm[j];
        }
      }
    }
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
#pragma unroll
      for (int h = 1; h < 8; h <<= 1)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(j & h)) {
            const float a = v[ps][j], b2 = v[ps][j | h];
            v[ps][j] = a + b2;
            v[ps][j | h] = a - b2;
          }
    }
    lane_stages<1, D::LPB>(v, lane);

    float am = 0.f, amax = 0.f;
#pragma unroll
    for (int half = 0; half < HALVES; ++half) {
      const bool mine = HALVES == 1 || (li >> 3) == half;  // this lane's 8 columns belong to the half
      const bool last = half == HALVES - 1;
      // ---- scale, and the three bf16 planes of this half's 64 columns
      if (mine) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int b = bgrp + D::SLOTS * ps;
          if (D::PAD_SLOTS || b < K) split3_store<D::FMA_R>(smem, PLANE, plane_off(b, pc8), v[ps], p.inv_div);
        }
      }
      __syncthreads();

      // ---- phase 2: Y = P_K . (hi + mid + lo) on the matrix cores
      f32x16 acc[RT][CT];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][c][r] = 0.f;
#pragma unroll
      for (int s = 0; s < D::KSTEPS; ++s) {
        bf16x8 bf[CT][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const char* base = smem + pl * PLANE + s * 2048;
            const s16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + a_lo[c]));
            const s16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + a_hi[c]));
            bf[c][pl] = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7));
          }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          if (D::LIGHT && t == RT - 1 && !heavy) continue;
#pragma unroll
          for (int pl = 2; pl >= 0; --pl)  // smallest terms first
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[t][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t][s], bf[c][pl], acc[t][c], 0, 0, 0);
        }
        if constexpr (D::B_ONE_STEP) __builtin_amdgcn_sched_barrier(0);  // one k-step of B fragments in flight at a time (108 registers hold A)
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) am = fmaxf(am, fabsf(acc[t][c][r]));  // padded rows and a light wave's last tile are zeros
      if (last) {
        am = wave_max(am);
        if (lane == 0) red[wave] = am;
      }
      __syncthreads();  // every wave is done reading the planes

      // ---- Y back to the natural layout through LDS: accumulator register r of lane (n, hf) is row 8 (r >> 2) + (r & 3) + 4 hf of
      // its tile; of a light wave's last row tile, which is Y's last, only the rows below K (the others are the padding)
      {
        const int hf = (tid >> 5) & 1;
        float* yb = ylds + (32 * mt0 + 4 * hf) * 64 + 32 * ct0 + (tid & 31);
        auto tile = [&](int t, bool tail) {
#pragma unroll
          for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rt = 8 * (r >> 2) + (r & 3);
              if (!tail || rt + 4 * hf < K - 32 * (D::TILES - 1)) yb[(32 * t + rt) * 64 + 32 * c] = acc[t][c][r];
            }
        };
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          if (D::LIGHT && t == RT - 1 && !heavy) continue;
          if (D::LIGHT && !heavy && t == RT - 2) tile(t, true);  // a light wave ends on Y's last row tile
          else tile(t, false);
        }
      }
      if (last) amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
          const int b = bgrp + D::SLOTS * ps;
          if (b < K) {
            const float* yr = ylds + b * 64 + pc8;
            const float4 y0 = *reinterpret_cast<const float4*>(yr), y1 = *reinterpret_cast<const float4*>(yr + 4);
            v[ps][0] = y0.x; v[ps][1] = y0.y; v[ps][2] = y0.z; v[ps][3] = y0.w;
            v[ps][4] = y1.x; v[ps][5] = y1.y; v[ps][6] = y1.z; v[ps][7] = y1.w;
          }
        }
      }
      if (!last) __syncthreads();  // Y is consumed before the next half's planes overwrite it
    }

    // ---- phase 3: optional fp output, per-token int8 quantisation (qdiff DynamicQuantizer: base_quantizer.py:101-162)
    if (p.out_fp) {
      if (p.out_dtype == WANQ_BF16) store_row<D, BF16>(p.out_fp, rbase, bgrp, c8, v);
      else if (p.out_dtype == WANQ_F16) store_row<D, F16>(p.out_fp, rbase, bgrp, c8, v);
      else store_row<D, F32>(p.out_fp, rbase, bgrp, c8, v);
    }
    if (p.q) {
      const float scale = dyn_scale(amax, 127.0f, 1e-6f);
      const float inv = 1.0f / scale;
      int isum = 0;
#pragma unroll
      for (int ps = 0; ps < PASSES; ++ps) {
        const int b = bgrp + D::SLOTS * ps;
        if (b < K) {
          uint32_t pk[2];
          quantN_pack_rne<8>(v[ps], scale, inv, pk);
          isum = byte_sum(pk[1], byte_sum(pk[0], isum));
          *reinterpret_cast<uint2*>(p.q + rbase + b * M + c8) = make_uint2(pk[0], pk[1]);
        }
      }
      isum = wave_sum(isum);
      if (lane == 0) red_i[wave] = isum;
      __syncthreads();
      if (tid == 0) {
        vec_store(p.scale, p.vec_dtype, row, scale);
        if (p.sum) vec_store(p.sum, p.vec_dtype, row, (float)(red_i[0] + red_i[1] + red_i[2] + red_i[3]) * scale);
      }
    } else {
      __syncthreads();  // Y is consumed before the next row's planes overwrite it
    }
  }
}

__global__ __launch_bounds__(256, 2) void rotate140_kernel(const RotPaleyParams p) {
  __shared__ __attribute__((aligned(16))) char smem[Paley140::LDS];
  rotate_paley_body<Paley140>(p, smem);
}
__global__ __launch_bounds__(256, 2) void rotate108_kernel(const RotPaleyParams p) {
  __shared__ __attribute__((aligned(16))) char smem[Paley108::LDS];
  rotate_paley_body<Paley108>(p, smem);
}

int rotate_paley_rows(int had_k, const void* x, int x_dtype, const float* premul, void* out_fp, int out_dtype, int8_t* q, void* scale,
                      void* sum, int vec_dtype, int64_t rows, hipStream_t st, const char* what) {
  if (rows == 0) return WANQ_OK;
  RotPaleyParams p{};
  p.x = x; p.x_dtype = x_dtype; p.premul = premul; p.out_fp = out_fp; p.out_dtype = out_dtype; p.q = q; p.scale = scale; p.sum = sum;
  p.vec_dtype = vec_dtype; p.rows = rows; p.inv_div = 1.0f / sqrtf((float)(had_k == 140 ? Paley140::N : Paley108::N));
  const unsigned grid = (unsigned)(rows < 512 ? rows : 512);  // 2 resident workgroups per CU, rows round-robin
  if (had_k == 140) hipLaunchKernelGGL(rotate140_kernel, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(rotate108_kernel, dim3(grid), dim3(256), 0, st, p);
  return check_launch(what);
}

}  // namespace wanq
