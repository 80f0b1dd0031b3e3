// wanq_quant_rows_mx4_project: the MXFP4 (e2m1) row quantiser of rowwise.hip and, in the same pass over the row, its projection onto
// the 16-bit down factor of a low-rank branch -- the producer of wanq_gemm_mx4_lowrank (gemm_mx.hip):
//   q, scale_u8 = wanq_quant_rows_mx (fmt E2M1) or wanq_quant_rows_mx_had32 of x, bit for bit (the per-block arithmetic is mx_block.h)
//   xt = round_T(act(x))                       one rounding of the fp32 row (behind the GELU, IN FRONT of the rotation) to T = dtype16
//   t[m, r] = round_T(sum_k xt[m, k] a16[r, k])  fp32 on v_mfma_f32_16x16x32_{bf16,f16}, k ascending in 32-deep steps
// x is read from HBM once; the branch costs R / K of the Linear's matrix work and no second pass over the activation.
//
// Work split.  A 256-thread workgroup owns a panel of 64 whole rows, a wave 16 of them: one MFMA token block.  A wave walks its rows'
// columns in K-steps of 64; nothing is split over k and nothing is shared between workgroups, so codes, scale bytes and t of a row
// come from one wave, and the order of a row's additions depends on cols only -- not on rows, nor on the row's place in the launch.
// Rows past `rows` read row rows - 1 (computed, never stored).  Occupancy follows R: 16 KiB of LDS per 64 ranks.
//
// Registers: the row.  Lane (fr, fq) = (l & 15, l >> 4) loads, for each of the step's two 32-deep halves kk, the 8 elements
// x[row fr, 64 t + 32 kk + 8 fq ..+ 7] -- the MFMA's own token operand layout (gemm16_common.h), so the four lanes of a row read 128
// (fp32) or 64 contiguous bytes per half, and the two halves complete the 128-byte lines.  The loads of step t + 1 are issued, as raw
// bits, before step t is worked on.  These registers feed both consumers:
//   * the quantiser.  Block 2 t + kk of the row is the four chunks of lanes fr, fr + 16, fr + 32, fr + 48: Hadamard stages 1, 2, 4 stay
//     inside the chunk, stages 8 and 16 and the block maximum are v_permlane16_swap / v_permlane32_swap exchanges (rowwise.hip: DPP
//     quad exchanges; the same additions in the same order).  A lane stores its dword of eight nibbles, lane group 0 the scale byte.
//   * the MFMA.  The fp32 chunk behind the GELU is rounded to T and is the lane's B operand of step (t, kk) as it stands.
//
// LDS: a16 only.  A K-step's slice of a16 is R rows x 128 B, copied global -> LDS by LDS-DMA (global_load_lds_dwordx4, R / 32
// instructions per wave, each 8 rows) into one of two buffers, once per workgroup and step -- a16 (at most 256 x 16384 x 2 B) stays in L2
// and is never read per wave from global memory.  One barrier per step:
//   wait for this wave's loads of step t | barrier | issue DMA and row loads of step t + 1 | quantise step t | fragment reads + MFMAs
// so the buffer the DMA overwrites was last read before every wave passed the barrier.  The image is gemm16_common.h's: 128-B rows,
// the 16-B chunk index XORed with (row >> 1) & 7 on the DMA source address and on the reads.
// Banks.  The one LDS read pattern is the A-operand fragment: lane (fr, fq) reads the 16 bytes of logical chunk 4 kk + fq of row
// 16 j + fr (ds_read_b128, served in four groups of 16 lanes: one lane group fq, rows fr 0-15).  Two rows make a 256-B bank line, so
// within a group row fr sits in half fr & 1 of line fr >> 1 at physical chunk (4 kk + fq) ^ (fr >> 1): the eight lines take eight
// distinct chunk positions, each twice in opposite halves -- sixteen distinct 16-byte slots of the 64 banks, no conflict (the
// derivation of gemm_w8a8_pp.hip, whose image this is).  The rank-block offset 16 j rows = 2 KiB and the buffer offset leave the banks alone.
// Every wave reads the whole slice: R / 16 fragments per half against R / 16 MFMAs, read eight at a time.
//
// t leaves as 8-byte stores: a lane's four accumulators of rank block j are ranks 16 j + 4 fq ..+ 3 of token fr (ldt % 8 == 0).
#include "gemm16_common.h"
#include "mx_block.h"
#include "row_frame.h"

namespace wanq {
namespace {

struct QpParams {
  const void* x;
  uint8_t* q;
  uint8_t* scale;
  const void* a16;
  void* t;
  int64_t rows;
  int cols, ldt, act, had;
};

// the block's lanes in the MFMA token layout: chunk index = lane >> 4
struct MxMfmaLanes {
  static __device__ __forceinline__ float x8(float v) {
    const uint2 r = pair16(__float_as_int(v));
    return __uint_as_float(threadIdx.x & 16 ? r.x : r.y);
  }
  static __device__ __forceinline__ float x16(float v) {
    const uint2 r = pair32(__float_as_int(v));
    return __uint_as_float(threadIdx.x & 32 ? r.x : r.y);
  }
};

// 8 elements as loaded (the conversion waits for the load; the load is issued a step ahead)
template <typename XT>
struct Raw8 {
  uint4 lo, hi;
  __device__ __forceinline__ void load(const void* x, int64_t elem) {
    if constexpr (std::is_same<XT, F32>::value) {
      const uint4* p = reinterpret_cast<const uint4*>(static_cast<const char*>(x) + elem * 4);
      lo = p[0];
      hi = p[1];
    } else {
      lo = *reinterpret_cast<const uint4*>(static_cast<const char*>(x) + elem * 2);
    }
  }
  __device__ __forceinline__ void floats(float (&v)[8]) const {  // Io<XT>::load8's conversions
    if constexpr (std::is_same<XT, F32>::value) {
      v[0] = __uint_as_float(lo.x); v[1] = __uint_as_float(lo.y); v[2] = __uint_as_float(lo.z); v[3] = __uint_as_float(lo.w);
      v[4] = __uint_as_float(hi.x); v[5] = __uint_as_float(hi.y); v[6] = __uint_as_float(hi.z); v[7] = __uint_as_float(hi.w);
    } else if constexpr (std::is_same<XT, BF16>::value) {
      const uint32_t w[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
      }
    } else {
      const __half2* h = reinterpret_cast<const __half2*>(&lo);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float2 f = __half22float2(h[i]);
        v[2 * i] = f.x;
        v[2 * i + 1] = f.y;
      }
    }
  }
};

// NR: R / 64
template <typename XT, bool F16IN, int NR>
__global__ void __launch_bounds__(256, 2) quant_project_kernel(const QpParams p) {
  constexpr int T16 = F16IN ? WANQ_F16 : WANQ_BF16, R = 64 * NR, NJ = R / 16, SLICE = R * TROW, NG = NJ % 8 == 0 ? 8 : 4;
  __shared__ __attribute__((aligned(1024))) char smem[2 * SLICE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int C = p.cols, nk = C / TK;
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + fr;
  const bool row_ok = row < p.rows;
  const int64_t rbase = (row_ok ? row : p.rows - 1) * (int64_t)C;

  // a16's LDS-DMA source: instruction q of this wave fills LDS rows 32 q + 8 wave .. + 7, lane l row + (l >> 3), physical chunk l & 7;
  // (row >> 1) & 7 does not depend on q, so one pointer and a stride of 32 rows serve all R / 32 instructions
  const int ar = 8 * wave + (lane >> 3), ac = (lane & 7) ^ ((ar >> 1) & 7);
  const char* asrc = static_cast<const char*>(p.a16) + (int64_t)ar * C * 2 + ac * 16;
  const int64_t astride = (int64_t)32 * C * 2;
  auto issue = [&](int t) {
    char* dst = smem + (t & 1) * SLICE + wave * 1024;
#pragma unroll
    for (int q = 0; q < R / 32; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(asrc + q * astride + (int64_t)t * TROW), (lds_void*)(dst + q * 4096), 16, 0, 0);
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const uint32_t rd[2] = {frag_addr(lds0, fr, fq, 0), frag_addr(lds0, fr, fq, 1)};

  v4f acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = v4f{0.f, 0.f, 0.f, 0.f};

  Raw8<XT> cur[2], nxt[2];
  issue(0);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) nxt[kk].load(p.x, rbase + 32 * kk + 8 * fq);

  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    cur[0] = nxt[0];
    cur[1] = nxt[1];
    if (t + 1 < nk) {
      issue(t + 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) nxt[kk].load(p.x, rbase + (t + 1) * TK + 32 * kk + 8 * fq);
    }
    __builtin_amdgcn_sched_barrier(0);

    v4i xt[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      float v[8];
      cur[kk].floats(v);
      if (p.act == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_tanh_fast_f32(v[j]);
      }
      const float lo4[4] = {v[0], v[1], v[2], v[3]}, hi4[4] = {v[4], v[5], v[6], v[7]};
      const uint2 a = pack16x4<T16>(lo4), b = pack16x4<T16>(hi4);
      xt[kk] = v4i{(int)a.x, (int)a.y, (int)b.x, (int)b.y};
      if (p.had) mx_block_hadamard<MxMfmaLanes>(v, fq);
      const int s = mx_block_scale<2>(mx_block_amax<MxMfmaLanes>(v));
      float sc[8];
      mx_block_scaled(v, s, sc);
      const int64_t e = rbase + t * TK + 32 * kk + 8 * fq;
      if (row_ok) {
        *reinterpret_cast<uint32_t*>(p.q + (e >> 1)) = e2m1_pack8(sc);
        if (fq == 0) p.scale[e >> 5] = (uint8_t)s;
      }
    }

    const uint32_t bo = (t & 1) * SLICE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int g = 0; g < NJ / NG; ++g) {
        v4i fa[NG];
        const uint32_t ad = rd[kk] + bo + g * NG * 16 * TROW;
        dsr<0>(fa[0], ad); dsr<16 * TROW>(fa[1], ad); dsr<32 * TROW>(fa[2], ad); dsr<48 * TROW>(fa[3], ad);
        if constexpr (NG == 8) {
          dsr<64 * TROW>(fa[4], ad); dsr<80 * TROW>(fa[5], ad); dsr<96 * TROW>(fa[6], ad); dsr<112 * TROW>(fa[7], ad);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NG; ++j) acc[g * NG + j] = mfma<F16IN>(fa[j], xt[kk], acc[g * NG + j]);
        __builtin_amdgcn_sched_barrier(0);
      }
  }

  if (!row_ok) return;
  uint16_t* trow = static_cast<uint16_t*>(p.t) + row * (int64_t)p.ldt + 4 * fq;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float y[4] = {acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
    *reinterpret_cast<uint2*>(trow + 16 * j) = pack16x4<T16>(y);
  }
}

template <typename XT, bool F16IN>
void launch_quant_project(const QpParams& p, int R, hipStream_t st) {
  const dim3 grid((unsigned)((p.rows + 63) / 64));
  switch (R / 64) {
    case 1: hipLaunchKernelGGL((quant_project_kernel<XT, F16IN, 1>), grid, dim3(256), 0, st, p); break;
    case 2: hipLaunchKernelGGL((quant_project_kernel<XT, F16IN, 2>), grid, dim3(256), 0, st, p); break;
    case 3: hipLaunchKernelGGL((quant_project_kernel<XT, F16IN, 3>), grid, dim3(256), 0, st, p); break;
    default: hipLaunchKernelGGL((quant_project_kernel<XT, F16IN, 4>), grid, dim3(256), 0, st, p); break;
  }
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_quant_rows_mx4_project(const void* x, int x_dtype, uint8_t* q, uint8_t* scale_u8, const void* a16, int dtype16, int R,
                                           void* t, int ldt, int64_t rows, int cols, int act, int had32, void* stream) {
  const char* what = "wanq_quant_rows_mx4_project";
  WANQ_REQUIRE(x && q && scale_u8 && a16 && t, WANQ_E_ARG, "%s: x, q, scale_u8, a16 and t must be non-NULL", what);
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "%s: bad x dtype %d", what, x_dtype);
  WANQ_REQUIRE(dtype16 == WANQ_BF16 || dtype16 == WANQ_F16, WANQ_E_ARG, "%s: dtype16=%d must be BF16 or F16", what, dtype16);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "%s: act must be 0 or 1", what);
  WANQ_REQUIRE(had32 == 0 || had32 == 1, WANQ_E_ARG, "%s: had32 must be 0 or 1", what);
  if (int e = check_rows(what, rows)) return e;
  WANQ_REQUIRE(cols >= 128 && cols % 128 == 0 && cols <= 16384, WANQ_E_SHAPE, "%s: cols=%d must be a multiple of 128 in [128, 16384]",
               what, cols);
  WANQ_REQUIRE(R >= 64 && R <= 256 && R % 64 == 0, WANQ_E_SHAPE, "%s: R=%d must be a multiple of 64 in [64, 256]", what, R);
  WANQ_REQUIRE(ldt >= R && ldt % 8 == 0, WANQ_E_SHAPE, "%s: ldt=%d must be a multiple of 8 and at least R=%d", what, ldt, R);
  WANQ_REQUIRE(aligned(x, 16) && aligned(a16, 16) && aligned(t, 16) && aligned(q, 16), WANQ_E_ARG,
               "%s: x, a16, t and q must be 16-byte aligned", what);
  if (rows == 0) return WANQ_OK;
  const QpParams p{x, q, scale_u8, a16, t, rows, cols, ldt, act, had32};
  hipStream_t st = (hipStream_t)stream;
  const bool h = dtype16 == WANQ_F16;
  if (x_dtype == WANQ_F32) h ? launch_quant_project<F32, true>(p, R, st) : launch_quant_project<F32, false>(p, R, st);
  else if (x_dtype == WANQ_BF16) h ? launch_quant_project<BF16, true>(p, R, st) : launch_quant_project<BF16, false>(p, R, st);
  else h ? launch_quant_project<F16, true>(p, R, st) : launch_quant_project<F16, false>(p, R, st);
  return check_launch(what);
}
