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
//
// Low-rank branch (wanq_gemm_wq16_lowrank; LOWRANK below): y = y0 + lr with y0 exactly what the plain / grouped kernel has before GELU
// (fma(acc, sw[n], bias[n]) / acc + bias[n]) and lr[m,n] = sum_r t[m,r] b[n,r], t [M, R] and b [N, R] of the activation dtype, summed
// in fp32 on the same MFMA, 64-deep r-tiles ascending, in an accumulator set of its own; then GELU, gate + residual, one rounding.
// R % 64 == 0, 64 <= R <= 256.  For LoRC (b a = the best rank-r approximation of W - W_hat) and LoRA adapters on a quantised Linear;
// t = x a^T is the caller's wanq_gemm_bf16 launch.  A zero branch leaves the flag-off kernel's bits; lr is bit-equal to
// wanq_gemm_bf16(t, b) in fp32; a row's bits do not depend on M.  tests/test_gpu_wq16_lowrank.py.
//
// Tests.  tests/test_gpu_wq16_probes.py pins, on answers known bit for bit, what is this file's alone: the fragment cut (which
// byte / nibble of which load reaches which (K-tile, kk, fq) slot of which channel, the decode up to c + zp = +-255) and the
// group-row schedule below (row buffer g & 1 through its first reuse, the zp refresh, the fold, one K-tile per group), with a
// numpy model of both kernels as written and its single-error mutants (profiles/wq16_probe_mutants.txt).  The shared epilogue:
// tests/test_gpu_gemm16_probes.py.
#include "gemm16_common.h"

namespace wanq {
namespace {

constexpr int QLDS = 2 * XTILE;           // two K-tile buffers of token rows, 16 KiB each
constexpr int GROW = TN * 4;              // one group row of the tile's channels, fp32
constexpr int GLDS = QLDS + 4 * GROW;     // grouped: token buffers | sw rows 0, 1 | zp rows 0, 1

struct WqGemmParams : Gemm16Params {  // sw: fp32 [N], grouped [K / g][N]; sa: unused
  const float* zp;
  int tpg;  // grouped: K-tiles per group
};

struct WqLowRankParams : WqGemmParams {  // the low-rank branch: t [M, R], b [N, R] of the activation dtype
  const void* t;
  const void* b;
  int R;
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

template <int OFF>
__device__ __forceinline__ void dsr32(float& d, uint32_t addr) {
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

// ---- GROUPED: group-wise scales (wanq_gemm_wq16_grouped): sw / zp are [K / g][N], one row per group of g input channels ----------
//   part_g[m,n] = sum_{k in group g} a[m,k] (c[n,k] + zp[g,n]);  acc = fma(part_g, sw[g,n], acc), g ascending from acc = 0;
//   y = acc + bias; GELU / gate + residual; one rounding (epilogue16<OUT, false>).
// The plain kernel with a second accumulator set: the MFMAs of a group sum into part[4][4] in that kernel's order, and the last
// K-tile of a group ((t + 1) 64 % g == 0) folds part into acc with the group's scale -- one fp32 fma per element -- and zeroes it.
// The scale never touches the 16-bit operand.
// Group rows.  Holding a group's 16 scales per lane in registers next to 128 accumulators, 32 + 32 operand dwords and the next
// tile's codes spills (256 VGPRs, 16-48 bytes of scratch), so the rows of the workgroup's 128 channels travel as the token tile
// does: one 4-byte LDS-DMA per wave and group (waves 0, 1: sw; waves 2, 3: zp; channels past N read channel N - 1) into one of two
// 512-byte rows each behind the token buffers, ONE GROUP AHEAD -- the rows of group g + 1 are issued under the first K-tile of
// group g, behind the barrier that ends every read of the buffer they replace (group g - 1's), and retired by the next tile's
// vmcnt(0) + barrier, at least one K-tile before they are read.  A lane reads its 4 zp (channel j 16 + fr, the zadj of the
// conversion) at the top of a group's first tile and its 4 float4 of sw (channels j 16 + 4 fq .. + 3) at the fold, when the operand
// registers are dead.
//
// ---- LOWRANK: the 16-bit side branch (wanq_gemm_wq16_lowrank): y = y0 + lr, lr[m,n] = sum_r t[m,r] b[n,r] ----------------------
// Behind the quantised K loop both token buffers are free, and a 64-deep slice of (t, b) is one K-tile of gemm_bf16.hip's shape:
// the t rows of the tile's 128 tokens go into buffer 0 and the b rows of its 128 channels into buffer 1, by the same LDS-DMA into the
// same swizzled 128-byte rows, and the same frag_addr reads feed 32 MFMAs (b as the A operand, as the weight is) into `part` -- idle
// in the plain form, zero again behind the last fold in the grouped one.  Per low-rank tile:
//   barrier (every wave has read both buffers) | issue the DMA of both halves | wait for this wave's DMA | barrier | 8 + 8 fragment
//   reads | 32 MFMAs
// The copy is NOT overlapped with MFMAs of the same workgroup (both buffers are its target); it overlaps with the other workgroup
// on the CU.  The epilogue adds part behind the bias (epilogue16<.., LOWRANK>): one fp32 add, so a zero branch leaves the bits of the
// flag-off kernel.  lr is summed r-tiles ascending in gemm_bf16.hip's order: bit-equal to wanq_gemm_bf16(t, b) with an fp32 output.
template <bool F16IN, bool W4, int OUT, bool GROUPED, bool LOWRANK = false>
__global__ void __launch_bounds__(256, 2)
    gemm_wq16_kernel(std::conditional_t<LOWRANK, WqLowRankParams, WqGemmParams> p) {
  __shared__ __attribute__((aligned(1024))) char smem[GROUPED ? GLDS : QLDS];
  const Frame f(p.nt);
  const int K = p.K, nk = K / TK, tpg = p.tpg, ng = GROUPED ? nk / tpg : 0;

  const char* src[4];  // LDS-DMA sources (token rows only)
  dma_sources(p.a, f.m0, p.M, (int64_t)K * 2, f, src);
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // (the offset: k = t TK < K in int, then bytes; widened first it becomes a 64-bit induction variable per source)
  auto issue = [&](int t) { dma_issue<4>(src, (int64_t)(t * TK) * 2, smem + (t & 1) * XTILE + f.wave * 1024); };

  // ---- group rows: this wave's 64 channels of sw (waves 0, 1) or zp (waves 2, 3), lane l -> channel 64 (wave & 1) + l
  const bool has_zp = p.zp != nullptr;
  const bool grow_wave = f.wave < 2 || has_zp;
  const int grow_n = f.n0 + f.wn * 64 + f.lane < p.N ? f.n0 + f.wn * 64 + f.lane : p.N - 1;
  const float* grow_src = (f.wave < 2 ? static_cast<const float*>(p.sw) : p.zp) + grow_n;
  auto issue_group = [&](int g) {
    if (grow_wave)
      __builtin_amdgcn_global_load_lds((glb_void*)(grow_src + (int64_t)g * p.N),
                                       (lds_void*)(smem + QLDS + f.wm * 2 * GROW + (g & 1) * GROW + f.wn * 256), 4, 0, 0);
  };
  const uint32_t sw_rd = lds0 + QLDS + f.wn * 256 + f.fq * 16;            // + (g & 1) GROW + 64 j: channels 16 j + 4 fq .. + 3
  const uint32_t zp_rd = lds0 + QLDS + 2 * GROW + f.wn * 256 + f.fr * 4;  // + (g & 1) GROW + 64 j: channel 16 j + fr

  // ---- fragment geometry: lane l holds row (16-row block) + (l & 15), the 8 k of logical chunk 4 kk + (l >> 4)
  const uint32_t rd0 = frag_addr(lds0, f.fr, f.fq, 0), rd1 = frag_addr(lds0, f.fr, f.fq, 1);

  // ---- weight codes of this lane: channel block j, step kk -> W8: 8 bytes at k = 64 t + 32 kk + 8 fq; W4: dword fq of the 16-byte
  // group of codes 64 t + 32 kk .. + 31 (low nibbles = codes 8 fq .. + 3, high nibbles = codes 8 fq + 4 .. + 7)
  constexpr int CT = W4 ? TK / 2 : TK;  // bytes of codes per row and K-tile
  constexpr float ZOFF = W4 ? 0.f : 128.f;
  const uint8_t* wp[4];
  float zadj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nr = f.n0 + f.wn * 64 + j * 16 + f.fr;
    const int n = nr < p.N ? nr : p.N - 1;
    wp[j] = static_cast<const uint8_t*>(p.w) + (int64_t)n * (W4 ? K / 2 : K) + f.fq * (CT / 8);
    zadj[j] = GROUPED ? -ZOFF : (p.zp ? p.zp[n] : 0.f) - ZOFF;  // GROUPED: refreshed from the group's zp row
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

  v4f acc[4][4], part[4][4];  // part: GROUPED only
  zero_acc(acc);
  zero_acc(part);
  v4f (&sum)[4][4] = GROUPED ? part : acc;

  issue(0);
  if constexpr (GROUPED) issue_group(0);
  load_codes(0);
  int g = 0, tin = 0;  // GROUPED: group of tile t, and t's place in it
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue(t + 1);
    if (GROUPED && tin == 0) {
      if (g + 1 < ng) issue_group(g + 1);
      if (has_zp) {
        const uint32_t za = zp_rd + (g & 1) * GROW;
        float z0, z1, z2, z3;
        dsr32<0>(z0, za); dsr32<64>(z1, za); dsr32<128>(z2, za); dsr32<192>(z3, za);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(z0), "+v"(z1), "+v"(z2), "+v"(z3) : : "memory");
        zadj[0] = z0 - ZOFF; zadj[1] = z1 - ZOFF; zadj[2] = z2 - ZOFF; zadj[3] = z3 - ZOFF;
      }
    }
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
    const uint32_t xo = (t & 1) * XTILE + f.wm * 64 * TROW;
    v4i xa[2][4];
    dsr4<TROW>(xa[0], rd0 + xo);
    dsr4<TROW>(xa[1], rd1 + xo);
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
        for (int j = 0; j < 4; ++j) sum[i][j] = mfma<F16IN>(wb[kk][j], xa[kk][i], sum[i][j]);
    if (GROUPED && ++tin == tpg) {  // the group's last tile: fold
      __builtin_amdgcn_sched_barrier(0);  // the scale reads stay behind the MFMAs: their operands are dead by then
      const uint32_t sa = sw_rd + (g & 1) * GROW;
      v4i sr[4];
      dsr<0>(sr[0], sa); dsr<64>(sr[1], sa); dsr<128>(sr[2], sa); dsr<192>(sr[3], sa);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sr[0]), "+v"(sr[1]), "+v"(sr[2]), "+v"(sr[3]) : : "memory");
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v4f s4 = __builtin_bit_cast(v4f, sr[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] = __fmaf_rn(part[i][j][e], s4[e], acc[i][j][e]);
          part[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
      ++g;
      tin = 0;
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  if constexpr (LOWRANK) {
    const char *tsrc[4], *bsrc[4];
    dma_sources(p.t, f.m0, p.M, (int64_t)p.R * 2, f, tsrc);
    dma_sources(p.b, f.n0, p.N, (int64_t)p.R * 2, f, bsrc);
    const uint32_t xo = f.wm * 64 * TROW, wo = XTILE + f.wn * 64 * TROW;
    for (int s = 0, ns = p.R / TK; s < ns; ++s) {
      __builtin_amdgcn_s_barrier();  // the last K-tile's (the previous low-rank tile's) reads of both buffers are done
      __builtin_amdgcn_sched_barrier(0);
      dma_issue<4>(tsrc, (int64_t)(s * TK) * 2, smem + f.wave * 1024);
      dma_issue<4>(bsrc, (int64_t)(s * TK) * 2, smem + XTILE + f.wave * 1024);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      v4i xa[2][4], wb[2][4];
      dsr4<TROW>(wb[0], rd0 + wo);
      dsr4<TROW>(xa[0], rd0 + xo);
      dsr4<TROW>(wb[1], rd1 + wo);
      dsr4<TROW>(xa[1], rd1 + xo);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) part[i][j] = mfma<F16IN>(wb[kk][j], xa[kk][i], part[i][j]);
      __builtin_amdgcn_sched_barrier(0);
    }
    epilogue16<OUT, !GROUPED, false, true>(acc, part, f, p);
  } else {
    epilogue16<OUT, !GROUPED>(acc, f, p);
  }
}

template <bool GROUPED, bool LOWRANK = false, class KP>
int launch_wq16(const KP& p, int dtype, int w_bits, int out_dtype, hipStream_t st, const char* what) {
  return with_out_dtype(out_dtype, [&](auto o) {
    constexpr int OUT = decltype(o)::value;
    const bool f16 = dtype == WANQ_F16;
    if (w_bits == 4)
      return f16 ? launch_tiles(gemm_wq16_kernel<true, true, OUT, GROUPED, LOWRANK>, p, st, what)
                 : launch_tiles(gemm_wq16_kernel<false, true, OUT, GROUPED, LOWRANK>, p, st, what);
    return f16 ? launch_tiles(gemm_wq16_kernel<true, false, OUT, GROUPED, LOWRANK>, p, st, what)
               : launch_tiles(gemm_wq16_kernel<false, false, OUT, GROUPED, LOWRANK>, p, st, what);
  });
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
  const WqGemmParams p{gemm16_params(a, w, nullptr, sw, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K), zp, 0};
  return launch_wq16<false>(p, dtype, w_bits, out_dtype, (hipStream_t)stream, what);
}

extern "C" int wanq_gemm_wq16_grouped(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp,
                                      int group_size, void* out, int out_dtype, const void* bias, int bias_dtype,
                                      const float* gate, const void* residual, int epi_flags, int64_t M, int N, int K,
                                      void* stream) {
  const char* what = "wanq_gemm_wq16_grouped";
  WANQ_REQUIRE(a && w && out && sw, WANQ_E_ARG, "%s: a, w, out and sw must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  WANQ_REQUIRE(w_bits == 4 || w_bits == 8, WANQ_E_ARG, "%s: w_bits=%d must be 4 or 8", what, w_bits);
  if (const int rc = check_gemm16_shapes(what, 64, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  WANQ_REQUIRE(group_size >= 64 && group_size % 64 == 0, WANQ_E_SHAPE, "%s: group_size=%d must be a positive multiple of 64", what,
               group_size);
  WANQ_REQUIRE(K % group_size == 0, WANQ_E_SHAPE, "%s: K=%d must be a multiple of group_size=%d", what, K, group_size);
  WANQ_REQUIRE(aligned(sw, 16) && aligned(zp, 16), WANQ_E_ARG, "%s: sw and zp must be 16-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const WqGemmParams p{gemm16_params(a, w, nullptr, sw, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K), zp,
                       group_size / TK};
  return launch_wq16<true>(p, dtype, w_bits, out_dtype, (hipStream_t)stream, what);
}

extern "C" int wanq_gemm_wq16_lowrank(const void* a, const void* w, int dtype, int w_bits, const float* sw, const float* zp,
                                      int group_size, const void* t, const void* b, int R, void* out, int out_dtype,
                                      const void* bias, int bias_dtype, const float* gate, const void* residual, int epi_flags,
                                      int64_t M, int N, int K, void* stream) {
  const char* what = "wanq_gemm_wq16_lowrank";
  WANQ_REQUIRE(a && w && out && sw, WANQ_E_ARG, "%s: a, w, out and sw must be non-NULL", what);
  WANQ_REQUIRE(t && b, WANQ_E_ARG, "%s: t and b must be non-NULL", what);
  WANQ_REQUIRE(dtype == WANQ_BF16 || dtype == WANQ_F16, WANQ_E_ARG, "%s: operand dtype %d must be BF16 or F16", what, dtype);
  WANQ_REQUIRE(w_bits == 4 || w_bits == 8, WANQ_E_ARG, "%s: w_bits=%d must be 4 or 8", what, w_bits);
  if (const int rc = check_gemm16_shapes(what, 64, a, w, out, out_dtype, bias, bias_dtype, gate, residual, epi_flags, M, N,
                                         K))
    return rc;
  if (group_size != 0) {
    WANQ_REQUIRE(group_size >= 64 && group_size % 64 == 0, WANQ_E_SHAPE, "%s: group_size=%d must be a positive multiple of 64",
                 what, group_size);
    WANQ_REQUIRE(K % group_size == 0, WANQ_E_SHAPE, "%s: K=%d must be a multiple of group_size=%d", what, K, group_size);
  }
  WANQ_REQUIRE(R >= 64 && R <= 256 && R % 64 == 0, WANQ_E_SHAPE, "%s: R=%d must be 64, 128, 192 or 256", what, R);
  WANQ_REQUIRE(aligned(sw, 16) && aligned(zp, 16), WANQ_E_ARG, "%s: sw and zp must be 16-byte aligned", what);
  WANQ_REQUIRE(aligned(t, 16) && aligned(b, 16), WANQ_E_ARG, "%s: t and b must be 16-byte aligned", what);
  if (const int rc = check_gemm16_tail(what, bias, bias_dtype, gate, M, N)) return rc;
  if (M == 0) return WANQ_OK;
  const WqLowRankParams p{
      {gemm16_params(a, w, nullptr, sw, out, bias, bias_dtype, gate, residual, epi_flags, M, N, K), zp, group_size / TK}, t, b, R};
  return group_size ? launch_wq16<true, true>(p, dtype, w_bits, out_dtype, (hipStream_t)stream, what)
                    : launch_wq16<false, true>(p, dtype, w_bits, out_dtype, (hipStream_t)stream, what);
}
