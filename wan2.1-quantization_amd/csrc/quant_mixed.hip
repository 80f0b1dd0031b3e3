// wanq_quant_rows_mx_mixed: the row quantiser of the mixed MX format (include/wanq_hip.h) -- the producer of wanq_gemm_mx_mixed.  A row
// is gathered into the layer's channel order `perm`, its first n8 permuted channels are quantised to MXFP8 (e4m3, emax 8) and the
// others to MXFP4 (e2m1, emax 2), one E8M0 scale byte per block of 32 PERMUTED channels:
//   q[m, :n8], scale[m, :n8 / 32]  = wanq_quant_rows_mx(fmt E4M3) of x[m, perm[:n8]]
//   q[m, n8:], scale[m, n8 / 32:]  = wanq_quant_rows_mx(fmt E2M1) of x[m, perm[n8:]]
// bit for bit: the per-block arithmetic is mx_block.h's, and the GELU (elementwise, so it commutes with the gather) is applied in fp32
// behind the gather.
//
// Why a shape of its own.  The row frame of rowwise.hip keeps a row in registers in its stored order; a permutation would be a
// per-element global gather.  Here the permutation happens on chip: a panel of whole rows is copied global -> LDS as it is stored, in
// its input dtype, by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, 1 KiB per wave instruction, fully coalesced, no register
// staging), and every element is then read from LDS once, at its permuted place.  x is read from global memory once; there is no
// second pass.
//
// Work split.  A row has nb = cols / 32 permuted blocks.  A 256-thread workgroup owns NB x 256 block slots (NB = 1 for cols <= 8192,
// else 2); slot s = tid + 256 i is block s % nb of row s / nb of a panel of RP = 256 NB / nb whole rows (cols = 1536: 5 rows, 240 of
// 256 lanes busy; cols = 8960: one row, 280 of 512 slots).  A panel is contiguous in x, so its copy is linear.  One lane takes one
// WHOLE permuted block: its 32 gathered elements, the block maximum (no exchange), the scale byte and the codes -- 32 e4m3 bytes leave
// as two 16-byte stores, 32 e2m1 nibbles as one.  The four scale bytes of an aligned quad of blocks are put together by two DPP quad
// exchanges and leave as one dword (a row's cols / 32 scale bytes are 4-byte aligned, not more, for cols % 512 != 0).
// A slot's block does not depend on the panel, so its 32 channel indices are read ONCE per workgroup, before the loop, and kept in
// 16 registers (two 16-bit indices each); workgroups walk the panels with the grid's stride.
//
// Pipeline.  Two LDS buffers where two panels fit 64 KiB (every shape of the model; fp32 rows wider than 8192 columns take one):
//   wait for this wave's DMA of panel i | barrier | issue the DMA of panel i + 1 into the other buffer | gather | quantise | store
// one barrier per panel: the buffer a copy overwrites was last read before every wave passed the barrier.  With one buffer a
// second barrier behind the gather frees it for the next copy.
// LDS reads.  ds_read_u16 (16-bit inputs) or ds_read_b32 at data-dependent places: a permutation's bank conflicts are what they are;
// for the layer's own perm (two ascending runs) neighbouring lanes read neighbouring blocks' runs.
// Chunks of a copy past the end of x (the last panel of a launch) re-read x's last 16 bytes; they land in LDS rows no slot reads.
#include "mx_block.h"
#include "row_frame.h"

namespace wanq {
namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

struct MixedRowParams {
  const void* x;
  const int* perm;
  uint8_t* q;
  uint8_t* scale;
  int64_t rows, npanels;
  int cols, n8, act, rp, bufbytes, nbuf;
};

// a whole block in one lane: nothing to exchange
struct MxSelfLane {
  static __device__ __forceinline__ float x8(float v) { return v; }
  static __device__ __forceinline__ float x16(float v) { return v; }
};

// element `idx` of the staged row at LDS byte address `row0`
template <typename XT>
__device__ __forceinline__ float lds_elem(const char* row0, int idx) {
  if constexpr (std::is_same<XT, F32>::value) {
    return *reinterpret_cast<const float*>(row0 + idx * 4);
  } else if constexpr (std::is_same<XT, BF16>::value) {
    return __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(row0 + idx * 2)) << 16);
  } else {
    return __half2float(*reinterpret_cast<const __half*>(row0 + idx * 2));
  }
}

template <typename XT, int NB>
__global__ void __launch_bounds__(256) quant_rows_mx_mixed_kernel(const MixedRowParams p) {
  constexpr int ES = std::is_same<XT, F32>::value ? 4 : 2;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.cols, nb = C / 32, nb8 = p.n8 / 32, pitch = p.n8 + (C - p.n8) / 2;

  // ---- this thread's slots: (row of the panel, block), and the block's channel indices, read once
  int srow[NB], sblk[NB];
  bool sok[NB];
  uint32_t pidx[NB][16];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int s = tid + 256 * i, r = s / nb;
    sok[i] = r < p.rp;
    srow[i] = sok[i] ? r : 0;
    sblk[i] = sok[i] ? s - r * nb : 0;
    const int4* pp = reinterpret_cast<const int4*>(p.perm + 32 * sblk[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int4 v = pp[j];
      const int last = C - 1;  // (a bad index reads another channel of the row, never outside it)
      pidx[i][2 * j] = (uint32_t)min(max(v.x, 0), last) | ((uint32_t)min(max(v.y, 0), last) << 16);
      pidx[i][2 * j + 1] = (uint32_t)min(max(v.z, 0), last) | ((uint32_t)min(max(v.w, 0), last) << 16);
    }
  }

  // ---- the copy of a panel: chunk c = 256 j + tid of its 16-byte chunks to LDS byte 16 c; NJ instructions per wave
  const int64_t pchunks = (int64_t)p.rp * C * ES / 16, xchunks = p.rows * (int64_t)C * ES / 16;
  const int nj = p.bufbytes / 4096;
  auto issue = [&](int64_t panel, int buf) {
    char* dst = smem + buf * p.bufbytes + wave * 1024;
    const int64_t c0 = panel * pchunks + wave * 64 + lane;
    for (int j = 0; j < nj; ++j) {
      int64_t c = c0 + 256 * j;
      c = c < xchunks ? c : xchunks - 1;
      __builtin_amdgcn_global_load_lds((glb_void*)(static_cast<const char*>(p.x) + c * 16), (lds_void*)(dst + j * 4096), 16, 0, 0);
    }
  };

  int buf = 0;
  if ((int64_t)blockIdx.x < p.npanels) issue(blockIdx.x, 0);
  for (int64_t panel = blockIdx.x; panel < p.npanels; panel += gridDim.x) {
    const int64_t next = panel + gridDim.x;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (p.nbuf == 2 && next < p.npanels) issue(next, buf ^ 1);

    float v[NB][4][8];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const char* row0 = smem + buf * p.bufbytes + (int64_t)srow[i] * C * ES;
#pragma unroll
      for (int e = 0; e < 32; ++e) v[i][e >> 3][e & 7] = lds_elem<XT>(row0, (int)((pidx[i][e >> 1] >> (16 * (e & 1))) & 0xffffu));
    }
    if (p.nbuf == 1) {
      __syncthreads();
      if (next < p.npanels) issue(next, 0);
    } else {
      buf ^= 1;
    }

#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if (p.act == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][c][j] = gelu_tanh_fast_f32(v[i][c][j]);
      }
      float m = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) m = fmaxf(m, mx_block_amax<MxSelfLane>(v[i][c]));
      const bool seg8 = sblk[i] < nb8;
      const int s = seg8 ? mx_block_scale<8>(m) : mx_block_scale<2>(m);
      // the quad's four scale bytes as one dword (nb % 4 == 0: a quad of slots is four consecutive blocks of one row)
      uint32_t sw = (uint32_t)s << (8 * (lane & 3));
      sw |= (uint32_t)lane_xor_dpp<1>((int)sw);
      sw |= (uint32_t)lane_xor_dpp<2>((int)sw);
      const int64_t row = panel * p.rp + srow[i];
      if (!sok[i] || row >= p.rows) continue;
      float t[4][8];
#pragma unroll
      for (int c = 0; c < 4; ++c) mx_block_scaled(v[i][c], s, t[c]);
      uint8_t* qrow = p.q + row * pitch;
      if (seg8) {
        uint2 w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = e4m3_pack8(t[c]);
        uint4* dst = reinterpret_cast<uint4*>(qrow + 32 * sblk[i]);
        dst[0] = make_uint4(w[0].x, w[0].y, w[1].x, w[1].y);
        dst[1] = make_uint4(w[2].x, w[2].y, w[3].x, w[3].y);
      } else {
        *reinterpret_cast<uint4*>(qrow + p.n8 / 2 + 16 * sblk[i]) =
            make_uint4(e2m1_pack8(t[0]), e2m1_pack8(t[1]), e2m1_pack8(t[2]), e2m1_pack8(t[3]));
      }
      if ((lane & 3) == 0) *reinterpret_cast<uint32_t*>(p.scale + row * nb + sblk[i]) = sw;
    }
  }
}

}  // namespace
}  // namespace wanq

using namespace wanq;

extern "C" int wanq_quant_rows_mx_mixed(const void* x, int x_dtype, const int32_t* perm, int n8, uint8_t* q, uint8_t* scale_u8,
                                        int64_t rows, int cols, int act, void* stream) {
  const char* what = "wanq_quant_rows_mx_mixed";
  WANQ_REQUIRE(x && q && scale_u8, WANQ_E_ARG, "%s: x, q and scale_u8 must be non-NULL", what);
  WANQ_REQUIRE(perm, WANQ_E_ARG, "%s: perm must be non-NULL", what);
  WANQ_REQUIRE(is_fp(x_dtype), WANQ_E_ARG, "%s: bad x dtype %d", what, x_dtype);
  WANQ_REQUIRE(act == 0 || act == 1, WANQ_E_ARG, "%s: act must be 0 or 1", what);
  if (int e = check_rows(what, rows)) return e;
  WANQ_REQUIRE(cols >= 256 && cols % 128 == 0 && cols <= 16384, WANQ_E_SHAPE, "%s: cols=%d must be a multiple of 128 in [256, 16384]",
               what, cols);
  WANQ_REQUIRE(n8 >= 128 && n8 % 128 == 0 && cols - n8 >= 128, WANQ_E_SHAPE,
               "%s: n8=%d must be a multiple of 128 with 128 <= n8 <= cols - 128 (cols=%d)", what, n8, cols);
  WANQ_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(perm) & 15) == 0 && (reinterpret_cast<uintptr_t>(scale_u8) & 3) == 0,
               WANQ_E_ARG, "%s: x, q and perm must be 16-byte aligned, scale_u8 4-byte aligned", what);
  if (rows == 0) return WANQ_OK;
  const int nbk = cols / 32, NB = nbk <= 256 ? 1 : 2, es = x_dtype == WANQ_F32 ? 4 : 2;
  MixedRowParams p{x, perm, q, scale_u8, rows, 0, cols, n8, act, 256 * NB / nbk, 0, 0};
  p.npanels = (rows + p.rp - 1) / p.rp;
  p.bufbytes = (int)(((int64_t)p.rp * cols * es + 4095) / 4096 * 4096);
  p.nbuf = 2 * p.bufbytes <= 65536 ? 2 : 1;
  const dim3 grid((unsigned)(p.npanels < 2048 ? p.npanels : 2048));
  const size_t lds = (size_t)p.nbuf * p.bufbytes;
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto xt) {
    using XT = decltype(xt);
    if (NB == 1) hipLaunchKernelGGL((quant_rows_mx_mixed_kernel<XT, 1>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((quant_rows_mx_mixed_kernel<XT, 2>), grid, dim3(256), lds, st, p);
  };
  if (x_dtype == WANQ_F32) launch(F32{});
  else if (x_dtype == WANQ_BF16) launch(BF16{});
  else launch(F16{});
  return check_launch(what);
}
