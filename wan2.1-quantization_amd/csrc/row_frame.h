// Shared frame of the row-wise kernels (rowwise.hip, attn_prep.hip, quant_tools.hip, rotate.hip, rotate_paley.hip): the chunk
// layout of a row over one or four waves, the cross-wave reduction, the width -> (WPR, NCH) ladder, the scale rule of the
// dynamic 8-bit quantiser and the host-side shape checks.  Internal to csrc/.
//
// Data layout: every tensor is row-major [rows, cols]; a row is split into 16-byte-aligned chunks of 8 elements; chunk c of a
// row goes to lane (c % (64*WPR)), so one wave instruction reads 64 consecutive chunks (1 KiB for 16-bit inputs, 2 KiB for
// fp32) -- fully coalesced.  A row lives in registers between its reductions and its store: each element is read from HBM once
// and written once (algorithmic bytes == traffic).
//   WPR = 1: one wave per row (cols <= 2048), 4 rows per 256-thread workgroup, no barriers, no LDS.
//   WPR = 4: four waves per row (cols <= 16384), reductions finished through 64 B of LDS.
#pragma once
#include <type_traits>

#include "wanq_common.h"

namespace wanq {

// ---------------------------------------------------------------- host: shape checks of the row-wise entry points
inline int check_rows(const char* what, int64_t rows) {
  WANQ_REQUIRE(rows >= 0 && rows < (1ll << 31), WANQ_E_SHAPE, "%s: rows=%lld out of range", what, (long long)rows);
  return WANQ_OK;
}
inline int check_rows_cols(const char* what, int64_t rows, int cols) {
  if (int e = check_rows(what, rows)) return e;
  WANQ_REQUIRE(cols >= 8 && cols % 8 == 0 && cols <= 16384, WANQ_E_SHAPE,
               "%s: cols=%d must be a multiple of 8 in [8, 16384]", what, cols);
  return WANQ_OK;
}

// ---------------------------------------------------------------- device: 8 elements of a run-time dtype
__device__ __forceinline__ void load8_rt(const void* base, int dt, int64_t elem, float (&v)[8]) {
  if (dt == WANQ_F16) Io<F16>::load8(base, elem, v);
  else if (dt == WANQ_BF16) Io<BF16>::load8(base, elem, v);
  else Io<F32>::load8(base, elem, v);
}
__device__ __forceinline__ void store8_rt(void* base, int dt, int64_t elem, const float (&v)[8]) {
  if (dt == WANQ_F16) Io<F16>::store8(base, elem, v);
  else if (dt == WANQ_BF16) Io<BF16>::store8(base, elem, v);
  else Io<F32>::store8(base, elem, v);
}

// ---------------------------------------------------------------- device: where a thread stands in its row
// 256 threads; chunk slot i of a lane is chunk sub * 64 + lane + i * 64 * WPR of the row.
template <int WPR, int NCH>
struct RowFrame {
  static_assert(WPR == 1 || WPR == 4, "one or four waves per row");
  int lane, wave, sub;  // sub: the wave's place inside its row
  int64_t row;

  static dim3 grid(int64_t rows) { return dim3((unsigned)(WPR == 1 ? (rows + 3) / 4 : rows)); }

  __device__ __forceinline__ RowFrame()
      : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), sub(WPR == 1 ? 0 : wave),
        row(WPR == 1 ? (int64_t)blockIdx.x * 4 + wave : (int64_t)blockIdx.x) {}
  // surplus wave of the last workgroup: it returns at once (the wave-per-row variants have no barriers)
  __device__ __forceinline__ bool surplus(int64_t rows) const { return WPR == 1 && row >= rows; }
  __device__ __forceinline__ int col(int i) const { return (sub * 64 + lane + i * 64 * WPR) * 8; }

  // The row (C columns, first element rbase) into registers: ok[i] says whether slot i holds a chunk of the row; slots past
  // the row end are zero.
  // One dtype branch per ROW, not per chunk: with a branch per chunk hipcc waits for each load (s_waitcnt vmcnt(0) at the
  // branch's end) before it issues the next one, and a row's NCH loads run back to back in latency instead of in parallel.
  template <typename T>
  __device__ __forceinline__ void load_t(const void* x, int64_t rbase, int C, float (&v)[NCH][8], bool (&ok)[NCH]) const {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      ok[i] = col(i) < C;
      if (ok[i]) {
        Io<T>::load8(x, rbase + col(i), v[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
  }
  __device__ __forceinline__ void load(const void* x, int dt, int64_t rbase, int C, float (&v)[NCH][8], bool (&ok)[NCH]) const {
    if (dt == WANQ_F32) load_t<F32>(x, rbase, C, v, ok);
    else if (dt == WANQ_BF16) load_t<BF16>(x, rbase, C, v, ok);
    else load_t<F16>(x, rbase, C, v, ok);
  }
  template <typename T>
  __device__ __forceinline__ void store_t(void* out, int64_t rbase, const float (&v)[NCH][8], const bool (&ok)[NCH]) const {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (ok[i]) Io<T>::store8(out, rbase + col(i), v[i]);
  }
  __device__ __forceinline__ void store(void* out, int dt, int64_t rbase, const float (&v)[NCH][8], const bool (&ok)[NCH]) const {
    if (dt == WANQ_F32) store_t<F32>(out, rbase, v, ok);
    else if (dt == WANQ_BF16) store_t<BF16>(out, rbase, v, ok);
    else store_t<F16>(out, rbase, v, ok);
  }
};

// ---------------------------------------------------------------- device: a reduction over the row
// The wave butterfly first, then (WPR = 4) the four waves' results through LDS, slots 0..3 in order from the operation's
// identity.  slots: WPR values per reduction id; every id is used once per kernel, so one barrier per reduction suffices.
template <int WPR>
struct RowReduce {
  float* slots;
  int wave;
  template <typename OP, typename T>
  __device__ __forceinline__ T reduce(T v, int id) const {
    static_assert(sizeof(T) == sizeof(float), "one LDS slot per value");
    v = wave_reduce<OP>(v);
    if (WPR == 1) return v;
    T* s = reinterpret_cast<T*>(slots) + id * WPR;
    if ((threadIdx.x & 63) == 0) s[wave] = v;
    __syncthreads();
    T t = (T)OP::id;
#pragma unroll
    for (int w = 0; w < WPR; ++w) t = OP::f(t, s[w]);
    return t;
  }
};

// ---------------------------------------------------------------- host: width -> (WPR, NCH)
// launch(WPR, NCH, grid) with WPR and NCH as std::integral_constant: the smallest form whose 64 * WPR * NCH chunk slots hold
// the row's cols / 8 chunks.
template <typename F>
inline void row_ladder(int cols, int64_t rows, F&& launch) {
  const int chunks = cols / 8;
#define WANQ_STEP(WPR, NCH) \
  launch(std::integral_constant<int, WPR>{}, std::integral_constant<int, NCH>{}, RowFrame<WPR, NCH>::grid(rows))
  if (chunks <= 64) WANQ_STEP(1, 1);
  else if (chunks <= 128) WANQ_STEP(1, 2);
  else if (chunks <= 192) WANQ_STEP(1, 3);
  else if (chunks <= 256) WANQ_STEP(1, 4);
  else if (chunks <= 512) WANQ_STEP(4, 2);
  else if (chunks <= 768) WANQ_STEP(4, 3);
  else if (chunks <= 1024) WANQ_STEP(4, 4);
  else if (chunks <= 1280) WANQ_STEP(4, 5);
  else if (chunks <= 1536) WANQ_STEP(4, 6);
  else if (chunks <= 1792) WANQ_STEP(4, 7);
  else WANQ_STEP(4, 8);
#undef WANQ_STEP
}

// ---------------------------------------------------------------- device: tail of the dynamic quantiser
// scale = absmax / levels floored at `floor`: the qdiff eps rule (base_quantizer.py:122-127); 127 and 1e-6 for the 8-bit forms
__device__ __forceinline__ float dyn_scale(float amax, float levels, float floor) {
  float scale = amax / levels;
  if (scale < floor) scale = floor;
  return scale;
}
// acc + the sum of the four signed bytes of a packed dword
__device__ __forceinline__ int byte_sum(uint32_t packed, int acc) {
  return __builtin_amdgcn_sdot4((int)packed, 0x01010101, acc, false);
}

}  // namespace wanq
