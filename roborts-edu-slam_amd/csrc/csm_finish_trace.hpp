// csm_finish_trace.hpp — the finish kernels' three trace builds, kept out of
// their bodies: those hold stamp macros only, which expand to nothing in the
// default build. The globals and their exported readouts belong to one unit
// each: it defines CSM_TRACE_UNIT_EXACT (csm_finish.hip) or
// CSM_TRACE_UNIT_FAST (csm_finish_fast.hip) before its includes.
#pragma once
#include <hip/hip_runtime.h>

#include "csm_device.hpp"

// ---- CSM_FINISH_TRACE: wall-clock stamps of the exact pass's phases for the
// first kTraceWindows windows that take it (tools/finish_trace.py). The window's
// row sits in its LDS block (SortCounters::trace); thread 0 alone uses it.
#if defined(CSM_FINISH_TRACE) && defined(CSM_TRACE_UNIT_EXACT)
namespace csm {
constexpr int kTraceWindows = 256;
__device__ unsigned long long g_trace[kTraceWindows][10];
__device__ int g_trace_n;
// per sort level: [2 l] = wall clock at the level's start, [2 l + 1] =
// segments in it << 32 | the first segment's length (csm_debug_finish_levels)
constexpr int kTraceLevels = 16;
__device__ unsigned long long g_ltrace[kTraceWindows][2 * kTraceLevels];

__device__ __forceinline__ void trace_claim(int32_t* row, int n) {
  if (threadIdx.x != 0) return;
  const int tr = atomicAdd(&g_trace_n, 1);
  *row = tr < kTraceWindows ? tr : -1;
  if (*row >= 0) g_trace[*row][9] = (unsigned long long)n;
}
__device__ __forceinline__ void trace_put(const int32_t* row, int i, unsigned long long v) {
  if (threadIdx.x == 0 && *row >= 0) g_trace[*row][i] = v;
}
__device__ __forceinline__ void trace_level(const int32_t* row, int level, int ncur, int len0) {
  if (threadIdx.x == 0 && *row >= 0 && level < kTraceLevels) {
    g_ltrace[*row][2 * level] = wall_clock64();
    g_ltrace[*row][2 * level + 1] = ((unsigned long long)ncur << 32) | (unsigned)len0;
  }
}
}  // namespace csm
#define CSM_TRACE_CLAIM(row, n) ::csm::trace_claim(row, n)
#define CSM_STAMP(row, i) ::csm::trace_put(row, i, wall_clock64())
#define CSM_TRACE_VALUE(row, i, v) ::csm::trace_put(row, i, (unsigned long long)(v))
#define CSM_STAMP_LEVEL(row, level, ncur, len0) ::csm::trace_level(row, level, ncur, len0)

// Trace readout for tools/finish_trace.py: copies and resets the stamps.
extern "C" int csm_debug_finish_levels(unsigned long long* out, int max_windows) {
  int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(csm::g_trace_n), sizeof(int)) != hipSuccess) return -1;
  n = n < csm::kTraceWindows ? n : csm::kTraceWindows;
  n = n < max_windows ? n : max_windows;
  if (n > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(csm::g_ltrace),
                                   (size_t)n * 2 * csm::kTraceLevels * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  return n;
}

extern "C" int csm_debug_finish_trace(unsigned long long* out, int max_windows) {
  int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(csm::g_trace_n), sizeof(int)) != hipSuccess) return -1;
  n = n < max_windows ? n : max_windows;
  n = n < csm::kTraceWindows ? n : csm::kTraceWindows;
  if (n > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(csm::g_trace), (size_t)n * 10 * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  const int zero = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(csm::g_trace_n), &zero, sizeof(int));
  return n;
}
#else
#define CSM_TRACE_CLAIM(row, n) (void)(row)
#define CSM_STAMP(row, i) (void)(row)
#define CSM_TRACE_VALUE(row, i, v) (void)(row)
#define CSM_STAMP_LEVEL(row, level, ncur, len0) (void)(row)
#endif

// ---- CSM_TRACE_FASTBLK: per block of the fast pass: start, end (wall clock),
// hw id, then the phase stamps 16-25 of its window (plain stores: no
// same-address atomics). The stamps are the few-window trace's (CSM_TS_MIN /
// CSM_TS_MAX, csm_device.hpp), redirected; they read the kernel's FinishArgs A.
#if defined(CSM_TRACE_FASTBLK) && defined(CSM_TRACE_UNIT_FAST)
namespace csm {
constexpr int kFastBlkTrace = 4096;
__device__ unsigned long long g_fast_blk[kFastBlkTrace][16];
__device__ int g_fast_cand;  // record launches of this many candidates only (0: every launch)
}  // namespace csm
#define CSM_FASTBLK_PUT(col, v)                                                     \
  do {                                                                              \
    if (threadIdx.x == 0 && blockIdx.x < ::csm::kFastBlkTrace &&                    \
        (::csm::g_fast_cand == 0 || A.n_cand == ::csm::g_fast_cand))                \
      ::csm::g_fast_blk[blockIdx.x][col] = (unsigned long long)(v);                 \
  } while (0)
#undef CSM_TS_MIN
#undef CSM_TS_MAX
#define CSM_TS_MIN(slot) CSM_TS_MAX(slot)
#define CSM_TS_MAX(slot) CSM_FASTBLK_PUT((slot) - 13, wall_clock64())
#define CSM_FASTBLK_BEGIN() const unsigned long long fastblk_start = wall_clock64()
#define CSM_FASTBLK_END()                \
  do {                                   \
    CSM_FASTBLK_PUT(0, fastblk_start);   \
    CSM_FASTBLK_PUT(1, wall_clock64());  \
    CSM_FASTBLK_PUT(2, __smid());        \
  } while (0)

// Per-block (start, end, hw id, phase stamps) of the last fast-finish launch
// (of n_cand candidates if selected; tools/fast_blocks.py).
extern "C" int csm_debug_fast_select(int n_cand) {
  return hipMemcpyToSymbol(HIP_SYMBOL(csm::g_fast_cand), &n_cand, sizeof(int)) == hipSuccess ? 0 : -1;
}
extern "C" int csm_debug_fast_blocks(unsigned long long* out, int max_blocks) {
  const int n = max_blocks < csm::kFastBlkTrace ? max_blocks : csm::kFastBlkTrace;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(csm::g_fast_blk), (size_t)n * 16 * 8) == hipSuccess ? n : -1;
}
#else
#define CSM_FASTBLK_BEGIN() (void)0
#define CSM_FASTBLK_END() (void)0
#endif

// ---- CSM_TRACE_SMALL: the fast pass's stamps (slots 16-25; tools/small_trace.py).
// g_small_trace is one static per translation unit: this reads the fast unit's.
#if defined(CSM_TRACE_SMALL) && defined(CSM_TRACE_UNIT_FAST)
extern "C" int csm_debug_fast_trace(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(csm::dev::g_small_trace), 64 * 8) != hipSuccess) return -1;
  unsigned long long init[64] = {0};
  init[0] = init[16] = ~0ull;
  return hipMemcpyToSymbol(HIP_SYMBOL(csm::dev::g_small_trace), init, 64 * 8) == hipSuccess ? 0 : -1;
}
#endif
