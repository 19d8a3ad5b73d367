// csm_finish.hip — device-side finish of a window, the exact pass: the
// reference's std::sort(candidates, greater) (correlate_scan_matcher.h:607)
// reproduced EXACTLY (same permutation, ties included; the emulation and why
// it is one: csm_introsort.hpp), then the three ordered scans that consume the
// sorted candidates: FindBestCandidate's prefix (:670-710) and the candidate
// lists of ComputePositionalCovariance (:911-928) and
// ComputeAngularCovariance (:985-1003). The fast pass that runs before it and
// flags the windows it must take is csm_finish_fast.hip; the LDS carve is
// csm_internal.hpp's finish_layout.
#define CSM_TRACE_UNIT_EXACT
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "csm_device.hpp"
#include "csm_finish_trace.hpp"
#include "csm_internal.hpp"
#include "csm_introsort.hpp"
#include "csm_tail.hpp"

#pragma clang fp contract(off)

namespace csm {

namespace {

using namespace dev;
using namespace introsort;

// Partial sort (positions past what the ordered scans read stay unsorted) for
// windows of at least this many candidates.
#ifndef CSM_PARTIAL_MIN
#define CSM_PARTIAL_MIN 256
#endif
constexpr int kPartialMinCand = CSM_PARTIAL_MIN;
#ifndef CSM_EXACT_GRID
#define CSM_EXACT_GRID 512  // blocks of a listed exact pass (they walk the list of flagged windows)
#endif

// Block-wide reduction (all threads of the 4-wave block must call it).
__device__ double block_max(double v, FinishShared* sh, int wave) {
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  __syncthreads();  // sh->red is free
  if ((threadIdx.x & 63) == 0) sh->red[wave] = v;
  __syncthreads();
  double r = sh->red[0];
  for (int i = 1; i < kWaves; ++i) r = sh->red[i] > r ? sh->red[i] : r;
  return r;
}

// Step 1. Reads the window's n scores. Leaves keys[i] = score, vals[i] = i,
// and (complete at the caller's next barrier) sh->nan = any NaN, sh->cnt_a =
// FindBest's prefix size; zeroes sh->cnt_b.
__device__ __forceinline__ void load_scores(const double* __restrict__ sc, int n, double* keys, uint16_t* vals,
                                            FinishShared* sh) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  // Load, and the limits of the partial sort: max, NaN, and the FindBest
  // prefix size (every element in_response_band(s, max): the prefix is
  // exactly that set, in sorted order).
  double lmax = -INFINITY;
  bool lnan = false;
  for (int i = threadIdx.x; i < n; i += 64 * kWaves) {
    const double x = sc[i];
    keys[i] = x;
    vals[i] = (uint16_t)i;
    lnan |= x != x;
    lmax = x > lmax ? x : lmax;
  }
  lmax = block_max(lmax, sh, wave);
  CSM_STAMP(&sh->sort.trace, 1);
  if (threadIdx.x == 0) {
    sh->nan = 0;
    sh->cnt_a = 0;
    sh->cnt_b = 0;
  }
  __syncthreads();
  if (__ballot(lnan) != 0 && lane == 0) atomicOr(&sh->nan, 1);
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 64 * kWaves) c += in_response_band(keys[i], lmax) ? 1 : 0;
  c = wave_sum_i(c);
  if (lane == 0) atomicAdd(&sh->cnt_a, c);
}

// Step 2's limit. Reads sh->nan and sh->cnt_a (after a barrier).
// stage 1: FindBest's prefix and the positional list's 20
// (small windows sort whole: the limits' extra passes cost more there)
__device__ __forceinline__ int stage1_limit(const FinishArgs& A, const FinishShared* sh, int n) {
  const bool full = sh->nan || A.order_out != nullptr || n < kPartialMinCand;
  const int need = (A.skip_lists & 1) ? 1 : kCovPoints;  // the positional list reads 20
  return full ? n : min(n, max(sh->cnt_a, need));
}

// Step 3. Reads the sorted prefix of keys / vals and the window's angle rows.
// Leaves FindBest's header fields in *o and the averaged best (x, y) in
// sh->bx, sh->by; `scratch` (scratch_bytes of LDS, free between the sort's
// runs) holds the staged angle rows meanwhile.
__device__ __forceinline__ void find_best_staged(const ScanWork& S, const AngleEntry* __restrict__ angles,
                                                 const CandGrid& g, const double* keys, const uint16_t* vals, int n,
                                                 double best, char* scratch, size_t scratch_bytes, FinishOut* o,
                                                 FinishShared* sh) {
  // The window's angle rows (cos, sin) in LDS for FindBest's sequential sums:
  // one dependent global load per prefix element made the loop latency-bound
  // (the super-fine level's prefix holds most of its 189 candidates). The
  // partition scratch (lpos .. stack) is free until stage 2 rewrites it.
  const int n_ang = n / (g.n_space * g.n_space);
  double2* acs = reinterpret_cast<double2*>(scratch);
  const bool staged = (size_t)n_ang * sizeof(double2) <= scratch_bytes;  // (not into the FinishOut)
  if (staged)
    for (int t = threadIdx.x; t < n_ang; t += 64 * kWaves) {
      const AngleEntry ae = angles[S.angle_off + t];
      acs[t] = make_double2(ae.cosine, ae.sine);
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    auto cos_sin = [&](int a) {
      const AngleEntry ae = staged ? AngleEntry{0.0, acs[a].x, acs[a].y} : angles[S.angle_off + a];
      return CosSin{ae.cosine, ae.sine};
    };
    find_best(keys, vals, n, best, g, cos_sin, o, &sh->bx, &sh->by);
  }
  __syncthreads();
}

// Step 4's limit. Reads keys; leaves the count of elements >= bound in
// sh->cnt_b and returns it (one barrier inside).
// Stage 2: the angular list reads the sorted order of every element with
// score >= bound while it still needs near-best ones.
__device__ __forceinline__ int stage2_limit(const double* keys, int n, double bound, FinishShared* sh) {
  int cr = 0;
  for (int i = threadIdx.x; i < n; i += 64 * kWaves) cr += keys[i] >= bound ? 1 : 0;
  cr = wave_sum_i(cr);
  if (lane_id() == 0) atomicAdd(&sh->cnt_b, cr);
  __syncthreads();
  return min(n, sh->cnt_b);  // every element >= bound
}

// Step 5 (wave 0). Reads the sorted keys / vals; leaves o->pos_idx,
// o->pos_score and o->n_pos.
// positional list (:915-928): the sorted prefix with score > bound, <= 20
__device__ __forceinline__ void write_positional(const double* keys, const uint16_t* vals, int n, double bound,
                                                 bool want_pos, FinishOut* o) {
  const int lane = lane_id();
  int npos = 0;
  for (int base = 0; want_pos && base < n && npos < kCovPoints; base += 64) {
    const int p = base + lane;
    const bool ok = p < n && keys[p] > bound;
    const uint64_t m = __ballot(ok);
    const int run = (m == ~0ull) ? 64 : __ffsll((long long)~m) - 1;  // prefix length in chunk
    if (lane < run && npos + lane < kCovPoints) {
      o->pos_idx[npos + lane] = vals[p];
      o->pos_score[npos + lane] = keys[p];
    }
    npos += run;
    if (run < 64) break;
  }
  if (lane == 0) o->n_pos = min(npos, kCovPoints);
}

// Step 6 (wave 0). Reads the sorted keys / vals and the best (bx, by); leaves
// o->ang_idx, o->ang_score and o->n_ang.
// angular list (:990-1003): score >= bound and (x, y) within lin_tol of the best
__device__ __forceinline__ void write_angular(const double* keys, const uint16_t* vals, int n, double bound,
                                              bool want_ang, const CandGrid& g, double bx, double by, double tol,
                                              FinishOut* o) {
  const int lane = lane_id();
  int nang = 0;
  for (int base = 0; want_ang && base < n && nang < kCovPoints; base += 64) {
    const int p = base + lane;
    bool ok = false;
    bool above = false;
    if (p < n) {
      const double s = keys[p];
      above = s >= bound;
      if (above) ok = near_best(g.x(vals[p]), g.y(vals[p]), bx, by, tol);
    }
    const uint64_t m = __ballot(ok);
    const int r = nang + popc(m & below_mask(lane));
    if (ok && r < kCovPoints) {
      o->ang_idx[r] = vals[p];
      o->ang_score[r] = keys[p];
    }
    nang += popc(m);
    if (__ballot(above) != ~0ull) break;  // sorted: nothing later is >= bound
  }
  if (lane == 0) o->n_ang = min(nang, kCovPoints);
}

}  // namespace

// The exact pass over one window (4 waves). Waves 1-3 return before the
// list scans; the caller's barrier joins them. Inlined into finish_kernel
// (as a call it took 211 VGPRs and scratch; inlined 129 and none, r04).
__device__ __forceinline__ void finish_window(const FinishArgs& A, const ScanWork* __restrict__ scans,
                              const AngleEntry* __restrict__ angles, const double* __restrict__ scores,
                              FinishOut* __restrict__ out, const int w, char* smem) {
  const int n = (int)A.n_cand;
  const int wave = threadIdx.x >> 6;
  const FinishLayout Lo = finish_layout(n);
  FinishShared* sh = reinterpret_cast<FinishShared*>(smem);
  double* keys = reinterpret_cast<double*>(smem + Lo.keys);
  uint16_t* vals = reinterpret_cast<uint16_t*>(smem + Lo.vals);
  FinishOut* o = reinterpret_cast<FinishOut*>(smem + Lo.fout);  // stored sealed at the end (emit_sealed)
  Seg* stack = reinterpret_cast<Seg*>(smem + Lo.stack);
  // clang-format off
  LevelSort sort{keys, vals, reinterpret_cast<uint16_t*>(smem + Lo.lpos), reinterpret_cast<uint16_t*>(smem + Lo.rpos),
                 stack, stack + Lo.seg_cap, Lo.seg_cap, reinterpret_cast<Seg*>(smem + Lo.defer), &sh->sort, &sh->part,
                 reinterpret_cast<WaveScratch*>(smem + Lo.wave_scratch) + wave, 0};
  // clang-format on
  int32_t* const tr = &sh->sort.trace;
  CSM_TRACE_CLAIM(tr, n);
  CSM_STAMP(tr, 0);

  load_scores(scores + (int64_t)w * (A.score_stride ? A.score_stride : A.n_cand), n, keys, vals, sh);
  __syncthreads();
  sort.seed(n);
  CSM_STAMP(tr, 2);
  sort.run(stage1_limit(A, sh, n));
  CSM_STAMP(tr, 3);
  CSM_TRACE_VALUE(tr, 8, sort.plim);

  // ---- ordered scans over the sorted candidates -----------------------------
  const ScanWork S = scans[w];
  const CandGrid g{S.x0, S.y0, A.step_cells, A.n_space};
  const double best = keys[0];
  find_best_staged(S, angles, g, keys, vals, n, best, smem + Lo.lpos, Lo.fout - Lo.lpos, o, sh);
  CSM_STAMP(tr, 4);
  const double bound = cov_bound(best);
  const WantLists want = want_lists(A.skip_lists);
  if (want.ang) sort.resume(stage2_limit(keys, n, bound, sh));  // uniform over the block
  CSM_STAMP(tr, 5);
  if (A.order_out)
    for (int i = threadIdx.x; i < n; i += 64 * kWaves) A.order_out[(int64_t)w * n + i] = vals[i];
  if (threadIdx.x == 0 && sh->sort.pad) o->count = -1;
  if (wave != 0) return;

  write_positional(keys, vals, n, bound, want.pos, o);
  write_angular(keys, vals, n, bound, want.ang, g, sh->bx, sh->by, A.lin_tol, o);
  // the LDS FinishOut (thread 0's header, the lanes' list entries) to memory, sealed
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  emit_sealed(A, o, out + w, want.lists, kSealExact, lane_id());
  CSM_STAMP(tr, 6);
}

// scores: window-major, n_cand per window (penalty applied). 4 waves/window.
// With the fast finish's list of flagged windows, a small grid walks the list
// (a block per window of all n_windows cost ~50 us of dispatch at 2048
// windows even though almost every block exits at once).
__device__ __forceinline__ void finish_entry(const FinishArgs& A, const ScanWork* __restrict__ scans,
                                             const AngleEntry* __restrict__ angles, const double* __restrict__ scores,
                                             FinishOut* __restrict__ out, char* smem) {
  if (A.exact_list) {
    // {count, tag} in one load: a pass whose launch's list has been reset by
    // the slot's next scoring launch (another tag) had nothing to do
    const uint64_t head = __hip_atomic_load(reinterpret_cast<uint64_t*>(A.exact_list), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    const int cnt = (uint32_t)(head >> 32) == (uint32_t)A.flag_value ? (int)(uint32_t)head : 0;
    for (int i = blockIdx.x; i < cnt; i += gridDim.x) {
      finish_window(A, scans, angles, scores, out, A.exact_list[2 + i], smem);
      __syncthreads();  // the next window reuses the LDS carve
    }
    // every block's sealed FinishOut stores complete, then the last block
    // signals the host (nothing flagged: the fast pass signalled it)
    if (A.host_flag && cnt > 0) signal_host(A, [] { return true; }, nullptr);
    return;
  }
  const int w = blockIdx.x;
  if (A.need_exact && A.need_exact[w] == 0) return;  // the fast finish settled this window
  finish_window(A, scans, angles, scores, out, w, smem);
}

__global__ __launch_bounds__(64 * kWaves) void finish_kernel(FinishArgs A, const ScanWork* __restrict__ scans,
                                                             const AngleEntry* __restrict__ angles,
                                                             const double* __restrict__ scores,
                                                             FinishOut* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  finish_entry(A, scans, angles, scores, out, smem);
}

hipError_t launch_finish(const FinishArgs& A, const ScanWork* d_scans, const AngleEntry* d_angles,
                         const double* d_scores, FinishOut* d_out, int32_t n_windows, hipStream_t stream,
                         hipStream_t exact_stream, hipEvent_t ev_fast, bool fast_done) {
  const size_t lds = finish_lds_bytes(A.n_cand);
  if (A.n_cand <= 0 || A.n_cand > kFinishMaxCand || lds > 160 * 1024 || n_windows <= 0) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&finish_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const bool listed = A.need_exact && A.exact_list && !A.order_out;
  if (listed && !A.host_flag) {  // with a host signal the scoring launch zeroed the count
    hipError_t e = hipMemsetAsync(A.exact_list, 0, 2 * sizeof(int32_t), stream);  // {count 0, tag 0}
    if (e != hipSuccess) return e;
  }
  if (A.need_exact && !A.order_out && !fast_done) {  // fast pass first; the exact pass only where it flagged
    hipError_t e = launch_fast(A, d_scans, d_angles, d_scores, d_out, n_windows, stream);
    if (e != hipSuccess) return e;
  }
  hipStream_t xs = stream;
  if (exact_stream && exact_stream != stream && A.need_exact && !A.order_out && ev_fast) {
    hipError_t e;
    if ((e = hipEventRecord(ev_fast, stream)) != hipSuccess || (e = hipStreamWaitEvent(exact_stream, ev_fast, 0)) != hipSuccess)
      return e;
    xs = exact_stream;
  }
  FinishArgs B = A;
  if (!A.host_flag) B.flag_value = 0;       // the tag the memset above left
  if (A.order_out) B.need_exact = nullptr;  // the permutation hook always sorts
  if (!listed) B.exact_list = nullptr;
  const dim3 grid(listed ? std::min(n_windows, CSM_EXACT_GRID) : n_windows);
  hipLaunchKernelGGL(finish_kernel, grid, dim3(64 * kWaves), lds, xs, B, d_scans, d_angles, d_scores, d_out);
  return hipGetLastError();
}

}  // namespace csm
