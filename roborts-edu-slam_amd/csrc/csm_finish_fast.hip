// csm_finish_fast.hip — the fast finish: no sort when no tie can matter.
// Everything the sorted candidates feed is decided by the elements with
// score >= bound = min(best - 0.1, 0.5) (:912,:986; FindBestCandidate's
// prefix, s >= best - 0.01, lies above it): the FindBest prefix (all of it, in
// sorted order: its sums are order-dependent), the first 20 with score > bound
// (:915-928) and the first 20 near the best with score >= bound (:990-1003).
// std::sort leaves distinct scores in strictly decreasing order, so if none of
// the scores these read repeats (nor the value just past a list's 20th), they
// are fixed by value alone:
//   1. max, NaN check; counts above eight thresholds best - delta;
//   2. the smallest threshold holding 20 elements > bound (or all of them):
//      compacted (<= kFastCap), ranked by value in LDS (rank = elements
//      greater), which gives the prefix and the positional list;
//   3. FindBest's sums -> (bx, by); the near-best elements >= bound compacted
//      (<= kFastNearCap) and ranked the same way for the angular list.
// A repeat where order decides, a NaN or an oversized set flags the window
// for finish_kernel's exact std::sort emulation, which runs next and skips
// every other window. One block of T threads per window; each thread holds
// its V = ceil(n / T) scores in registers (loaded once, all in flight: the
// passes re-reading the scores from L2 were latency-bound, one round trip per
// 256 candidates per pass), and the window's angle rows sit in LDS for the
// sequential FindBest sums. T = 1024 for launches of few windows (the
// reference's single-scan levels), 256 otherwise.
#define CSM_TRACE_UNIT_FAST
#include <hip/hip_runtime.h>

#include <cstddef>

#include "csm_device.hpp"
#include "csm_finish_trace.hpp"
#include "csm_internal.hpp"
#include "csm_tail.hpp"

#pragma clang fp contract(off)

namespace csm {

using namespace dev;

constexpr int kFastCap = 512;      // compacted candidates of step 2
constexpr int kFastNearCap = 512;  // compacted near-best candidates of step 3
constexpr int kFastAngles = 256;   // angle rows staged in LDS (more: read from memory)

// Host signal (A.host_flag): every block's FinishOut stores complete (write-
// through sc0 sc1 stores to the coherent host buffer, each wave waits for
// them), the blocks count in; the last one, if no window was flagged for the
// exact pass, stores the flag value itself -- the exact launch behind it then
// returns at once and is off the host's critical path. The count-in is
// relaxed: the host reads every window through its seal, so a flag seen
// before a window's stores costs a spin, never a wrong result (DESIGN §7
// "Host signals"; a per-block system-scope release, one L2 write-back per
// block, cost 25-50 us per launch).
__device__ __forceinline__ void fast_signal(const FinishArgs& A) {
  // flag() counts with device-scope atomics before each block's add; with
  // host_fast_flag every header is in: settled windows complete now
  auto none_flagged = [&] { return __hip_atomic_load(A.exact_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0; };
  signal_host(A, none_flagged, A.host_fast_flag);
}

template <int T, int V>
__device__ __forceinline__ void finish_fast_body(const FinishArgs& A, const ScanWork* __restrict__ scans,
                                                 const AngleEntry* __restrict__ angles,
                                                 const double* __restrict__ scores, FinishOut* __restrict__ out);

template <int T, int V>
__global__ __launch_bounds__(T) void finish_fast_kernel(FinishArgs A, const ScanWork* __restrict__ scans,
                                                        const AngleEntry* __restrict__ angles,
                                                        const double* __restrict__ scores,
                                                        FinishOut* __restrict__ out) {
  CSM_TS_MIN(16);
  CSM_FASTBLK_BEGIN();
  finish_fast_body<T, V>(A, scans, angles, scores, out);
  CSM_TS_MAX(24);  // body done
  if (A.host_flag) fast_signal(A);
  CSM_TS_MAX(25);  // signalled
  CSM_FASTBLK_END();
}

template <int T, int V>
__device__ __forceinline__ void finish_fast_body(const FinishArgs& A, const ScanWork* __restrict__ scans,
                                                 const AngleEntry* __restrict__ angles,
                                                 const double* __restrict__ scores, FinishOut* __restrict__ out) {
  constexpr int NW = T / 64;
  // LDS lists sized to what the instantiation can hold (n <= V * T): a block
  // of the 189- and 1331-candidate levels then fits 8 to a CU, so a part's
  // 2048 windows take one round of blocks, not two (23.2 KB of LDS a block
  // allowed 7). The caps only decide when the exact pass takes a window.
  constexpr int CAP = V * T < kFastCap ? V * T : kFastCap;
  constexpr int NCAP = V * T < kFastNearCap ? V * T : kFastNearCap;
  constexpr int ACAP = T == 128 ? 64 : (V * T < kFastAngles ? V * T : kFastAngles);
  __shared__ __attribute__((aligned(16))) double ck[CAP + 4];  // step 2 candidates (value, index), then ...
  __shared__ int ci[CAP];
  __shared__ double sk[CAP];   // ... sorted by value (rank order)
  __shared__ int si[CAP];
  __shared__ __attribute__((aligned(16))) double nk[NCAP + 4];
  __shared__ int ni[NCAP];
  __shared__ double acs[ACAP], asn[ACAP];
  __shared__ double red[NW];
  __shared__ int cnt_s[kFinishLevels];
  __shared__ int nC_s, nN_s, flag_s;
  __shared__ double sbx, sby;
  // FinishOut is assembled in LDS and stored once at the end (34 16-byte
  // stores): written field by field it was dozens of scattered stores, to
  // pinned host memory on the few-window path, each barrier after them
  // waiting for their completions.
  __shared__ __attribute__((aligned(16))) FinishOut so;
  const int w = blockIdx.x;
  const int n = (int)A.n_cand;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* sc = scores + (int64_t)w * (A.score_stride ? A.score_stride : A.n_cand);
  int32_t* need = A.need_exact + w;
  auto flag = [&]() {  // thread 0: the exact pass takes this window
    *need = 1;
    if (A.exact_list) A.exact_list[2 + atomicAdd(A.exact_list, 1)] = w;
    if (A.host_fast_flag) store_pending_seal(A, out + w);  // the exact pass owes it
  };
  // the scores, every load in flight (index clamped, value masked after)
  double v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int i = tid + k * T;
    const double x = sc[min(i, n - 1)];
    v[k] = i < n ? x : -INFINITY;
  }
  const ScanWork S = scans[w];
  const int ns = A.n_space;
  const int nss = ns * ns;
  CSM_TS_MAX(17);  // score loads issued
  {
    const int na = min(n / nss, ACAP);
    for (int t = tid; t < na; t += T) {
      const AngleEntry ae = angles[S.angle_off + t];
      acs[t] = ae.cosine;
      asn[t] = ae.sine;
    }
  }
  if (tid < kFinishLevels) cnt_s[tid] = 0;
  if (tid == 0) {
    nC_s = 0;
    nN_s = 0;
    flag_s = 0;
  }

  // 1. best = the front of the sorted candidates (:607); NaN anywhere: exact path
  double m = -INFINITY;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    nan |= (v[k] != v[k]);
    m = (v[k] > m) ? v[k] : m;
  }
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  if (__ballot(nan) != 0 && lane == 0) flag_s = 1;
  __syncthreads();
  double best = red[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) best = fmax(best, red[q]);
  CSM_TS_MAX(18);  // max reduced
  if (flag_s || n <= 0) {
    if (tid == 0) flag();
    return;
  }
  const double bound = cov_bound(best);
  int lv[V];
  {
    // per-lane counts (LevelCounts; a wave counts at most 64 * V < 2^16 per
    // level), added across the wave in two 64-bit words: vector work only.
    // (Per-level ballots and scalar popcounts kept the CU's one scalar unit
    // busy for every wave: ~4.6 us of a coarse window's block,
    // tools/fast_blocks.py.)
    static_assert(64 * V < 65536, "16-bit level counts");
    LevelCounts lc;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      lv[k] = level_of(v[k], best, bound);  // -INFINITY padding: no level
      lc.add(lv[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lc.c0 += __shfl_xor(lc.c0, o, 64);
      lc.c1 += __shfl_xor(lc.c1, o, 64);
    }
    if (lane < kFinishLevels) {
      const int t = lc.level(lane);
      if (t) atomicAdd(&cnt_s[lane], t);
    }
  }
  __syncthreads();
  CSM_TS_MAX(19);  // level counts
  // 2. the level select_level picks, its scores compacted
  const WantLists want = want_lists(A.skip_lists);
  const bool want_pos = want.pos, want_ang = want.ang;
  int L, nC;
  select_level(cnt_s, want_pos, &L, &nC);
  if (nC > CAP) {
    if (tid == 0) flag();
    return;
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int i = tid + k * T;
    const bool in = lv[k] <= L;  // padding never qualifies
    const uint64_t mm = __ballot(in);
    if (mm) {  // wave-uniform
      int base = 0;
      if (lane == 0) base = atomicAdd(&nC_s, popc(mm));
      base = uni(base);
      if (in) {
        const int p = ballot_slot(base, mm, lane);
        ck[p] = v[k];
        ci[p] = i;
      }
    }
  }
  if (tid < 4 && nC + tid < CAP + 4) ck[nC + tid] = -INFINITY;  // the rank loop's padding (nC known)
  __syncthreads();
  // rank = elements greater; any equal value where the order decides: exact
  // path (the prefix, the positional 20 and the value just past them)
  // (ck padded with -inf to a multiple of 4: read 4 at a time, 2 LDS loads)
  for (int t = tid; t < nC; t += T) {
    const double x = ck[t];
    int r, eq;
    rank_among(ck, nC, x, &r, &eq);
    if (tie_matters_positional(eq, r, in_response_band(x, best), want_pos)) flag_s = 1;
    sk[r] = x;  // distinct ranks whenever nothing is flagged
    si[r] = ci[t];
  }
  __syncthreads();
  CSM_TS_MAX(20);  // compacted and ranked
  if (flag_s) {
    if (tid == 0) flag();
    return;
  }
  const CandGrid g{S.x0, S.y0, A.step_cells, ns};
  FinishOut* const o = &so;
  // Only the pieces the host reads are stored: the header, plus the lists the
  // level keeps (skip_lists) -- 64 B per window instead of 544 B on a level
  // whose lists are dead, the bytes that cross to host memory with a host signal.
  auto emit = [&]() {  // all threads: the LDS FinishOut and its seal to out[w]
    __syncthreads();
    if (wave == 0) emit_sealed(A, &so, out + w, want.lists, kSealFast, lane);
  };
  if (tid == 0) {
    auto cos_sin = [&](int a) {  // the staged rows, memory past them
      return CosSin{a < ACAP ? acs[a] : angles[S.angle_off + a].cosine,
                    a < ACAP ? asn[a] : angles[S.angle_off + a].sine};
    };
    find_best(sk, si, nC, best, g, cos_sin, o, &sbx, &sby);
    o->n_pos = want_pos ? min(nC, kCovPoints) : 0;
  }
  // positional list (:915-928): the sorted prefix with score > bound, <= 20
  if (want_pos && tid < min(nC, kCovPoints)) {
    o->pos_idx[tid] = si[tid];
    o->pos_score[tid] = sk[tid];
  }
  __syncthreads();
  CSM_TS_MAX(21);  // prefix sums and positional list
  // 3. angular list (:990-1003): near the best, score >= bound
  if (!want_ang) {
    if (tid == 0) o->n_ang = 0;
    emit();
    if (tid == 0) *need = 0;
    return;
  }
  const double bx = sbx, by = sby, tol = A.lin_tol;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int i = tid + k * T;
    const double s = v[k];
    bool in = false;
    if (s >= bound) in = near_best(g.x(i), g.y(i), bx, by, tol);  // padding (-inf) never qualifies
    const uint64_t mm = __ballot(in);
    if (mm) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&nN_s, popc(mm));
      base = uni(base);
      if (in) {
        const int p = ballot_slot(base, mm, lane);
        if (p < NCAP) {
          nk[p] = s;
          ni[p] = i;
        }
      }
    }
  }
  __syncthreads();
  CSM_TS_MAX(22);  // near-best compacted
  const int nN = nN_s;
  if (nN > NCAP) {
    if (tid == 0) flag();
    return;
  }
  if (tid < 4) nk[nN + tid] = -INFINITY;  // the rank loop's padding
  __syncthreads();
  for (int t = tid; t < nN; t += T) {
    const double x = nk[t];
    int r, eq;
    rank_among(nk, nN, x, &r, &eq);  // (nk padded with -inf like ck)
    if (tie_matters_angular(eq, r)) flag_s = 1;
    if (r < kCovPoints) {
      o->ang_idx[r] = ni[t];
      o->ang_score[r] = x;
    }
  }
  __syncthreads();
  CSM_TS_MAX(23);  // near-best ranked
  if (tid == 0) o->n_ang = min(nN, kCovPoints);
  if (flag_s) {  // (flag_s is read after the barrier above: uniform)
    if (tid == 0) flag();
    return;
  }
  emit();
  if (tid == 0) *need = 0;
}

// Scores per thread of the fast finish's instantiations: the smallest V with
// V * T >= n (n <= kFinishMaxCand = 10240).
template <int T, int V>
hipError_t launch_fast_tv(const FinishArgs& A, const ScanWork* s, const AngleEntry* a, const double* sc,
                          FinishOut* o, int32_t nw, hipStream_t stream) {
  hipLaunchKernelGGL((finish_fast_kernel<T, V>), dim3(nw), dim3(T), 0, stream, A, s, a, sc, o);
  return hipGetLastError();
}

hipError_t launch_fast(const FinishArgs& A, const ScanWork* s, const AngleEntry* a, const double* sc, FinishOut* o,
                       int32_t nw, hipStream_t stream) {
  const int64_t n = A.n_cand;
  if (nw <= (A.wide_windows ? A.wide_windows : kFinishWideWindows)) {  // few windows: 16 waves per window
    if (n <= 1024) return launch_fast_tv<1024, 1>(A, s, a, sc, o, nw, stream);
    if (n <= 2048) return launch_fast_tv<1024, 2>(A, s, a, sc, o, nw, stream);
    if (n <= 4096) return launch_fast_tv<1024, 4>(A, s, a, sc, o, nw, stream);
    if (n <= 6144) return launch_fast_tv<1024, 6>(A, s, a, sc, o, nw, stream);
    return launch_fast_tv<1024, 10>(A, s, a, sc, o, nw, stream);
  }
  if (n <= 256) return launch_fast_tv<256, 1>(A, s, a, sc, o, nw, stream);
  if (n <= 512) return launch_fast_tv<256, 2>(A, s, a, sc, o, nw, stream);
  if (n <= 1024) return launch_fast_tv<256, 4>(A, s, a, sc, o, nw, stream);
  // two waves a window (20 KB of LDS, ~80 VGPRs): 8 blocks a CU, where
  // <256, 6> held 7 (66 VGPRs, 23.2 KB)
  if (n <= 1408) return launch_fast_tv<128, 11>(A, s, a, sc, o, nw, stream);
  if (n <= 1536) return launch_fast_tv<256, 6>(A, s, a, sc, o, nw, stream);
  if (n <= 2560) return launch_fast_tv<256, 10>(A, s, a, sc, o, nw, stream);
  if (n <= 5120) return launch_fast_tv<256, 20>(A, s, a, sc, o, nw, stream);
  return launch_fast_tv<256, 40>(A, s, a, sc, o, nw, stream);
}

}  // namespace csm
