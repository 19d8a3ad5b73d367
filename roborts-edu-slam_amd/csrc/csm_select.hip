// csm_select.hip — the device selection over a collected list (csm_select.hpp).
#include <hip/hip_runtime.h>

#include "csm_select.hpp"

namespace csm {

namespace {

constexpr int kSB = 256;

__device__ __forceinline__ int sel_shift(int pass) {
  const int s = 64 - kSelBits * (pass + 1);
  return s < 0 ? 0 : s;
}
__device__ __forceinline__ int sel_bits(int pass) { return pass + 1 < kSelPasses ? kSelBits : 64 - kSelBits * (kSelPasses - 1); }

// one hit, a 16-byte load
__device__ __forceinline__ PyrHit load_hit(const PyrHit* __restrict__ hits, int64_t i) {
  const ulonglong2 v = reinterpret_cast<const ulonglong2*>(hits)[i];
  return PyrHit{__longlong_as_double((long long)v.x), (int64_t)v.y};
}

__device__ __forceinline__ bool sel_pred(const SelectSpec& sp, const PyrHit& h) {
  if (!sp.near_on) return true;
  const int idx = (int)h.flat;
  return near_best(sp.grid.x(idx), sp.grid.y(idx), sp.bx, sp.by, sp.tol);
}

__device__ __forceinline__ int64_t sel_count(const unsigned long long* __restrict__ n_dev, int64_t cap) {
  const unsigned long long n = *n_dev;
  return n < (unsigned long long)cap ? (int64_t)n : cap;
}

__global__ __launch_bounds__(kSB) void select_init_kernel(SelectState* __restrict__ st, SelectHead* __restrict__ out,
                                                          int32_t k) {
  if (threadIdx.x == 0) {
    st->prefix = 0;
    st->remaining = (unsigned long long)k;
    st->all = 0;
    st->pad = 0;
    out->count = 0;
    out->key = 0;
  }
  for (int i = threadIdx.x; i < kSelBins; i += kSB) st->bins[i] = 0;
}

// The current digit's histogram over the hits that pass pred and match the
// prefix above it.
__global__ __launch_bounds__(kSB) void select_hist_kernel(const PyrHit* __restrict__ hits,
                                                          const unsigned long long* __restrict__ n_dev, int64_t cap,
                                                          SelectSpec sp, SelectState* __restrict__ st, int pass) {
  __shared__ unsigned int h[kSelBins];
  if (st->all) return;  // uniform
  for (int i = threadIdx.x; i < kSelBins; i += kSB) h[i] = 0;
  __syncthreads();
  const int64_t n = sel_count(n_dev, cap);
  const unsigned long long prefix = st->prefix;
  const int shift = sel_shift(pass), bits = sel_bits(pass), hi = shift + bits;
  const unsigned int mask = (1u << bits) - 1u;
  for (int64_t i = (int64_t)blockIdx.x * kSB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSB) {
    const PyrHit x = load_hit(hits, i);
    if (!sel_pred(sp, x)) continue;
    const uint64_t key = select_key(x.score);
    if (hi < 64 && (key >> hi) != (prefix >> hi)) continue;
    atomicAdd(&h[(unsigned int)(key >> shift) & mask], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSelBins; i += kSB) {
    const unsigned int c = h[i];
    if (c) atomicAdd(&st->bins[i], c);
  }
}

// One block: the digit at which the count from the top reaches the remaining
// rank. Thread t owns the 8 bins below kSelBins - 8 t, top down.
__global__ __launch_bounds__(kSB) void select_pick_kernel(SelectState* __restrict__ st, int pass) {
  static_assert(kSelBins == 8 * kSB, "8 bins a thread");
  __shared__ unsigned long long sums[kSB];
  if (st->all) return;  // uniform
  const int t = threadIdx.x;
  const unsigned long long rem = st->remaining, prefix = st->prefix;
  const int top = kSelBins - 1 - 8 * t;
  unsigned int c[8];
  unsigned long long own = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = st->bins[top - j];
    own += c[j];
  }
  sums[t] = own;
  __syncthreads();
  for (int off = 1; off < kSB; off <<= 1) {  // inclusive scan, from the top bins down
    const unsigned long long v = t >= off ? sums[t - off] : 0ull;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  const unsigned long long incl = sums[t], total = sums[kSB - 1];
#pragma unroll
  for (int j = 0; j < 8; ++j) st->bins[top - j] = 0;  // for the next pass
  if (total < rem) {  // fewer than K pass pred (the first pass): the lowest key, every one selected
    if (t == 0) {
      st->all = 1;
      st->prefix = 0;
    }
    return;
  }
  unsigned long long acc = incl - own;
  if (acc < rem && rem <= incl) {  // one thread
    int digit = top;
    unsigned long long before = acc;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool here = !found && acc + c[j] >= rem;
      if (here) {
        digit = top - j;
        before = acc;
        found = true;
      }
      acc += c[j];
    }
    st->prefix = prefix | ((unsigned long long)digit << sel_shift(pass));
    st->remaining = rem - before;
  }
}

__global__ __launch_bounds__(kSB) void select_compact_kernel(const PyrHit* __restrict__ hits,
                                                             const unsigned long long* __restrict__ n_dev, int64_t cap,
                                                             SelectSpec sp, const SelectState* __restrict__ st,
                                                             SelectHead* __restrict__ out, int64_t out_cap) {
  const int64_t n = sel_count(n_dev, cap);
  const uint64_t key_k = st->all ? 0ull : st->prefix;
  if (blockIdx.x == 0 && threadIdx.x == 0) out->key = key_k;
  PyrHit* __restrict__ entries = reinterpret_cast<PyrHit*>(out + 1);
  const int lane = threadIdx.x & 63;
  // the wave's first hit: uniform, so every lane of the wave makes every pass
  for (int64_t base = (int64_t)blockIdx.x * kSB + (threadIdx.x & ~63); base < n; base += (int64_t)gridDim.x * kSB) {
    const int64_t i = base + lane;
    PyrHit x{0.0, 0};
    bool member = false;
    if (i < n) {
      x = load_hit(hits, i);
      member = sel_pred(sp, x) && (select_key(x.score) >= key_k || (sp.band_on && in_response_band(x.score, sp.best)));
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(member);
    if (m == 0) continue;  // uniform
    unsigned long long first = 0;
    if (lane == 0) first = atomicAdd(&out->count, (unsigned long long)__builtin_popcountll(m));
    first = __shfl(first, 0, 64);
    if (member) {
      const int64_t o = (int64_t)first + __builtin_popcountll(m & (((uint64_t)1 << lane) - 1));
      if (o < out_cap) entries[o] = x;
    }
  }
}

int select_blocks(int64_t upper) {
  int64_t b = (upper + kSB - 1) / kSB;
  if (b > kSelMaxBlocks) b = kSelMaxBlocks;
  return (int)(b < 1 ? 1 : b);
}

// A gated search's per-window state before a descent: no flat yet; the keys at
// the lowest key, or kept as the descent before left them (keep_keys).
__global__ __launch_bounds__(kSB) void gate_init_kernel(unsigned long long* __restrict__ wkey,
                                                        long long* __restrict__ wflat, int64_t n_windows,
                                                        int keep_keys) {
  for (int64_t i = (int64_t)blockIdx.x * kSB + threadIdx.x; i < n_windows; i += (int64_t)gridDim.x * kSB) {
    if (!keep_keys) wkey[i] = 0;
    wflat[i] = INT64_MAX;
  }
}

// Over the list's first min(*n_dev, cap) entries: an entry whose key equals
// its window's final key is one of the window's best candidates; the lowest
// flat among them wins (a 64-bit atomicMin, skipped when a plain look at
// wflat[w] already shows a lower one: wflat only falls). Thread 0 also copies
// the descent's counters next to the per-window arrays, so one copy brings
// everything back.
__global__ __launch_bounds__(kSB) void gate_window_best_kernel(const PyrHit* __restrict__ hits,
                                                               const unsigned long long* __restrict__ n_dev,
                                                               int64_t cap, int64_t n_cand,
                                                               const unsigned long long* __restrict__ wkey,
                                                               long long* __restrict__ wflat,
                                                               const unsigned long long* __restrict__ scored,
                                                               GateHead* __restrict__ head) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int d = 0; d < kGateLevels; ++d) head->scored[d] = scored[d];
    head->listed = *n_dev;
  }
  const int64_t n = sel_count(n_dev, cap);
  for (int64_t i = (int64_t)blockIdx.x * kSB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSB) {
    const PyrHit x = load_hit(hits, i);
    const int64_t w = x.flat / n_cand;
    if (select_key(x.score) != wkey[w]) continue;
#if CSM_GATE_MUTATION == 1  // a plain store in place of the atomicMin must fail the tests
    wflat[w] = (long long)x.flat;
#else
    if ((long long)x.flat < __hip_atomic_load(wflat + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(wflat + w, (long long)x.flat);
#endif
  }
}

}  // namespace

hipError_t launch_gate_init(unsigned long long* wkey, long long* wflat, int64_t n_windows, bool keep_keys,
                            hipStream_t stream) {
  if (!wkey || !wflat || n_windows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gate_init_kernel, dim3(select_blocks(n_windows)), dim3(kSB), 0, stream, wkey, wflat, n_windows,
                     keep_keys ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_gate_window_best(const PyrHit* hits, const unsigned long long* n_dev, int64_t cap, int64_t n_cand,
                                   const unsigned long long* wkey, long long* wflat, const unsigned long long* scored,
                                   GateHead* head, hipStream_t stream) {
  if (!hits || !n_dev || !wkey || !wflat || !scored || !head || cap < 1 || n_cand < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gate_window_best_kernel, dim3(select_blocks(cap)), dim3(kSB), 0, stream, hits, n_dev, cap, n_cand,
                     wkey, wflat, scored, head);
  return hipGetLastError();
}

hipError_t launch_list_select(const PyrHit* hits, const unsigned long long* n_dev, int64_t cap, int64_t upper,
                              const SelectSpec& spec, SelectState* state, SelectHead* out, int64_t out_cap,
                              hipStream_t stream, int* launches) {
  if (!hits || !n_dev || !state || !out || cap < 0 || out_cap < 0 || spec.k < 1) return hipErrorInvalidValue;
  const int nb = select_blocks(upper < cap ? upper : cap);
  hipError_t e;
  int nl = 0;
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(kSB), 0, stream, state, out, spec.k);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  ++nl;
  for (int pass = 0; pass < kSelPasses; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(nb), dim3(kSB), 0, stream, hits, n_dev, cap, spec, state, pass);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(kSB), 0, stream, state, pass);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    nl += 2;
  }
  hipLaunchKernelGGL(select_compact_kernel, dim3(nb), dim3(kSB), 0, stream, hits, n_dev, cap, spec,
                     (const SelectState*)state, out, out_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  ++nl;
  if (launches) *launches = nl;
  return hipSuccess;
}

}  // namespace csm
