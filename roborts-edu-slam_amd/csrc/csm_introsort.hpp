// csm_introsort.hpp — a device emulation of libstdc++'s std::sort(greater) over
// (key f64, value u16) pairs in LDS, for the exact finish (csm_finish.hip).
//
// Why an emulation and not a GPU sort: the winner among exactly tied scores,
// the averaged best pose and both covariances depend on the order std::sort
// leaves tied candidates in, and real grids tie constantly (sub-cell window
// steps land many candidates on the same cells). libstdc++'s std::sort is
// deterministic given the comparison outcomes:
//   introsort loop (threshold 16, depth limit 2*floor(log2 n)); pivot = median
//   of (first+1, mid, last-1) swapped to first; unguarded Hoare partition;
//   heap sort at depth 0; final insertion sort.
// Segments left by the loop are ordered relative to each other (left >= pivot
// >= right), so the final insertion sort equals an independent stable sort of
// each leaf segment, and segments can be processed in any order. The unguarded
// partition is computed in parallel: with l_k the k-th position (ascending)
// whose key is not > pivot and r_k the k-th position (descending) whose key is
// not < pivot, the sequential loop swaps exactly the pairs (l_k, r_k) with
// l_k < r_k and returns cut = min(l_{p+1}, r_p) for p such pairs.
// The formulation is validated against libstdc++ in tests/wave_sort_model.py.
//
// Layout: one 4-wave workgroup per window, segments in per-level LDS lists. A
// segment of more than 64 elements is partitioned by one wave in LDS; a segment of at most 64 is
// loaded into registers (lane = element) and finished there: its whole
// introsort recursion (ballot / bpermute partitions) and the stable sort of
// its leaves, then written back once.
#pragma once

#include <hip/hip_runtime.h>

#include "csm_device.hpp"
#include "csm_finish_trace.hpp"
#include "csm_internal.hpp"

#pragma clang fp contract(off)

namespace csm {
namespace introsort {

using namespace dev;

// Waves per window of the exact path. Segments are handed out level by level
// with barriers in between (an earlier version pulled them from a spin-locked
// LDS stack and, rarely, spun past its iteration bound).
constexpr int kWaves = kFinishWaves;

__device__ __forceinline__ bool gt(double a, double b) { return a > b; }  // comp = greater

__device__ __forceinline__ void swap_kv(double* k, uint16_t* v, int a, int b) {
  const double tk = k[a];
  k[a] = k[b];
  k[b] = tk;
  const uint16_t tv = v[a];
  v[a] = v[b];
  v[b] = tv;
}

// std::__move_median_to_first(result, a, b, c) — lane 0 only.
static __device__ void move_median_to_first(double* k, uint16_t* v, int result, int a, int b, int c) {
  if (gt(k[a], k[b])) {
    if (gt(k[b], k[c])) swap_kv(k, v, result, b);
    else if (gt(k[a], k[c])) swap_kv(k, v, result, c);
    else swap_kv(k, v, result, a);
  } else if (gt(k[a], k[c])) swap_kv(k, v, result, a);
  else if (gt(k[b], k[c])) swap_kv(k, v, result, c);
  else swap_kv(k, v, result, b);
}

// std::__adjust_heap / __push_heap / heap sort of [first, last) — one lane.
static __device__ void adjust_heap(double* k, uint16_t* v, int base, int hole, int len, double vk, uint16_t vv) {
  const int top = hole;
  int second = hole;
  while (second < (len - 1) / 2) {
    second = 2 * (second + 1);
    if (gt(k[base + second], k[base + second - 1])) second--;
    k[base + hole] = k[base + second];
    v[base + hole] = v[base + second];
    hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) {
    second = 2 * (second + 1);
    k[base + hole] = k[base + second - 1];
    v[base + hole] = v[base + second - 1];
    hole = second - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && gt(k[base + parent], vk)) {
    k[base + hole] = k[base + parent];
    v[base + hole] = v[base + parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  k[base + hole] = vk;
  v[base + hole] = vv;
}

static __device__ void heap_sort(double* k, uint16_t* v, int first, int last) {
  const int len = last - first;
  if (len >= 2) {
    for (int parent = (len - 2) / 2;; --parent) {
      adjust_heap(k, v, first, parent, len, k[first + parent], v[first + parent]);
      if (parent == 0) break;
    }
  }
  while (last - first > 1) {
    --last;
    const double vk = k[last];
    const uint16_t vv = v[last];
    k[last] = k[first];
    v[last] = v[first];
    adjust_heap(k, v, first, 0, last - first, vk, vv);
  }
}

// ---- large segments: one wave, LDS -------------------------------------------
// Parallel std::__unguarded_partition(first+1, last, pivot=first). lpos/rpos
// are the window-sized scratch arrays; this segment uses [first, last). One
// pass ranks both stop kinds from the left: lpos[k] = the k-th left stop
// (l_k), rposl[g] = the g-th right stop from the LEFT, so the k-th from the
// right is r_k = rposl[totR + 1 - k] (no counting pass for totR first).
// Every pass takes kU chunks of 64 per iteration, their LDS reads issued
// together (one wave works a segment alone: nothing else hides the latency);
// ranks are still assigned chunk by chunk in order.
constexpr int kU = 4;
static __device__ int partition_lds(double* k, uint16_t* v, uint16_t* lpos_all, uint16_t* rpos_all,
                             int first, int last) {
  const int lane = lane_id();
  const int m = last - first;
  const int cap = m / 2 + 2;  // pairs <= m/2; ranks up to pairs + 1 are read
  uint16_t* lpos = lpos_all + first - 1;   // ranks are 1-based
  uint16_t* rposl = rpos_all + first - 1;  // right stops, ranked from the left
  const double P = k[first];
  int cntL = 0, cntR = 0;
  for (int base = first + 1; base < last; base += 64 * kU) {
    double key[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int p = base + 64 * u + lane;
      key[u] = p < last ? k[p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int p = base + 64 * u + lane;
      const bool ok = p < last;
      const bool isL = ok && !gt(key[u], P);
      const bool isR = ok && !gt(P, key[u]);
      const uint64_t mL = __ballot(isL), mR = __ballot(isR);
      const int rl = cntL + popc(mL & below_mask(lane)) + 1;
      const int rr = cntR + popc(mR & below_mask(lane)) + 1;
      if (isL) lpos[rl] = (uint16_t)p;
      if (isR) rposl[rr] = (uint16_t)p;
      cntL += popc(mL);
      cntR += popc(mR);
    }
  }
  const int totL = cntL, totR = cntR;
  const int kmax = min(min(totL, totR), cap);
  // the pairs (l_k < r_k) are a prefix of the ranks: l_k rises, r_k falls
  int npairs = 0;
  bool open = true;
  for (int kb = 1; open && kb <= kmax; kb += 64 * kU) {
    int lp[kU], rp[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kk = kb + 64 * u + lane;
      lp[u] = kk <= kmax ? (int)lpos[kk] : 0;
      rp[u] = kk <= kmax ? (int)rposl[totR + 1 - kk] : 0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kk = kb + 64 * u + lane;
      const uint64_t mk = __ballot(kk <= kmax && lp[u] < rp[u]);
      if (open) npairs += popc(mk);
      open = open && mk == ~0ull;
    }
  }
  int cut = INT32_MAX;
  if (npairs + 1 <= totL) cut = lpos[npairs + 1];
  if (npairs >= 1) cut = min(cut, (int)rposl[totR + 1 - npairs]);
  // the swapped positions are all distinct: the kU chunks' swaps are independent
  for (int kb = 1; kb <= npairs; kb += 64 * kU) {
    int lp[kU], rp[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kk = kb + 64 * u + lane;
      lp[u] = kk <= npairs ? (int)lpos[kk] : -1;
      rp[u] = kk <= npairs ? (int)rposl[totR + 1 - kk] : -1;
    }
    double kl[kU], kr[kU];
    uint16_t vl[kU], vr[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (lp[u] >= 0) {
        kl[u] = k[lp[u]];
        kr[u] = k[rp[u]];
        vl[u] = v[lp[u]];
        vr[u] = v[rp[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (lp[u] >= 0) {
        k[lp[u]] = kr[u];
        k[rp[u]] = kl[u];
        v[lp[u]] = vr[u];
        v[rp[u]] = vl[u];
      }
    }
  }
  return uni(cut);
}

// The same partition by the whole 4-wave block, for a level holding one
// large segment (the partial sort's chain down to the prefix): each wave
// ranks both stop kinds of a contiguous quarter from the quarter's left, into
// the quarter's own part of the scratch (one pass); after one barrier the
// global rank k maps to (the wave holding it, its local rank) through the
// waves' counts. The pairs, the cut and the swaps are the single-wave pass's.
constexpr int kCoopMin = 256;
static __device__ int partition_block(double* k, uint16_t* v, uint16_t* lpos_all, uint16_t* rpos_all, int first,
                               int last, BlockPartition* bp, int wave) {
  const int lane = lane_id();
  const int m = last - first;
  const int cap = m / 2 + 2;
  if (threadIdx.x == 0) {
    move_median_to_first(k, v, first, first + 1, first + m / 2, last - 1);
    bp->fail = INT32_MAX;
  }
  __syncthreads();
  const double P = k[first];
  const int cq = ((m - 1 + 63) / 64 + kWaves - 1) / kWaves;  // 64-chunks per quarter
  auto q_lo = [&](int w) { return min(first + 1 + w * cq * 64, last); };
  const int q0 = q_lo(wave), q1 = q_lo(wave + 1);
  int cL = 0, cR = 0;  // local ranks: wave w's j-th left stop at lpos_all[q0 - 1 + j]
  for (int base = q0; base < q1; base += 64 * kU) {
    double key[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int p = base + 64 * u + lane;
      key[u] = p < q1 ? k[p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int p = base + 64 * u + lane;
      const bool ok = p < q1;
      const bool isL = ok && !gt(key[u], P);
      const bool isR = ok && !gt(P, key[u]);
      const uint64_t mL = __ballot(isL), mR = __ballot(isR);
      const int rl = cL + popc(mL & below_mask(lane)) + 1;
      const int rr = cR + popc(mR & below_mask(lane)) + 1;
      if (isL) lpos_all[q0 - 1 + rl] = (uint16_t)p;
      if (isR) rpos_all[q0 - 1 + rr] = (uint16_t)p;
      cL += popc(mL);
      cR += popc(mR);
    }
  }
  if (lane == 0) {
    bp->wl[wave] = cL;
    bp->wr[wave] = cR;
  }
  __syncthreads();
  int offL[kWaves + 1], offR[kWaves + 1];  // counts of the earlier quarters
  offL[0] = offR[0] = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    offL[w + 1] = offL[w] + bp->wl[w];
    offR[w + 1] = offR[w] + bp->wr[w];
  }
  const int totL = offL[kWaves], totR = offR[kWaves];
  auto lpos = [&](int kk) -> int {  // l_k, kk in [1, totL]
    int w = 0;
#pragma unroll
    for (int t = 1; t < kWaves; ++t) w += kk > offL[t] ? 1 : 0;
    return lpos_all[q_lo(w) - 1 + (kk - offL[w])];
  };
  auto rpos = [&](int kk) -> int {  // r_k: the (totR + 1 - k)-th right stop from the left
    const int g = totR + 1 - kk;
    int w = 0;
#pragma unroll
    for (int t = 1; t < kWaves; ++t) w += g > offR[t] ? 1 : 0;
    return rpos_all[q_lo(w) - 1 + (g - offR[w])];
  };
  const int kmax = min(min(totL, totR), cap);
  for (int kk = 1 + (int)threadIdx.x; kk <= kmax; kk += 64 * kWaves)
    if (!(lpos(kk) < rpos(kk))) {  // ranks past the pairs fail from here on
      atomicMin(&bp->fail, kk);
      break;
    }
  __syncthreads();
  const int f = bp->fail;
  const int npairs = f == INT32_MAX ? kmax : f - 1;
  int cut = INT32_MAX;
  if (npairs + 1 <= totL) cut = lpos(npairs + 1);
  if (npairs >= 1) cut = min(cut, rpos(npairs));
  __syncthreads();  // every thread read the cut before the swaps move elements
  for (int kk = 1 + (int)threadIdx.x; kk <= npairs; kk += 64 * kWaves) swap_kv(k, v, lpos(kk), rpos(kk));
  __syncthreads();
  return cut;
}

// ---- small segments: one wave, registers ----------------------------------------
// Finishes [base, base+m), m <= 64, entirely: introsort recursion from depth
// `depth`, heap sort where a sub-segment runs out of depth, stable sort of the
// leaves, one write back.
static __device__ void sort_small(double* keys, uint16_t* vals, int base, int m, int depth, WaveScratch* ws) {
  const int lane = lane_id();
  double k = lane < m ? keys[base + lane] : 0.0;
  int v = lane < m ? (int)vals[base + lane] : 0;
  uint64_t starts = 1ull;   // starts of final segments (relative)
  uint64_t heaped = 0ull;   // lanes of heap-sorted sub-segments (already ordered)
  int sp = 0;
  if (lane == 0) ws->st[0] = Seg{0, m, depth};
  sp = 1;
  while (sp > 0) {
    --sp;
    const Seg s = ws->st[sp];
    const int f = uni(s.first), l = uni(s.last), d = uni(s.depth);
    const int len = l - f;
    if (len <= 16) {
      starts |= 1ull << f;
      continue;
    }
    if (d == 0) {  // std::__partial_sort(first, last, last): heap sort on one lane
      if (lane < m) {
        keys[base + lane] = k;
        vals[base + lane] = (uint16_t)v;
      }
      if (lane == 0) heap_sort(keys, vals, base + f, base + l);
      if (lane < m) {
        k = keys[base + lane];
        v = vals[base + lane];
      }
      starts |= 1ull << f;
      const uint64_t seg = ((l == 64) ? ~0ull : ((1ull << l) - 1)) & ~((1ull << f) - 1);
      heaped |= seg;
      continue;
    }
    // __move_median_to_first(f, f+1, mid, l-1)
    const int a = f + 1, b = f + len / 2, c = l - 1;
    const double ka = bcast_lane(k, a), kb = bcast_lane(k, b), kc = bcast_lane(k, c);
    int sel;
    if (gt(ka, kb)) sel = gt(kb, kc) ? b : (gt(ka, kc) ? c : a);
    else sel = gt(ka, kc) ? a : (gt(kb, kc) ? c : b);
    const double kf = bcast_lane(k, f), ks = bcast_lane(k, sel);
    const int vf = read_lane_i(v, f), vs = read_lane_i(v, sel);
    if (lane == f) {
      k = ks;
      v = vs;
    } else if (lane == sel) {
      k = kf;
      v = vf;
    }
    const double P = ks;
    const bool inr = lane > f && lane < l;
    const bool isL = inr && !gt(k, P);
    const bool isR = inr && !gt(P, k);
    const uint64_t mL = __ballot(isL), mR = __ballot(isR);
    const int totL = popc(mL), totR = popc(mR);
    const int rL = popc(mL & below_mask(lane)) + 1;  // rank ascending
    const int rR = popc(mR & above_mask(lane)) + 1;  // rank from the right
    if (isR) ws->T[rR] = (uint8_t)lane;
    if (isL) ws->U[rL] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int pL = (isL && rL <= totR) ? (int)ws->T[rL] : -1;
    const int pR = (isR && rR <= totL) ? (int)ws->U[rR] : 64;
    const bool swL = isL && pL > lane;   // l_k < r_k
    const bool swR = isR && pR < lane;
    const int npairs = popc(__ballot(swL));
    int cut = INT32_MAX;
    if (npairs + 1 <= totL) cut = ws->U[npairs + 1];
    if (npairs >= 1) cut = min(cut, (int)ws->T[npairs]);
    cut = uni(cut);
    const int src = swL ? pL : (swR ? pR : lane);
    k = __shfl(k, src, 64);
    v = __shfl(v, src, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane == 0) {
      ws->st[sp] = Seg{cut, l, d - 1};
      ws->st[sp + 1] = Seg{f, cut, d - 1};
    }
    sp += 2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  // stable sort of each leaf (the final insertion sort restricted to it)
  const uint64_t bnd = starts | ((m == 64) ? 0ull : (1ull << m));
  const uint64_t le_mask = bnd & above_mask(lane);
  const int le = le_mask ? __builtin_ctzll(le_mask) : 64;
  const uint64_t ls_mask = bnd & (below_mask(lane) | (1ull << lane));
  const int ls = 63 - __builtin_clzll(ls_mask ? ls_mask : 1ull);
  const bool active = lane < m && !((heaped >> lane) & 1ull);
  int rank = 0;
  for (int t = 0; t < 16; ++t) {  // every lane shuffles: sources must be active lanes
    const int j = ls + t;
    const bool okj = active && j < le;
    const double kj = __shfl(k, okj ? j : lane, 64);
    if (okj) rank += (gt(kj, k) || (kj == k && j < lane)) ? 1 : 0;
  }
  const int dest = active ? ls + rank : lane;
  if (lane < m) {
    keys[base + dest] = k;
    vals[base + dest] = (uint16_t)v;
  }
}

// ---- the level-synchronous driver --------------------------------------------
// Level-synchronous introsort: every segment of a level is independent, so
// the waves take them round-robin, children go to the next level's list
// (LDS atomic add, no lock), a barrier separates levels. Depth decreases at
// every partition, so there are at most 2*floor(log2 n) + 2 levels.
// Partial: a segment starting at or past the limit is set aside (positions
// past the limit are never read, and no element crosses a segment boundary
// afterwards), kept for a later resume() in the deferred list.
//
// The contract the finish relies on: after run(p), positions [0, p) of keys /
// vals hold exactly what std::sort(greater) of the whole array leaves there;
// resume(p2) extends that to [0, max(p, p2)). After a list overflow ("cannot
// happen") c->pad is set, the runs stop early, and the caller reports
// count = -1. Every thread of the kWaves-wave block calls seed / run / resume
// with the same arguments; the struct is a per-thread copy of the pointers.
struct LevelSort {
  double* keys;
  uint16_t *vals, *lpos, *rpos;  // lpos, rpos: partition scratch, n each
  Seg *cur, *nxt;                // this level's segments, the next level's
  int cap;                       // ... each list's capacity
  Seg* deferred;                 // kFinishDefer segments set aside
  SortCounters* c;
  BlockPartition* bp;
  WaveScratch* ws;               // this wave's
  int plim;                      // the limit of the current run

  // A segment goes to the next level's list, or straight to the
  // deferred list when it starts at or past the limit: a level then holds only
  // the segments that are partitioned, so the partial sort's chain (one live
  // segment per level) takes the whole block's partition_block, not one wave.
  __device__ __forceinline__ void push(const Seg& s) const {  // one lane
    if (s.first >= plim) {
      const int at = atomicAdd(&c->ndef, 1);
      if (at < kFinishDefer) deferred[at] = s;
      else c->pad = 1;  // cannot happen: at most one straddling segment per level
    } else {
      const int at = atomicAdd(&c->pending, 1);
      if (at < cap) nxt[at] = s;
      else c->pad = 1;  // list overflow: cannot happen for the layout's capacity
    }
  }

  // One segment [0, n), depth 2*floor(log2 n), nothing deferred.
  __device__ __forceinline__ void seed(int n) {
    if (threadIdx.x == 0) {
      int lg = 0;
      while ((2 << lg) <= n) ++lg;  // floor(log2 n)
      cur[0] = Seg{0, n, 2 * lg};
      c->top = 1;      // segments in cur
      c->pending = 0;  // segments appended to nxt
      c->ndef = 0;
      c->pad = 0;
    }
  }

  // Sorts until every segment that starts below `limit` is final.
  __device__ __forceinline__ void run(int limit) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    plim = limit;
    __syncthreads();  // thread 0's seeding
    for (int level = 0;; ++level) {
      const int ncur = c->top;
      CSM_STAMP_LEVEL(&c->trace, level, ncur, ncur > 0 ? cur[0].last - cur[0].first : 0);
      if (ncur == 0) break;
      if (level > 64) {  // cannot happen (depth bound); reported as count = -1
        if (threadIdx.x == 0) c->pad = 1;
        break;
      }
      const Seg s0 = cur[0];
      if (ncur == 1 && s0.first < plim && s0.last - s0.first > kCoopMin && s0.depth > 0) {
        // one large segment: the whole block partitions it
        const int cut = partition_block(keys, vals, lpos, rpos, s0.first, s0.last, bp, wave);
        if (threadIdx.x == 0) {
          push(Seg{cut, s0.last, s0.depth - 1});
          push(Seg{s0.first, cut, s0.depth - 1});
        }
      } else
      for (int i = wave; i < ncur; i += kWaves) {
        const Seg s = cur[i];
        const int first = uni(s.first), last = uni(s.last), depth = uni(s.depth);
        const int len = last - first;
        if (first >= plim) {  // (a resumed or seeded one past the limit): set aside
          if (lane == 0) push(s);
        } else if (len <= 64) {
          if (len > 1) sort_small(keys, vals, first, len, depth, ws);
        } else if (depth == 0) {
          if (lane == 0) heap_sort(keys, vals, first, last);
        } else {
          if (lane == 0) move_median_to_first(keys, vals, first, first + 1, first + len / 2, last - 1);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          const int cut = partition_lds(keys, vals, lpos, rpos, first, last);
          if (lane == 0) {
            push(Seg{cut, last, depth - 1});
            push(Seg{first, cut, depth - 1});
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        c->top = c->pad ? 0 : c->pending;
        c->pending = 0;
      }
      Seg* t = cur;
      cur = nxt;
      nxt = t;
      __syncthreads();
    }
    __syncthreads();
  }

  // Raises the limit to `limit` (never lowers it): the deferred segments that
  // start below it go back into the current list, then run().
  __device__ __forceinline__ void resume(int limit) {
    limit = max(plim, limit);
    if (threadIdx.x == 0) {
      int nd = 0;
      const int ndef = min(c->ndef, kFinishDefer);
      for (int i = 0; i < ndef; ++i)
        if (deferred[i].first < limit) cur[nd++] = deferred[i];
      c->ndef = 0;
      c->top = c->pad ? 0 : nd;
      c->pending = 0;
    }
    run(limit);
  }
};
}  // namespace introsort
}  // namespace csm
