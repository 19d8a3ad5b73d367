// csm_finish_rules.hpp — the finish's decision rules, each stated once.
//
// The finish turns a window's scores into the FinishOut the host completes:
// the front of std::sort(candidates, greater) (correlate_scan_matcher.h:
// 607-611), FindBestCandidate's tied prefix and weighted sums (:670-710) and
// the candidate lists of ComputePositionalCovariance / ComputeAngularCovariance
// (:887-1003). Four finishes apply these rules: the fast pass
// (finish_fast_body, csm_finish_fast.hip), the fused fast pass (tail::finish,
// csm_tail.hpp), the exact pass (finish_window, csm_finish.hip) and the host's
// std::sort (host_sort_finish, csm_host_finish.cpp). The fast forms add "no
// tie here can change an output, so no sort is needed".
//
// Pure functions for host and device: no HIP builtins, no LDS, no wave
// intrinsics, no atomics. Every device use is force-inlined (a call inside
// finish_window cost 211 VGPRs and scratch against 129 and none).
// tests/cpp/finish_rules_check.cpp drives them on the CPU against a plain
// std::sort finish.
#pragma once

#include <cstdint>

#include "csm_internal.hpp"

#define CSM_RULE __host__ __device__ __forceinline__

namespace csm {

constexpr double kResponseFilterTolerance = 1e-2;  // correlate_scan_matcher.h:763

// util::DoubleEqual(a, b, tol) on d = a - b (util/slam_util.h:70-73)
CSM_RULE bool within_tol(double d, double tol) {
  return d < 0.0 ? d >= -__builtin_fabs(tol) : d <= __builtin_fabs(tol);
}
// FindBestCandidate's prefix test (:676): DoubleEqual(s, best, 1e-2), i.e.
// within_tol with the positive tolerance. best is the window's max, so d < 0
// is the usual side; the hint also keeps the two comparisons branches in
// find_best's sequential loop (folded into a select they cost 2 VGPRs there,
// an occupancy step of finish_fast_kernel<1024, 4>: 64 -> 66).
CSM_RULE bool in_response_band(double s, double best) {
  const double d = s - best;
  if (__builtin_expect(d < 0.0, 1)) return d >= -kResponseFilterTolerance;
  return d <= kResponseFilterTolerance;
}
// std::min(best - 0.1, 0.5): the covariance lists' score bound (:912, :986)
CSM_RULE double cov_bound(double best) {
  const double lo = best - 0.1;
  return (0.5 < lo) ? 0.5 : lo;
}
// the angular list's test (:994-996): (x, y) within lin_tol of the best pose
CSM_RULE bool near_best(double x, double y, double bx, double by, double tol) {
  return within_tol(x - bx, tol) && within_tol(y - by, tol);
}

// A window's candidates by flat enumeration index, as the reference stored
// them in Candidate2D (:554, :569, :572): angle-major, then x, then y.
struct CandGrid {
  double x0, y0, step;
  int n_space;
  CSM_RULE double x(int idx) const { return x0 + ((idx / n_space) % n_space) * step; }
  CSM_RULE double y(int idx) const { return y0 + (idx % n_space) * step; }
  CSM_RULE int angle_index(int idx) const { return idx / (n_space * n_space); }
};

// FinishArgs::skip_lists as the lists a finish fills; `lists` is the seal's.
struct WantLists {
  bool pos, ang;
  int lists;
};
CSM_RULE WantLists want_lists(int skip_lists) {
  const bool pos = !(skip_lists & 1), ang = !(skip_lists & 2);
  return WantLists{pos, ang, (pos ? 1 : 0) | (ang ? 2 : 0)};
}

// ---- levels: which scores the fast finish compacts ----------------------
// Level k < 7 holds s > bound with s - best >= -0.01 * 2^k, level 7 every
// s > bound; kFinishLevels: none. Branch-free: d >= -dl holds from the first
// such level on (dl doubles), so the level counts the failures.
constexpr int kFinishLevels = 8;
CSM_RULE int level_of(double s, double best, double bound) {
  const double d = s - best;
  double dl = 0.01;
  int lv = 0;
#ifdef __clang__
#pragma unroll
#endif
  for (int k = 0; k < kFinishLevels - 1; ++k, dl *= 2.0) lv += (d < -dl) ? 1 : 0;
  return (s > bound) ? lv : kFinishLevels;
}
// A lane's level counts, 16 bits a level (levels 0-3 in c0, 4-7 in c1; below
// 2^16 scores a lane and wave). The callers add c0 and c1 across lanes.
struct LevelCounts {
  uint64_t c0 = 0, c1 = 0;
  CSM_RULE void add(int lv) {
    const uint64_t one = 1ull << (16 * (lv & 3));
    c0 += lv < 4 ? one : 0ull;
    c1 += (lv >= 4 && lv < kFinishLevels) ? one : 0ull;
  }
  CSM_RULE int level(int k) const { return (int)(((k < 4 ? c0 : c1) >> (16 * (k & 3))) & 0xFFFF); }
};
// The smallest level whose cumulative count reaches kCovPoints (or all
// > bound); without the positional list, level 0: exactly FindBest's prefix
// set. n_selected: the scores of levels 0..level.
CSM_RULE void select_level(const int* counts, bool want_pos, int* level, int* n_selected) {
  int L = want_pos ? kFinishLevels - 1 : 0, cum = 0;
  for (int k = 0; want_pos && k < kFinishLevels; ++k) {
    cum += counts[k];
    if (cum >= kCovPoints) {
      L = k;
      break;
    }
  }
  int n = 0;
  for (int k = 0; k <= L; ++k) n += counts[k];
  *level = L;
  *n_selected = n;
}

// ---- ranks and ties -----------------------------------------------------
// x's rank by value among keys[0..n): the elements greater, and those equal
// (x itself among them). keys is 16-byte aligned and padded with -inf to a
// multiple of 4: read 4 at a time, two 16-byte loads.
struct __attribute__((aligned(16), may_alias)) ScorePair {
  double x, y;
};
CSM_RULE void rank_among(const double* keys, int n, double x, int* greater, int* equal) {
  int r = 0, eq = 0;
  for (int j = 0; j < n; j += 4) {
    const ScorePair u01 = *reinterpret_cast<const ScorePair*>(&keys[j]);
    const ScorePair u23 = *reinterpret_cast<const ScorePair*>(&keys[j + 2]);
    r += ((u01.x > x) ? 1 : 0) + ((u01.y > x) ? 1 : 0) + ((u23.x > x) ? 1 : 0) + ((u23.y > x) ? 1 : 0);
    eq += ((u01.x == x) ? 1 : 0) + ((u01.y == x) ? 1 : 0) + ((u23.x == x) ? 1 : 0) + ((u23.y == x) ? 1 : 0);
  }
  *greater = r;
  *equal = eq;
}
// A repeated score decides an output, so std::sort's order is needed: inside
// FindBest's prefix (its sums are order-dependent), or among the positional
// list's 20 and the value just past them (rank 20 included: the list stores
// ranks below 20, :915-928).
CSM_RULE bool tie_matters_positional(int equal, int rank, bool in_band, bool want_pos) {
  return equal > 1 && (in_band || (want_pos && rank <= kCovPoints));
}
// ... among the near-best set's first 20 and the value just past them (:990-1003)
CSM_RULE bool tie_matters_angular(int equal, int rank) { return equal > 1 && rank <= kCovPoints; }

// ---- FindBestCandidate (:670-710) ---------------------------------------
// The sequential sums over the sorted candidates' tied prefix (keys[i],
// idx[i], i < n, in sorted order; best = keys[0]) and FinishOut's header
// fields from them. cos_sin(a) returns angle row a's (cosine, sine): host libm
// values, wherever the caller keeps them. The summation order and the
// count > 1 branch (:700-707; the atan2 of thy / ssum, thx / ssum is left to
// the host) are the reference's.
struct CosSin {
  double cosine, sine;
};
template <class Keys, class Idx, class AngleFn>
CSM_RULE void find_best(Keys keys, Idx idx, int n, double best, const CandGrid& g, AngleFn cos_sin, FinishOut* o,
                        double* best_x, double* best_y) {
  double ax = 0.0, ay = 0.0, thx = 0.0, thy = 0.0, ssum = 0.0;
  int count = 0;
  for (int i = 0; i < n; ++i) {
    const double s = keys[i];
    if (!in_response_band(s, best)) break;
    const int id = (int)idx[i];
    const CosSin cs = cos_sin(g.angle_index(id));
    ax += g.x(id) * s;
    ay += g.y(id) * s;
    thx += cs.cosine * s;
    thy += cs.sine * s;
    ssum += s;
    count++;
  }
  const int front = (int)idx[0];
  o->front_idx = front;
  o->count = count;
  o->best_score = best;
  o->thx = thx;
  o->thy = thy;
  o->ssum = ssum;
  if (count > 1) {
    *best_x = ax / ssum;
    *best_y = ay / ssum;
  } else {
    *best_x = g.x(front);
    *best_y = g.y(front);
  }
  o->best_x = *best_x;
  o->best_y = *best_y;
}

}  // namespace csm
