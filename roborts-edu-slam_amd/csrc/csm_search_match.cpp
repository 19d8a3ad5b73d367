// csm_search_match.cpp — the finish's host half (finish_complete) and the
// finish over a collected list (list_finish); csm_search_match.hpp. Host
// arithmetic only: no HIP call, no context.
#include "csm_search_match.hpp"

#include <algorithm>
#include <cmath>

#include "csm.h"  // csm_match_type

namespace csm {

double finish_complete(const FinishOut& o, const FinishWindow& W, int skip_lists, double pose_map[3], double cov[9],
                       CovSums* sums) {
  const double best_score = o.best_score;
  const double best_x = o.best_x, best_y = o.best_y;
  double best_a = W.angles[W.grid.angle_index(o.front_idx)].angle;
  if (o.count > 1) best_a = std::atan2(o.thy / o.ssum, o.thx / o.ssum);  // :702-706

  const double max_ang_var = 4 * (W.ares * W.ares);  // :801
  CovSums S;

  auto positional = [&]() {  // ComputePositionalCovariance (:887-956)
    for (int i = 0; i < 9; ++i) cov[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (best_score < kDoubleTolerance) {
      cov[0] = kMaxVariance;
      cov[4] = kMaxVariance;
      cov[8] = max_ang_var;
      return;
    }
    double vxx = 0.0, vxy = 0.0, vyy = 0.0, norm = 0.0;
    for (int i = 0; i < o.n_pos; ++i) {
      const double sc = o.pos_score[i];
      const double dx = W.grid.x(o.pos_idx[i]) - best_x, dy = W.grid.y(o.pos_idx[i]) - best_y;
      norm += sc;
      vxx += (dx * dx * sc);
      vxy += (dx * dy * sc);
      vyy += (dy * dy * sc);
    }
    S.pos_norm = norm;
    S.vxx = vxx;
    S.vxy = vxy;
    S.vyy = vyy;
    if (norm > kDoubleTolerance) {
      double xx = vxx / norm, xy = vxy / norm, yy = vyy / norm;
      const double r = W.sres / W.mres;
      const double minv = 0.1 * (r * r);
      xx = std::max<double>(xx, minv);
      yy = std::max<double>(yy, minv);
      const double m2 = W.mres * W.mres;
      cov[0] = (xx * m2) / best_score;
      cov[1] = (xy * m2) / best_score;
      cov[3] = (xy * m2) / best_score;
      cov[4] = (yy * m2) / best_score;
      cov[8] = max_ang_var;
    }
    if (within_tol(cov[0] - 0.0, kDoubleTolerance)) cov[0] = kMaxVariance;  // util::DoubleEqual(cov, 0)
    if (within_tol(cov[4] - 0.0, kDoubleTolerance)) cov[4] = kMaxVariance;
  };
  auto angular = [&]() {  // ComputeAngularCovariance (:965-1019)
    if (best_score < kDoubleTolerance) {
      cov[8] = max_ang_var;
      return;
    }
    double norm = 0.0, acc = 0.0;
    for (int i = 0; i < o.n_ang; ++i) {
      const double sc = o.ang_score[i];
      const double d = W.angles[W.grid.angle_index(o.ang_idx[i])].angle - best_a;
      norm += sc;
      acc += (d * d * sc);
    }
    S.ang_norm = norm;
    S.ang_acc = acc;
    // :1007-1013: the max / 4 assigned for a tiny accumulated variance is
    // overwritten by accumulated / norm on the next line
    cov[8] = (norm > kDoubleTolerance) ? acc / norm : 200 * max_ang_var;
  };
  const bool pos = !(skip_lists & 1), ang = !(skip_lists & 2);
  switch (W.type) {
    case CSM_COARSE:
      if (pos) positional();
      if (ang) angular();
      break;
    case CSM_FINE:
      if (pos) positional();
      break;
    case CSM_SUPER:
      if (ang) angular();
      break;
    default:
      break;
  }
  pose_map[0] = best_x;
  pose_map[1] = best_y;
  pose_map[2] = best_a;
  if (sums) *sums = S;
  return best_score > 1.0 ? 1.0 : best_score;  // :861-863
}

void sorted_best_xy(const PyrHit* hits, int64_t n, const FinishWindow& W, double* bx, double* by) {
  struct Scores {
    const PyrHit* h;
    double operator[](int i) const { return h[i].score; }
  };
  struct Indices {
    const PyrHit* h;
    int64_t operator[](int i) const { return h[i].flat; }
  };
  auto cos_sin = [&](int a) { return CosSin{W.angles[a].cosine, W.angles[a].sine}; };
  FinishOut o{};
  find_best(Scores{hits}, Indices{hits}, (int)n, hits[0].score, W.grid, cos_sin, &o, bx, by);
}

void list_finish(PyrHit* hits, int64_t n, const FinishWindow& W, double cov[9], ListFinish* out) {
  std::sort(hits, hits + n, [](const PyrHit& a, const PyrHit& b) { return a.score > b.score; });
  *out = ListFinish{};
  FinishOut& o = out->o;
  const double best = hits[0].score;
  const double bound = cov_bound(best);
  const bool want_pos = W.type != CSM_SUPER, want_ang = W.type != CSM_FINE;  // the lists the type reads (:835-858)
  // ranks and ties over the candidates above the bound: a run of equal scores
  // starting at sorted position r has rank r
  int64_t n_above = 0;
  while (n_above < n && hits[n_above].score > bound) ++n_above;
  for (int64_t r = 0; r < n_above;) {
    int64_t e = r + 1;
    while (e < n && hits[e].score == hits[r].score) ++e;
    if (tie_matters_positional((int)std::min<int64_t>(e - r, 2), (int)std::min<int64_t>(r, kCovPoints + 1),
                               in_response_band(hits[r].score, best), want_pos)) {
      out->tie_matters = true;
      return;
    }
    if (r > kCovPoints && !in_response_band(hits[r].score, best)) break;  // no later run can matter
    r = e;
  }
  // FindBestCandidate over the sorted list (the band lies above the bound)
  struct Scores {
    const PyrHit* h;
    double operator[](int i) const { return h[i].score; }
  };
  struct Indices {
    const PyrHit* h;
    int64_t operator[](int i) const { return h[i].flat; }
  };
  auto cos_sin = [&](int a) { return CosSin{W.angles[a].cosine, W.angles[a].sine}; };
  double bx, by;
  find_best(Scores{hits}, Indices{hits}, (int)n, best, W.grid, cos_sin, &o, &bx, &by);
  // ComputePositionalCovariance's candidates (:915-928)
  o.n_pos = 0;
  for (int64_t i = 0; want_pos && i < n_above && o.n_pos < kCovPoints; ++i) {
    o.pos_idx[o.n_pos] = (int32_t)hits[i].flat;
    o.pos_score[o.n_pos] = hits[i].score;
    o.n_pos++;
  }
  // ComputeAngularCovariance's candidates (:990-1003): the near-best set in
  // sorted order, ranks and ties within it
  o.n_ang = 0;
  const double lin_tol = W.sres / W.mres;
  int64_t rank = 0;       // near-best candidates so far
  int64_t run_rank = 0;   // ... before the current run of equal scores
  int64_t run_len = 0;    // near-best candidates of the current run
  double run_score = 0.0;
  for (int64_t i = 0; want_ang && i < n; ++i) {
    const double s = hits[i].score;
    if (!(s >= bound)) break;
    const int idx = (int)hits[i].flat;
    if (!near_best(W.grid.x(idx), W.grid.y(idx), bx, by, lin_tol)) continue;
    if (run_len > 0 && s == run_score) {
      ++run_len;
    } else {
      run_rank = rank;
      run_len = 1;
      run_score = s;
    }
    if (tie_matters_angular((int)std::min<int64_t>(run_len, 2), (int)std::min<int64_t>(run_rank, kCovPoints + 1))) {
      out->tie_matters = true;
      return;
    }
    if (run_rank > kCovPoints) break;  // past the list and the value after it
    if (o.n_ang < kCovPoints) {
      o.ang_idx[o.n_ang] = idx;
      o.ang_score[o.n_ang] = s;
      o.n_ang++;
    }
    ++rank;
  }
  out->response = finish_complete(o, W, 0, out->pose_map, cov, &out->sums);
}

}  // namespace csm
