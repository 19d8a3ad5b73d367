// csm_optimize_step.hpp — the Gauss-Newton matcher's step rules, each stated
// once (BasedOptimizeScanMatch::ScanMatch, optimize_scan_matcher.h:84-152).
//
// What happens between two UpdateCost evaluations: the cost's normalisation
// (:220), CalculateDet's H.ldlt().solve(b) (:136-142; Eigen 3.3 restated),
// the NaN test (:103-106), the two stop tests (:112-118) and UpdatePose with
// util::MaxAbxLimit (:144-152). The host loop (optimize_batch,
// csm_optimize_host.cpp) and the one-launch solve (optimize_solve_kernel,
// csm_optimize.hip) both call step(), so a scan takes the same path and gets
// the same bits whichever runs it.
//
// Pure functions for host and device: no HIP builtins, no LDS, no libm calls
// (fabs and the NaN test are spelled so that both compilers emit the plain
// operation). Every operation is a separately rounded binary64 add, subtract,
// multiply or divide: nothing may be contracted into an FMA (the library is
// built with -ffp-contract=off; the pragma below holds for a device build
// that forgets it). tests/cpp/optimize_step_check.cpp drives them on the CPU
// against tests/opt_pyref.py.
#pragma once

#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__)
#define CSM_OPT_RULE __host__ __device__ __forceinline__
#pragma clang fp contract(off)
#else
#define CSM_OPT_RULE inline
#endif

namespace csm {
namespace opt {

constexpr double kCostPointSize = 1000;  // optimize_scan_matcher.h:234

// per scan: kSkip = invalid input (pose untouched, kMaxCost), kRun =
// iterating, kDone = converged or out of iterations, kNan = NaN step,
// kHost = the angle left the device sincos' domain (the host loop re-runs it)
enum : int32_t { kSkip = 0, kRun = 1, kDone = 2, kNan = 3, kHost = 4 };

// What step() reads of OptimizeScanMatchParam. max_update_cells =
// max_update_distance / map_resolution_ (:146-147), divided once by the caller.
struct StepParam {
  double cost_decrease_threshold, cost_min_threshold;
  double max_update_cells, max_update_angle;
};

CSM_OPT_RULE double abs_(double v) { return __builtin_fabs(v); }
CSM_OPT_RULE bool is_nan(double v) { return v != v; }
CSM_OPT_RULE void swap_(double& a, double& b) {
  const double t = a;
  a = b;
  b = t;
}

// util::MaxAbxLimit (util/slam_util.h:79-86)
CSM_OPT_RULE double max_abs_limit(double value, double limit) {
  if (value > abs_(limit))
    value = abs_(limit);
  else if (value < -abs_(limit))
    value = -abs_(limit);
  return value;
}

// H_.ldlt().solve(b_) (optimize_scan_matcher.h:136-142): Eigen 3.3
// LDLT<Matrix3d, Lower>. Factor: diagonal pivoting on the trailing corner
// (first maximum wins), symmetric swaps through the lower triangle, then
// a_kk -= a_k. . (D a_k.)^T and the column below scaled by the pivot.
// Solve: P, unit-lower rows, D pseudo-inverse (|d| > DBL_MIN), unit-upper
// rows from the bottom, P^T. s = lower triangle of the symmetric H as
// {H00, H10, H11, H20, H21, H22}.
CSM_OPT_RULE void ldlt_solve3(const double s[6], const double rhs[3], double out[3]) {
  double a[3][3] = {{s[0], s[1], s[3]}, {s[1], s[2], s[4]}, {s[3], s[4], s[5]}};
  int tr[3] = {0, 1, 2};
  for (int k = 0; k < 3; ++k) {
    int big = k;
    double bv = abs_(a[k][k]);
    for (int i = k + 1; i < 3; ++i)
      if (abs_(a[i][i]) > bv) {
        bv = abs_(a[i][i]);
        big = i;
      }
    tr[k] = big;
    if (big != k) {
      for (int j = 0; j < k; ++j) swap_(a[k][j], a[big][j]);
      for (int i = big + 1; i < 3; ++i) swap_(a[i][k], a[i][big]);
      swap_(a[k][k], a[big][big]);
      for (int i = k + 1; i < big; ++i) {
        const double t = a[i][k];
        a[i][k] = a[big][i];
        a[big][i] = t;
      }
    }
    if (k > 0) {
      double t[2];
      for (int i = 0; i < k; ++i) t[i] = a[i][i] * a[k][i];
      a[k][k] -= (k == 1) ? (a[k][0] * t[0]) : (a[k][0] * t[0] + a[k][1] * t[1]);
      if (k == 1) a[2][1] -= a[2][0] * t[0];
    }
    const double akk = a[k][k];
    const bool valid = abs_(akk) > 0.0;
    if (k == 0 && !valid) {
      tr[0] = 0;
      tr[1] = 1;
      tr[2] = 2;
      break;
    }
    if (k < 2 && valid)
      for (int r = k + 1; r < 3; ++r) a[r][k] /= akk;
  }
  double d[3] = {rhs[0], rhs[1], rhs[2]};
  for (int k = 0; k < 3; ++k)
    if (tr[k] != k) swap_(d[k], d[tr[k]]);
  d[1] -= a[1][0] * d[0];
  d[2] -= (a[2][0] * d[0] + a[2][1] * d[1]);
  for (int i = 0; i < 3; ++i) d[i] = (abs_(a[i][i]) > DBL_MIN) ? d[i] / a[i][i] : 0.0;
  d[1] -= a[2][1] * d[2];
  d[0] -= (a[1][0] * d[1] + a[2][0] * d[2]);
  for (int k = 2; k >= 0; --k)
    if (tr[k] != k) swap_(d[k], d[tr[k]]);
  out[0] = d[0];
  out[1] = d[1];
  out[2] = d[2];
}

// UpdateCost's normalisation (:220): v0 = the sum of e^2, valid = points in the map
CSM_OPT_RULE double normalized_cost(double v0, int32_t valid) {
  const int valid_point = 1 + valid;
  return v0 * (kCostPointSize / valid_point);
}

// :112-118, from the second iteration on
CSM_OPT_RULE bool stops(int iter, double last_cost, double cost, const StepParam& P) {
  return iter > 0 && (last_cost - cost < P.cost_decrease_threshold || cost < P.cost_min_threshold);
}

// UpdatePose (:144-152)
CSM_OPT_RULE void update_pose(const double det[3], const StepParam& P, double est[3]) {
  est[0] += max_abs_limit(det[0], P.max_update_cells);
  est[1] += max_abs_limit(det[1], P.max_update_cells);
  est[2] += max_abs_limit(det[2], P.max_update_angle);
}

// One iteration's step after its UpdateCost: v = {cost, H00, H10, H11, H20,
// H21, H22, b0, b1, b2} summed in point order, valid = points in the map,
// *cost = the previous iteration's cost in, this one's out; est (map cells)
// is stepped when the result is kRun. Returns kRun, kDone or kNan.
CSM_OPT_RULE int32_t step(const double v[10], int32_t valid, int iter, const StepParam& P, double est[3],
                          double* cost) {
  const double last = *cost;  // :88
  *cost = normalized_cost(v[0], valid);
  double det[3];
  ldlt_solve3(v + 1, v + 7, det);  // CalculateDet (:101)
  if (is_nan(det[0]) || is_nan(det[1]) || is_nan(det[2])) return kNan;  // :103-106
  if (stops(iter, last, *cost, P)) return kDone;
  update_pose(det, P, est);
  return kRun;
}

}  // namespace opt
}  // namespace csm
