// csm_search_match.hpp — the host half of a window's finish, and the finish
// over a collected list (csm_search_match, include/csm.h).
//
// BasedCorrelationScanMatch::ScanMatch after the candidates are sorted
// (correlate_scan_matcher.h:835-869; covariances :887-1019) reads a small part
// of the window: with s* the best score and T = cov_bound(s*),
//   FindBestCandidate (:670-710)           the sorted prefix with s >= s* - 0.01
//   ComputePositionalCovariance (:887-956) the first 20 sorted candidates with s > T
//   ComputeAngularCovariance (:965-1019)   in sorted order, the candidates with s >= T
//                                          near the best pose, 20 of them at most
// so the set {s >= T}, sorted by score, gives every output the full sort
// gives -- unless two equal scores sit where std::sort's order among them
// decides an output (csm_finish_rules.hpp tie_matters_*). list_finish says so
// then, and the caller takes the exhaustive finish.
//
// Host only, no HIP call: tests/cpp/search_match_check.cpp drives it
// stand-alone against a plain std::sort finish over full score arrays.
#pragma once

#include <cstdint>

#include "csm_finish_rules.hpp"

namespace csm {

constexpr double kMaxVariance = 500.0;      // util/slam_util.h:57
constexpr double kDoubleTolerance = 1e-06;  // util/slam_util.h:59

// What the finish's host half reads of a window besides its FinishOut.
struct FinishWindow {
  CandGrid grid;             // candidate (x, y) by flat index, map cells
  const AngleEntry* angles;  // the window's angle rows: angle, host libm cos / sin
  int type;                  // csm_match_type: which covariances are computed (:835-858)
  double mres;               // map resolution (GetCellLength)
  double sres;               // search_space_resolution
  double ares;               // search_angle_resolution
};

// The covariance lists' sums as the reference accumulates them (zero for a
// list that was not summed).
struct CovSums {
  double pos_norm = 0.0, vxx = 0.0, vxy = 0.0, vyy = 0.0;  // :915-928
  double ang_norm = 0.0, ang_acc = 0.0;                    // :990-1003
};

// Everything ScanMatch does once the sorted candidates are summarised in `o`
// (:700-707 the averaged angle's atan2, :835-858 the covariances per type,
// :861-863 the response): pose_map = the best pose in map cells / rad, cov is
// in/out and written per type as the reference writes it, skip_lists (bit 0
// positional, bit 1 angular) leaves a covariance to a later level. Returns the
// response.
double finish_complete(const FinishOut& o, const FinishWindow& W, int skip_lists, double pose_map[3], double cov[9],
                       CovSums* sums = nullptr);

struct ListFinish {
  bool tie_matters;  // true: nothing else is set, cov is untouched
  FinishOut o;       // front, FindBest's count / sums / averaged (x, y), the two lists
  CovSums sums;
  double response;
  double pose_map[3];
};

// The finish over hits[0, n): every candidate of the window with score >= T,
// T = cov_bound(the best score), in any order (sorted here, in place, by score
// descending; equal scores in any order: they reach an output only when a tie
// matters). n >= 1. The early returns are the reference's (best <
// kDoubleTolerance: :894-899, :973-976).
void list_finish(PyrHit* hits, int64_t n, const FinishWindow& W, double cov[9], ListFinish* out);

}  // namespace csm
