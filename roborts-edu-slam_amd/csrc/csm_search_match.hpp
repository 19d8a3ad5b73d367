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

#include <algorithm>
#include <cstdint>

#include "csm.h"  // csm_match_type
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

// ---- the reduced finish -------------------------------------------------
// list_finish reads FindBest's band, 20 positional and 20 near-best angular
// candidates of the collected set H, yet sorts all of it. The reduced finish
// feeds it a subset R of H that a selection (csm_select.hpp on the device; any
// function with the same definition) cuts out of the unsorted list:
//
//   select(pred, K, band_on, best) =
//     { h : pred(h) and (key(h) >= key_K or (band_on and in_response_band(h.score, best))) }
//
// key: the order-preserving 64-bit image of score + 0.0; key_K: the K-th
// largest key among the hits passing pred (the lowest when fewer than K pass),
// so the result is closed under ties with the K-th. With K = kCovPoints + 2:
//   A = select(always, K, band on, best)        ranks 0..21 and the whole band:
//                                               a tie-closed prefix of sorted H
//   (bx, by) = find_best over sorted A          the band lies inside A
//   B = select(near_best(bx, by, sres / mres), K, band off)
//   R = A u B (flat is unique within a window)
//
// list_finish(R) = list_finish(H):
//   - every run of equal scores that list_finish's first loop tests starts at
//     rank <= 20 or lies in the band, so it lies inside A, whole (A is closed
//     under ties), at the rank it has in H;
//   - the first element of R past A has rank >= 22 and is outside the band:
//     its run's test is false and the loop breaks there, exactly as on H;
//   - find_best reads the band, the positional list the first 20 of A;
//   - the angular loop reads near-best runs with run_rank <= 20: B holds the
//     near-best set's ranks 0..21, closed under ties, so all of them, at the
//     ranks they have in H's near-best subsequence;
//   - a near-best member of A that scores below B's K-th comes after at least
//     22 near-best entries and only triggers the `break`.
// tests/cpp/list_reduce_check.cpp checks it bit for bit against
// list_finish(H) on planted ties and bands.
#ifndef CSM_REDUCE_K  // the check's mutation builds with 21, which must fail
#define CSM_REDUCE_K (kCovPoints + 2)
#endif
constexpr int kReduceK = CSM_REDUCE_K;

struct SelectSpec {
  int32_t k;        // >= 1
  int32_t band_on;  // also every hit with in_response_band(score, best)
  double best;
  int32_t near_on;  // pred: near_best(grid.x(flat), grid.y(flat), bx, by, tol); 0: always
  CandGrid grid;
  double bx, by, tol;
};

// The selection's key: a double's order-preserving 64-bit image (-0.0 and
// +0.0 share one: score + 0.0 first; negatives flip all bits, the others the
// sign bit).
CSM_RULE uint64_t select_key(double score) {
  const double s = score + 0.0;
  const uint64_t u = (uint64_t)__builtin_bit_cast(int64_t, s);
  return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}

// (bx, by) as list_finish's find_best gives them over hits[0, n) sorted by
// score descending (hits[0].score the best).
void sorted_best_xy(const PyrHit* hits, int64_t n, const FinishWindow& W, double* bx, double* by);

enum class Reduced { kDone, kOverflow, kFailed };

// select(spec, out, cap) -> the selection's full count (out[0, min(count,
// cap)) written), or < 0 when it failed. a and b: max_sel entries each; the
// union is built in a (2 * max_sel entries). kOverflow: a selection outgrew
// max_sel (a huge band, or many candidates tied at the K-th), or its front is
// not `best`: nothing is written, the caller finishes the whole list.
template <class Select>
Reduced reduced_finish(Select&& select, PyrHit* a, PyrHit* b, int64_t max_sel, double best, const FinishWindow& W,
                       double cov[9], ListFinish* out, int64_t* n_reduced = nullptr) {
  SelectSpec sa{};
  sa.k = kReduceK;
  sa.band_on = 1;
  sa.best = best;
  sa.grid = W.grid;
  const int64_t na = select(sa, a, max_sel);
  if (na < 0) return Reduced::kFailed;
  if (na < 1 || na > max_sel) return Reduced::kOverflow;
  int64_t n = na;
  if (W.type != CSM_FINE) {  // FINE reads no angular list: A alone
    std::sort(a, a + na, [](const PyrHit& x, const PyrHit& y) { return x.score > y.score; });
    if (!(a[0].score == best)) return Reduced::kOverflow;
    SelectSpec sb = sa;
    sb.band_on = 0;
    sb.near_on = 1;
    sb.tol = W.sres / W.mres;
    sorted_best_xy(a, na, W, &sb.bx, &sb.by);
    const int64_t nb = select(sb, b, max_sel);
    if (nb < 0) return Reduced::kFailed;
    if (nb > max_sel) return Reduced::kOverflow;
    // R = A u B: B's members that A does not hold (a merge of the two by flat)
    auto by_flat = [](const PyrHit& x, const PyrHit& y) { return x.flat < y.flat; };
    std::sort(a, a + na, by_flat);
    std::sort(b, b + nb, by_flat);
    int64_t i = 0;
    for (int64_t j = 0; j < nb; ++j) {
      while (i < na && a[i].flat < b[j].flat) ++i;
      if (i < na && a[i].flat == b[j].flat) continue;
      a[n++] = b[j];
    }
  }
  if (n_reduced) *n_reduced = n;
  list_finish(a, n, W, cov, out);
  return Reduced::kDone;
}

}  // namespace csm
