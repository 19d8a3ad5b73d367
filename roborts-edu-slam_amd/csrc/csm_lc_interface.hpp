// csm_lc_interface.hpp — the host rules of csm_loop_closure_scan_match
// (include/csm_loop_closure.h): what SlamProcessor::ScanMatchInterface
// (slam/slam_processor.cpp:250-326) and ScanMatchers::ScanMatch
// (scan_match/scan_matchers.h:179-289) decide around the correlative levels,
// stated once and free of HIP calls. csm_loop_closure.cpp computes with them;
// tests/cpp/lc_interface_check.cpp checks them against a restatement on the
// host alone.
//
//   box         MapSizeCheck's box (scan_matchers.h:365-390) against a submap that
//               cannot grow: UpdateBound's own criterion (grid_map_base.h:247-264)
//   start pose  where the fine level starts (correlate_scan_matcher.h:866-869)
//   score       the mean over the levels run (:281), the penalty, the clamp
//               (slam_processor.cpp:316-317)
//   wide gate   the largest level-0 gate that loses no final score above T
//
// Compiled with -ffp-contract=off like every host unit: each double
// expression rounds as the reference's does.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <initializer_list>

namespace csm {

// MapSizeCheck's box around a pose, in map cells: center +- (range_max + offset) / GetCellLength(),
// the centre GetMapCoordsPose of the pose (scale_factor * w + scale_factor * map_offset) and
// GetCellLength() = 1 / scale_factor (grid_map_base.h:307-309).
struct InterfaceBox {
  double min_x, min_y, max_x, max_y;
};

inline InterfaceBox interface_box(double resolution, const double map_offset[2], const double pose_world[3],
                                  double range_max, double search_space_size) {
  const double s = 1.0 / resolution;  // scale_factor_ (grid_map_base.h:50)
  const double cx = s * pose_world[0] + s * map_offset[0], cy = s * pose_world[1] + s * map_offset[1];
  const double max_size = (range_max + search_space_size) / (1 / s);
  return InterfaceBox{cx - max_size, cy - max_size, cx + max_size, cy + max_size};
}

// UpdateBound on a map whose bound box UpdateBoundAdaptMap left at (0, 0) .. (size + 1)
// (grid_map_base.h:266-273; what ResetScanMatchMapWithRangeVec's InitMapWithRangeVec does without
// auto resize): the box is kept when both its corners lie strictly inside that bound (BoundBox::
// IsInBounds). Otherwise the bound takes the box in: a low corner that missed leaves the bound's
// minimum <= 0, a high corner that missed leaves its maximum >= size + 1 > size, and either way
// PointInMap of that corner fails (strict, :344-352) and the reference grows the map. So "would
// grow" is exactly "does not fit" (a NaN corner does not fit).
inline bool interface_box_fits(const InterfaceBox& b, int32_t size_x, int32_t size_y) {
  const double bx = (double)(size_x + 1), by = (double)(size_y + 1);
  const auto in = [&](double x, double y) { return x > 0.0 && x < bx && y > 0.0 && y < by; };
  return in(b.min_x, b.min_y) && in(b.max_x, b.max_y);
}

// The smallest square submap in which the box would fit, centred as this one is (the box's middle
// keeps its distance from the map's centre, size / 2); for the error message.
inline int64_t interface_size_that_fits(const InterfaceBox& b, int32_t size_x, int32_t size_y) {
  const double cx = 0.5 * size_x, cy = 0.5 * size_y;
  // a low corner d cells below the centre needs n / 2 - d > 0: n > 2 d; a high corner d cells
  // above it needs n / 2 + d < n + 1: n > 2 d - 2
  double need = 0.0;
  for (double v : {2.0 * (cx - b.min_x), 2.0 * (cy - b.min_y), 2.0 * (b.max_x - cx) - 2.0, 2.0 * (b.max_y - cy) - 2.0}) {
    if (!(v < 1e15)) return -1;  // no size an int32 holds (a NaN or huge pose)
    if (v > need) need = v;
  }
  return (int64_t)std::floor(need) + 1;
}

// correlate_scan_matcher.h:866-869: a level writes its pose back only when its (clamped) response
// exceeds its threshold; otherwise the next level starts where this one did.
inline void interface_start_pose(int32_t accepted, const double averaged_world[3], const double pose_world[3],
                                 double out[3]) {
  const double* from = accepted ? averaged_world : pose_world;
  out[0] = from[0];
  out[1] = from[1];
  out[2] = from[2];
}

// scan_matchers.h:281 then slam_processor.cpp:316-317: the running sum starts at 0.0, takes each
// level's clamped response in order, is divided by the levels run, multiplied by the penalty and
// clamped to 1 last. responses[k] of a level not run is not read.
inline double interface_mean(const double responses[3], int32_t levels_run) {
  double sum = 0.0;  // (0.0 + r0 first: the reference's sum starts there)
  for (int32_t k = 0; k < levels_run; ++k) sum = sum + responses[k];
  return sum / levels_run;  // an int divisor, converted exactly
}

// the product first, the clamp on the product
inline double interface_score(double mean, double map_penalty) {
  const double penalised = mean * map_penalty;
  return penalised > 1.0 ? 1.0 : penalised;
}

// The largest min_response with which no submap whose final score exceeds T (the caller's strict >)
// is gated out, for a penalty <= 1: MapCheckPenalize with the logistic (csm_map_check_plan.hpp
// map_check_logistic: 1 / (1 + exp(..)) never exceeds 1; use_logistic = 1 is what ScanMatchInterface
// passes) or no map check. Not for use_logistic = 0: the raw coefficient reaches 1 + 2 * penalty_gain.
// Every level's response is clamped to 1 (:861-863), so with three levels
// score <= (min(s0, 1) + 1 + 1) / 3 and score > T needs s0 > 3 T - 2; with one level, s0 > T. The
// three-level gate is lowered by 8 ulps of 1: the five roundings between s0 and the score (two sums,
// the division, the product, and 3 T - 2 itself) each move a value below 4 by at most 2^-52.
inline double interface_wide_gate(double T, int32_t levels_run) {
  if (levels_run == 1) return T;
  return 3.0 * T - 2.0 - 8.0 * DBL_EPSILON;
}

}  // namespace csm
