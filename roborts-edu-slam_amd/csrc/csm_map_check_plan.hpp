// csm_map_check_plan.hpp — the host rules of the map check
// (OccuGridMap::MapFeedbackResponsePenalty, map/occu_grid_map.h:331-392, and
// SlamProcessor::MapCheckPenalize, slam/slam_processor.cpp:573-595), stated
// once and free of HIP calls: csm_gridmap.cpp computes with them, the batch
// kernel (csm_gridmap.hip) reads the pose records they fill, and
// tests/cpp/map_check_plan_check.cpp checks them against a restatement on the
// host alone.
//
//   guard        the arguments with which the reference returns 1.0 at once
//   beam rule    which points of a scan are checked
//   min_d2       the bound tolerance as a squared integer distance
//   pose record  GetMapCoordsPose, PointInMap, the host's sincos, the start cell
//   coefficient  the penalty from the count of rays that hit, and the logistic
//
// Compiled with -ffp-contract=off like every host unit: each double
// expression rounds as the reference's does.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "host_math.hpp"

namespace csm {

// :337-341: the coefficient is 1.0 and nothing else is looked at.
inline bool map_check_guard(int32_t check_point_num, double bound_tolerance, double penalty_gain) {
  return bound_tolerance < 0 || check_point_num <= 0 || penalty_gain <= 0.0 || penalty_gain >= 1.0;
}

// :368 divides all_point_num by check_point_num - 1: with one check point and
// a scan of two points or more the reference divides by zero.
inline bool map_check_divides_by_zero(int32_t check_point_num, int64_t n_points) {
  return check_point_num == 1 && n_points >= 2;
}

// point_step_num (:362-369); past the guard and the division by zero. The
// checked points are 0, step, 2 step, ... < n_points.
inline int32_t map_check_step(int32_t n_points, int32_t check_point_num) {
  if ((int64_t)n_points < 2 * (int64_t)check_point_num) return 1;
  return n_points / (check_point_num - 1);
}

// How many points that loop visits (:372).
inline int32_t map_check_checked(int32_t n_points, int32_t step) {
  return n_points <= 0 ? 0 : (int32_t)(((int64_t)n_points + step - 1) / step);
}

// The smallest integer squared cell distance whose sqrt exceeds the tolerance
// (util::EuclideanDistance2d, slam_util.h:94-96, compared at :463; sqrt is
// monotonic, so the callback's test is d2 >= min_d2). INT64_MAX for a NaN or
// huge tolerance: no cell is ever far enough.
inline int64_t map_check_min_d2(double bound_tolerance) {
  int64_t min_d2 = INT64_MAX;
  if (bound_tolerance < 1e9) {
    const double t0 = std::floor(bound_tolerance * bound_tolerance) - 2.0;
    min_d2 = t0 > 0.0 ? (int64_t)t0 : 0;
    while (!(std::sqrt((double)min_d2) > bound_tolerance)) ++min_d2;
  }
  return min_d2;
}

// One checked pose. 64 bytes, read by feedback_batch_kernel as it is: the
// pose's points are pts[pt_begin + k * step], k < n_checked, in metres.
struct MapCheckPose {
  int64_t pt_begin;   // first point of the pose's scan in the points buffer
  int32_t n_checked;  // points the beam rule visits
  int32_t step;       // their distance in the buffer
  double c, s;        // cos / sin of the pose angle (host sincos)
  double tx, ty;      // the pose's position in map cells
  int32_t x0, y0;     // the start cell: the sensor origin (0, 0) through the pose
  int32_t no_rays;    // the pose lies outside the map: coefficient 0.0, nothing is walked
  int32_t reserved;
};
static_assert(sizeof(MapCheckPose) == 64, "the kernel reads pose records as the host wrote them");

// PointInMap(x, y) with tolerance 0 on doubles (grid_map_base.h:344-352)
inline bool map_check_point_in_map(double x, double y, int32_t size_x, int32_t size_y) {
  return x > 0.0 && x < size_x - 0.0 && y > 0.0 && y < size_y - 0.0;
}

// GetMapCoordsPose (grid_map_base.h:89-93), PointInMap (:351-354), the pose's
// sincos and the start cell (:355-360 with sensor_origin (0, 0): the rotation
// of the origin adds nothing to the translation). Returns whether the pose
// lies in the map; outside, the record walks no rays and holds no start cell.
inline bool map_check_pose(double scale_factor, double offset_x, double offset_y, int32_t size_x, int32_t size_y,
                           const double pose[3], MapCheckPose* r) {
  const double s = scale_factor;
  r->tx = s * pose[0] + s * offset_x;
  r->ty = s * pose[1] + s * offset_y;
  host_sincos(pose[2], &r->s, &r->c);
  r->reserved = 0;
  if (!map_check_point_in_map(r->tx, r->ty, size_x, size_y)) {
    r->x0 = 0;
    r->y0 = 0;
    r->no_rays = 1;
    return false;
  }
  r->x0 = (int)(r->tx + 0.5);  // 0 < tx < size_x: the cast is defined
  r->y0 = (int)(r->ty + 0.5);
  r->no_rays = 0;
  return true;
}

// :371-391: `penalty` is a double raised by 1.0 per ray that hit (a sum of
// `count` ones is (double)count exactly), times the gain; floored at 0.1.
inline double map_check_coeff(int64_t count, double penalty_gain) {
  double penalty = (double)count;
  penalty *= penalty_gain;
  return std::max((1.0 + 2 * penalty_gain - penalty), 0.1);  // a NaN gain passes the guard and stays NaN here
}

// MapCheckPenalize's logistic (slam_processor.cpp:590), the host's exp.
inline double map_check_logistic(double penalty) { return (1 / (1 + std::exp(-10 * (penalty - 0.4)))); }

}  // namespace csm
