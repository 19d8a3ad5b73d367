// csm_ranges_host.hpp — raw laser ranges to scan endpoints on the host: the
// arithmetic of SlamNode::BuildRangeDataContainer (roborts_slam_node.cpp:290-311)
// followed by RangeDataContainer::CreateFrom (sensor_data_manager.h:99-115),
// operation for operation (build with -ffp-contract=off). Pure host code over
// csm.h and host_math.hpp, so tests/cpp/ranges_check.cpp compiles it alone.
// The device path (csm_ranges.hip) takes its threshold and its per-beam
// (cos, sin) table from here and repeats only the comparisons and multiplies.
#pragma once

#include <cmath>
#include <cstdint>

#include "csm.h"
#include "host_math.hpp"

namespace csm {

// LaserRangeFinder::set_range_threshold_scale (sensor_data_manager.h:43-49).
// False where the reference leaves range_threshold_ uninitialised
// (min_range_ >= max_range_) and for fields no LaserScan should carry.
inline bool laser_threshold(const csm_laser& L, double* threshold) {
  if (L.n_beams <= 0) return false;
  if (!std::isfinite(L.angle_min) || !std::isfinite(L.angle_increment) || !std::isfinite(L.range_min) ||
      !std::isfinite(L.range_max) || !std::isfinite(L.range_threshold_scale))
    return false;
  const double lo = (double)L.range_min, hi = (double)L.range_max;
  if (!(lo < hi)) return false;
  const double span = hi - lo;
  const double part = L.range_threshold_scale * span;
  *threshold = lo + part;
  return true;
}

// Beam i's (cos a_i, sin a_i), a_0 = angle_min, a_{i+1} = a_i + angle_increment
// in double (roborts_slam_node.cpp:294,306), one sincos per beam (:303 as GCC
// compiles it). cs holds n_beams (cos, sin) pairs.
inline void laser_trig_table(const csm_laser& L, double* cs) {
  double a = (double)L.angle_min;
  const double inc = (double)L.angle_increment;
  for (int32_t i = 0; i < L.n_beams; ++i) {
    double s, c;
    host_sincos(a, &s, &c);
    cs[2 * i] = c;
    cs[2 * i + 1] = s;
    a += inc;
  }
}

// roborts_slam_node.cpp:300
inline bool range_kept(float r, double range_min, double threshold) {
  const double d = (double)r;
  return d > range_min && d < threshold;
}

// The kept beams' endpoints of n_scans scans, back to back, and their prefix
// counts. pts null: offsets only. Returns false when more than `capacity`
// points would be written (nothing is written past it).
inline bool ranges_to_points(const csm_laser& L, double threshold, const double* cs, int32_t n_scans,
                             const float* ranges, double factor, double* pts, int64_t capacity, int64_t* offsets) {
  const double lo = (double)L.range_min;
  int64_t n = 0;
  offsets[0] = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    const float* r = ranges + (int64_t)s * L.n_beams;
    for (int32_t i = 0; i < L.n_beams; ++i) {
      if (!range_kept(r[i], lo, threshold)) continue;
      if (pts) {
        if (n >= capacity) return false;
        const double d = (double)r[i];
        const double x = cs[2 * i] * d, y = cs[2 * i + 1] * d;  // :303
        pts[2 * n] = x * factor;                                // sensor_data_manager.h:111
        pts[2 * n + 1] = y * factor;
      }
      ++n;
    }
    offsets[s + 1] = n;
  }
  return true;
}

}  // namespace csm
