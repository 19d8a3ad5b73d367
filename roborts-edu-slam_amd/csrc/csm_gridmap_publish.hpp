// csm_gridmap_publish.hpp — the host rules of the map publisher, stated once:
// which cells SlamNode::PublishMapThread (roborts_slam_node.cpp:355-488) shows
// and where it puts them in the world. Pure functions on doubles and ints: no
// HIP, no allocation (tests/cpp/publish_info_check.cpp compiles this header
// alone). Compiled like the rest of the host side (-O2 -ffp-contract=off), so
// every double expression rounds as the reference's does.
//
// Paths cited are relative to the reference root.
#pragma once

#include <cmath>
#include <cstdint>

namespace csm {

// The cells of one published grid: cell (start_x + i, start_y + j) of the map
// is byte (j, i) of a width x height grid.
struct PublishBox {
  int32_t start_x, start_y;
  int32_t width, height;
};

// BoundBox::GetSizeX / GetSizeY (util/boundbox.h:99-111) on one axis:
// ceil(max) - floor(min) + 1 cells, 0 when that difference is negative. The
// reference casts the double to int whatever it holds; a difference that is
// NaN, or a count, first cell or last cell beyond int32 is undefined there and
// defined here as 0 cells (*fits = false).
inline int32_t publish_axis_size(double min_b, double max_b, bool* fits = nullptr) {
  const double lo = std::floor(min_b), hi = std::ceil(max_b);
  const double d = hi - lo;
  const bool ok = d >= 0.0 && d + 1 <= 2147483647.0 && lo >= -2147483648.0 && hi <= 2147483647.0;
  if (fits) *fits = ok;
  if (d < 0) return 0;  // :100-102
  return ok ? static_cast<int32_t>(d + 1) : 0;
}

// The bound-box form (roborts_slam_node.cpp:420-452): GetStartGrid =
// floor(min), GetEndGrid = ceil(max) (map/grid_map_base.h:319-328), both ends
// included, so GetEndGrid may name column size_x or row size_y.
// A bound box never set (min FLT_MAX, max FLT_MIN, util/boundbox.h:38-42)
// gives 0 x 0; the reference's `int start_x = floor(FLT_MAX)` is undefined
// there, and an empty grid starts at cell (0, 0) here.
inline PublishBox publish_box(double min_x, double min_y, double max_x, double max_y) {
  PublishBox b{0, 0, 0, 0};
  b.width = publish_axis_size(min_x, max_x);
  b.height = publish_axis_size(min_y, max_y);
  if (b.width > 0 && b.height > 0) {
    b.start_x = static_cast<int32_t>(std::floor(min_x));
    b.start_y = static_cast<int32_t>(std::floor(min_y));
  }
  return b;
}

// kDisplayFullMap (roborts_slam_node.cpp:391-404): every cell of the map.
inline PublishBox publish_full_box(int32_t size_x, int32_t size_y) { return PublishBox{0, 0, size_x, size_y}; }

// map_.info.origin.position (roborts_slam_node.cpp:392-395, 427-430):
// GetWorldCoords(start) (grid_map_base.h:68-76) minus half a cell, per
// component. map_to_world_ is world_to_map_.inverse() with world_to_map_ =
// Scaling(s) * Translation(offset) (:63-66); Eigen's affine inverse is the
// 2x2 inverse (s * (1 / (s * s)) on the diagonal) and the translation
// -(A^-1 * t), t = s * offset: the expressions of Geometry::to_world
// (csm_host.hpp). GetCellLength() is 1 / scale_factor_.
inline void publish_origin(double scale_factor, double offset_x, double offset_y, int32_t start_x,
                           int32_t start_y, double* origin_x, double* origin_y) {
  const double tx = scale_factor * offset_x, ty = scale_factor * offset_y;
  const double det = scale_factor * scale_factor - 0.0 * 0.0;
  const double inv_a = scale_factor * (1.0 / det);
  const double ntx = -(inv_a * tx), nty = -(inv_a * ty);
  const double half = (1 / scale_factor) * 0.5;
  *origin_x = (inv_a * static_cast<double>(start_x) + ntx) - half;
  *origin_y = (inv_a * static_cast<double>(start_y) + nty) - half;
}

// map_.info.resolution (:385, :397, :432): GetCellLength().
inline double publish_resolution(double scale_factor) { return 1 / scale_factor; }

}  // namespace csm
