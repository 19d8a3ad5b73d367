// csm_gridmap_internal.hpp — types shared by the occupancy-map kernels
// (csm_gridmap.hip) and their host side (csm_gridmap.cpp). Not installed;
// include/csm_gridmap.h is the public boundary.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace csm {

enum { kGmProbability = 0, kGmCount = 1 };

// Device cell arrays of one map (pass/hit null for ProbabilityCell).
struct GmCells {
  float* prob;
  float* pass;
  float* hit;
  int32_t* uidx;
  uint8_t* touched;  // map_update_point_ as a set of linear indices
  int32_t row;       // size_x_ (row length of GetCell)
  int32_t size_x, size_y;
  // Fixed-point mirror of prob the scan matcher reads (nullable): cell (x, y)
  // at fpm[y * fpm_pitch + x] holds (prob - fpm_outside) * fpm_scale, exact
  // (csm_internal.hpp gridi layout). Kernels that write prob keep it equal.
  int32_t* fpm;
  int32_t fpm_pitch;
  float fpm_outside;
  double fpm_scale;
};

// Cell-function parameters (grid_map_cell.h).
struct GmOps {
  int32_t kind;
  float occu_factor, free_factor;
  float occu_threshold, min_pass;  // CountCell states
};

// One endpoint to draw: its cell and the scan's update indices
// (cur_mark_free_index / cur_mark_occu_index, occu_grid_map.h:272-273).
struct GmEnd {
  int32_t x, y;
  int32_t free_idx, occu_idx;
};

hipError_t gm_launch_fresh(const GmCells& C, int64_t n, float first, hipStream_t s);
hipError_t gm_launch_reset(const GmCells& C, int64_t n, float v, bool only_touched, bool clear_touched,
                           hipStream_t s);
hipError_t gm_launch_extend_copy(const GmCells& O, const GmCells& N, int gx, int gy, hipStream_t s);
hipError_t gm_launch_blur(const GmEnd* ends, int n, const GmCells& C, int hk, const float* ktab, int tol,
                          hipStream_t s);
hipError_t gm_launch_occupied(const GmEnd* ends, int n, const GmCells& C, const GmOps& P, int tol, hipStream_t s);
hipError_t gm_launch_lines(const GmEnd* ends, int n, int sx, int sy, const GmCells& C, const GmOps& P,
                           uint64_t* fkey, uint32_t* oseq, uint32_t seq, int tol, hipStream_t s);
hipError_t gm_launch_feedback(const GmEnd* ends, int n, int sx, int sy, const GmCells& C, const GmOps& P,
                              int use_blur, double occu_offset, int64_t min_d2, int* count, hipStream_t s);
// The map check of n_poses pose records (csm_map_check_plan.hpp) in one
// launch: pts the points the records index (metres, x then y), factor =
// 1 / resolution, counts[k] the rays of pose k that hit.
struct MapCheckPose;
hipError_t gm_launch_feedback_batch(const MapCheckPose* poses, int n_poses, const double* pts, double factor,
                                    const GmCells& C, const GmOps& P, int use_blur, double occu_offset,
                                    int64_t min_d2, int* counts, hipStream_t s);
// GetGridStates (100 / 0 / -1) of the box (x0, y0, w, h), row-major into
// out[h * w] (device, 4-byte aligned; w * h below 2^31). Cells are read at the
// linear index y * size_x + x; -1 for a negative x or y or an index past the array.
hipError_t gm_launch_states(const GmCells& C, const GmOps& P, int x0, int y0, int w, int h, int8_t* out,
                            hipStream_t s);

// The map's fixed-point mirror for a matcher whose off-grid value is
// `outside` (gridmap_fixed_point): ok = false when the map's values are not
// known to be exactly summable in fixed point (a line or occupied update on
// the device wrote values the host cannot bound), and the matcher converts
// the grid itself.
struct GridMapFixed {
  bool ok;
  const int32_t* fpm;
  int32_t pitch;
  int32_t exp;        // E: values are multiples of 2^-E
  double max_abs;     // max |value| (and |outside|) the map can hold
  float outside;
};

// What the scan matcher needs to borrow a map's probabilities.
struct GridMapView {
  const float* prob;
  int32_t size_x, size_y;
  double resolution, offset_x, offset_y;
  int32_t map_update_index;
  hipEvent_t ready;  // recorded after the map's last update
  int device;
};
}  // namespace csm

struct csm_gridmap;
namespace csm {
int gridmap_view(csm_gridmap* m, GridMapView* v);
// Builds (or keeps) the mirror for `outside`; the map's `ready` event covers it.
int gridmap_fixed_point(csm_gridmap* m, float outside, GridMapFixed* f);
// A matcher stream reads the map: the map's next updates wait for the work
// enqueued on it so far. drop_reader: the stream is going away.
void gridmap_add_reader(csm_gridmap* m, hipStream_t s);
// The stream stops reading the map (its context moved to another grid): the
// reads enqueued so far become a one-shot fence the next update waits for.
void gridmap_release_reader(csm_gridmap* m, hipStream_t s);
// A one-shot fence: the reads enqueued on s so far (a device-to-device copy).
void gridmap_add_read_fence(csm_gridmap* m, hipStream_t s);
// The stream goes away: every map it reads keeps a fence of its reads.
void gridmap_drop_reader(hipStream_t s);

}  // namespace csm
