/*
 * csm_gridmap.h — C-ABI of the device-resident occupancy-grid maps that the
 * correlative scan matcher reads (map building; row f4:
 * the post-match map check).
 *
 * A csm_gridmap is one OccuGridMap<ProbabilityCell> (the reference's
 * ScanMatchMap) or OccuGridMap<CountCell> (its PubMap) whose cells live in
 * HBM as separate arrays (prob, pass, hit, update_index). Geometry, bound box
 * and update counters are mirrored on the host, where the reference's
 * per-scan bookkeeping runs; every per-cell update is a HIP kernel.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repository root):
 *
 *   csm_gridmap_create        OccuGridMap(resolution, size, offset, deviation,
 *                             default_cell_prob)        map/occu_grid_map.h:201-217
 *                             (GaussianBlur kernel :38-115, AllocateGridCell
 *                             map/grid_map_base.h:152-166)
 *   csm_gridmap_set_options   set_use_auto_map_resize / set_just_update_occu /
 *                             set_cell_occu_prob_offset  occu_grid_map.h:429-439,
 *                             set_extend_factor          grid_map_base.h:175-179
 *   csm_gridmap_set_cell_params  SetUpdateFreeFactor / SetUpdateOccupiedFactor /
 *                             SetOccuThreshold / SetMinPassThrough  occu_grid_map.h:413-427
 *   csm_gridmap_set_map_offset   GridMapBase::set_map_offset  grid_map_base.h:275-279
 *   csm_gridmap_reset         GridMapBase::Reset               grid_map_base.h:95-103
 *   csm_gridmap_update_bound  GridMapBase::UpdateBound (may ExtendSize)  grid_map_base.h:247-264
 *                             (called by ScanMatchers::MapSizeCheck, scan_matchers.h:365-390)
 *   csm_gridmap_update_by_range  OccuGridMap::UpdateMapByRange occu_grid_map.h:258-329
 *   csm_gridmap_init_with_range_vec  OccuGridMap::InitMapWithRangeVec  occu_grid_map.h:222-255
 *                             (with use_reset_speedup: ResetValueSpeedup grid_map_base.h:112-117)
 *   csm_gridmap_feedback_penalty OccuGridMap::MapFeedbackResponsePenalty occu_grid_map.h:331-392
 *   csm_gridmap_info / csm_gridmap_download   GridMapBase getters and GetCell reads
 *   csm_gridmap_states / csm_gridmap_occupancy_grid*   GetGridStates over a box, and the
 *                             box, size and origin of SlamNode::PublishMapThread
 *                             (roborts_slam_node.cpp:355-488; see "the map publisher" below)
 *   csm_set_grid_gridmap      the scan matcher reads this map's probabilities
 *                             (ScanMatchers::ScanMatch on fine_map, scan_matchers.h:238-256)
 *
 * Points are RangeDataContainer contents after CreateFrom(raw, 1/resolution)
 * (slam/sensor_data_manager.h:99-115): map-cell units, sensor frame. Poses are
 * world (x, y, theta) in metres / radians.
 *
 * Update modes (as the reference uses them):
 *   just_update_occu + blur    ScanMatchMaps (slam_processor.cpp:493-510,458): each
 *                              endpoint raises its blur kernel's cells (max);
 *   just_update_occu, no blur  each hit cell is set occupied once per scan;
 *   full (lines), no blur      PubMap: Bresenham free marking + occupied endpoints.
 *   full + blur is order-dependent in the reference and never used by it; it
 *   returns CSM_ERR_UNSUPPORTED. ProbabilityCell supports all three modes,
 *   CountCell the two without blur.
 *
 * Every result (cells, update indices, touched-cell set, bound box, offset,
 * size after growth) equals the reference's sequential code bit for bit.
 * Calls are ordered on the map's own HIP stream; csm_set_grid_gridmap makes
 * the matcher's stream wait for the map's last update.
 */
#ifndef ROBORTS_CSM_GRIDMAP_H
#define ROBORTS_CSM_GRIDMAP_H

#include <stdint.h>

#include "csm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum csm_cell_kind {
  CSM_PROBABILITY_CELL = 0, /* ProbabilityCell (grid_map_cell.h:301-388): ScanMatchMap */
  CSM_COUNT_CELL = 1        /* CountCell (grid_map_cell.h:42-161): PubMap */
};

typedef struct csm_gridmap csm_gridmap;

/* Geometry and counters of a map. */
typedef struct csm_gridmap_state {
  double resolution;        /* GetCellLength()                                   */
  double offset_x, offset_y;/* map_offset_                                       */
  double bound_min_x, bound_min_y, bound_max_x, bound_max_y; /* bound_box_       */
  int32_t size_x, size_y;
  int32_t map_update_index; /* map_update_index_ (IsMapInit: >= 0)               */
  int32_t cur_update_index; /* OccuGridMap::cur_update_index                      */
  int32_t half_kernel;      /* GaussianBlur half kernel (0: blur invalid)         */
  int32_t blur_states;
  int32_t kind;             /* enum csm_cell_kind                                */
  int32_t reserved;
  double scale_factor;      /* scale_factor_ = 1/resolution as constructed         */
} csm_gridmap_state;

int csm_gridmap_create(int device, int32_t kind, double resolution, int32_t size_x, int32_t size_y,
                       double offset_x, double offset_y, double deviation, float default_cell_prob,
                       csm_gridmap** out);
int csm_gridmap_destroy(csm_gridmap* map);
const char* csm_gridmap_last_error(const csm_gridmap* map);

int csm_gridmap_set_options(csm_gridmap* map, int32_t use_auto_map_resize, int32_t just_update_occu,
                            double cell_occu_prob_offset, double extend_factor);
/* occu_threshold and min_pass apply to CountCell only (ProbabilityCell's setters are no-ops). */
int csm_gridmap_set_cell_params(csm_gridmap* map, float update_free_factor, float update_occu_factor,
                                float occu_threshold, float min_pass);
int csm_gridmap_set_map_offset(csm_gridmap* map, double offset_x, double offset_y);
int csm_gridmap_reset(csm_gridmap* map);
/* *inside = UpdateBound's return value (0: the map grew to hold the box). */
int csm_gridmap_update_bound(csm_gridmap* map, double min_x, double min_y, double max_x, double max_y,
                             int32_t* inside);

/* *updated = UpdateMapByRange's return value (0 when the scan made the map grow). */
int csm_gridmap_update_by_range(csm_gridmap* map, const double* points_xy, int32_t n_points,
                                const double origin[2], const double sensor_pose[3], int32_t use_blur,
                                int32_t* updated);
/* scans: point_offsets has n_scans+1 prefix offsets into points_xy; origins
 * n_scans*2 (null: all zero, as roborts_slam_node.cpp:293 sets), poses n_scans*3. */
int csm_gridmap_init_with_range_vec(csm_gridmap* map, int32_t n_scans, const double* points_xy,
                                    const int64_t* point_offsets, const double* origins,
                                    const double* sensor_poses, int32_t use_blur, int32_t use_reset_speedup);
int csm_gridmap_feedback_penalty(csm_gridmap* map, const double* points_xy, int32_t n_points,
                                 const double origin[2], const double best_pose[3], int32_t check_point_num,
                                 double bound_tolerance, double penalty_gain, int32_t use_blur,
                                 double* response_coeff);

int csm_gridmap_get_state(csm_gridmap* map, csm_gridmap_state* out);
/* Copy cells to the host (size_y*size_x each; any pointer may be null).
 * touched: 1 where map_update_point_ holds the linear index. */
int csm_gridmap_download(csm_gridmap* map, float* prob, float* pass_count, float* hit_count,
                         int32_t* update_index, uint8_t* touched);
/* Device pointer of the probability array (row-major y*size_x + x). Valid
 * until the next call that grows or destroys the map. */
int csm_gridmap_device_prob(csm_gridmap* map, const float** device_prob);

/* ---- the map publisher ---------------------------------------------------
 * What SlamNode::PublishMapThread (roborts_slam_node.cpp:355-488) computes of
 * a nav_msgs::OccupancyGrid, without the ROS message: the cells' states
 * (100 occupied, 0 free, -1 unknown), classified on the device, and the
 * grid's origin, resolution, width and height. */
typedef struct csm_occupancy_grid_info {
  double origin_x, origin_y, resolution;   /* map_.info.origin.position, .resolution */
  int32_t width, height;                   /* map_.info.width / .height               */
  int32_t start_x, start_y;                /* first cell of the box                   */
  int32_t map_update_index;                /* the map state the grid shows            */
  int32_t reserved;
} csm_occupancy_grid_info;

/* GetGridStates(x, y) (map/occu_grid_map.h -> CountCellFunctions::GetGridStates
 * map/grid_map_cell.h:125-136, ProbabilityCellFunctions:: :367-375) of the
 * cells (x0 + i, y0 + j), i < w, j < h, as the node's loop writes them
 * (roborts_slam_node.cpp:444-469): out[j * w + i], copied to the host before
 * the call returns. The cell is GetCell(x, y), linear index y * size_x + x
 * (grid_map_base.h:315-317), so x = size_x reads the next row's first cell;
 * a negative x or y, or an index past the array, gives -1. Negative w or h
 * and w * h >= 2^31 are CSM_ERR_INVALID_ARG; w * h == 0 does nothing. */
int csm_gridmap_states(csm_gridmap* map, int32_t x0, int32_t y0, int32_t w, int32_t h, int8_t* out);
/* The published grid's geometry alone (a caller sizes its buffer from it).
 * full_map = 0: the bound box, GetStartGrid .. GetEndGrid with both ends
 * (grid_map_base.h:319-328), GetBoundSizeX/Y (util/boundbox.h:99-111), origin
 * GetWorldCoords(GetStartGrid()) - GetCellLength() / 2
 * (roborts_slam_node.cpp:427-436); a bound box never set gives 0 x 0 at
 * start (0, 0). full_map != 0: kDisplayFullMap (:391-404), every cell, origin
 * from GetWorldCoords(0, 0). */
int csm_gridmap_occupancy_grid_info(csm_gridmap* map, int32_t full_map, csm_occupancy_grid_info* info);
/* Start one grid: under the map's lock, the info as above, the states kernel
 * on the map's stream and one device-to-host copy into a pinned buffer the map
 * owns; returns without waiting for either. The map's later updates run on
 * the same stream, so the grid is the state info->map_update_index names
 * whatever is enqueued after it. A second _begin before _end waits for the
 * first. */
int csm_gridmap_occupancy_grid_begin(csm_gridmap* map, int32_t full_map, csm_occupancy_grid_info* info);
/* Wait for the grid _begin started (outside the map's lock: updates of the
 * map go on meanwhile) and hand out the map's buffer, height * width bytes,
 * valid until the next _begin on this map or its destruction. Without a
 * _begin: CSM_ERR_INVALID_ARG. */
int csm_gridmap_occupancy_grid_end(csm_gridmap* map, const int8_t** data);
/* _begin, _end and a copy into data (the whole of roborts_slam_node.cpp:
 * 386-471 for one map). capacity < width * height: CSM_ERR_INVALID_ARG, info
 * filled, data untouched. */
int csm_gridmap_occupancy_grid(csm_gridmap* map, int32_t full_map, csm_occupancy_grid_info* info, int8_t* data,
                               int64_t capacity);

/* Diagnostics (no reference counterpart): the states kernel of that grid alone,
 * `repeats` launches back to back on the map's stream between two HIP events;
 * *ms = their mean time. An empty grid is CSM_ERR_INVALID_ARG. */
int csm_gridmap_occupancy_grid_kernel_ms(csm_gridmap* map, int32_t full_map, int32_t repeats, double* ms);

/* Point the scan matcher at this map (borrowed, like csm_set_grid_device):
 * size, resolution, offset and update index come from the map.
 * Ordering, both ways: the matcher's work runs after the map's last update,
 * and the map's later updates (update_by_range, reset, init, update_bound)
 * wait for every match or copy already enqueued on that matcher context, so
 * a map may be updated right after set_grid returns, from any thread. */
int csm_set_grid_gridmap(csm_ctx* ctx, csm_gridmap* map);

/* Make n maps of one size, resolution and offset resident as a grid stack
 * (device-to-device copies ordered after each map's last update); scans then
 * name their map with csm_scan_matchers_batch_grids. Replaces the grid. */
int csm_set_grid_stack_gridmaps(csm_ctx* ctx, csm_gridmap* const* maps, int32_t n_maps);

#ifdef __cplusplus
}
#endif

#endif /* ROBORTS_CSM_GRIDMAP_H */
