/*
 * csm_chain_maps.h — C-ABI of the resident scan store and the stack builder:
 * the matcher's grid stack drawn on the device from chains of kept scans.
 *
 * Reference: a loop-closure or near-chain map is not a stored image.
 * SlamProcessor::ScanMatchInterface (slam/slam_processor.cpp:250-326) rebuilds
 * it for every call from the chain's kept scans at the poses the pose graph
 * holds at that moment, centred on the current sensor pose
 * (ResetScanMatchMapWithRangeVec, :448-462). Here the kept scans live on the
 * device (csm_scan_store), their poses on the host, and every submap of a
 * query is drawn straight into the matcher's grid stack by one fill and one
 * splat launch (csm_set_grid_stack_chains).
 *
 * Only the order-independent mode is built: ScanMatchMaps with
 * just_update_occu_ and the Gaussian blur (both reference YAMLs,
 * *_map_use_blur: true), where SetCellOccuBlur (map/occu_grid_map.h:531-576)
 * only ever raises a ProbabilityCell to a maximum (SetGridProbability,
 * map/grid_map_cell.h:361-365) and never writes update_index_. The result is
 * the sequential one bit for bit, in any order of scans, chains and points.
 */
#ifndef ROBORTS_CSM_CHAIN_MAPS_H
#define ROBORTS_CSM_CHAIN_MAPS_H

#include <stdint.h>

#include "csm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct csm_scan_store csm_scan_store;

int csm_scan_store_create(int device, csm_scan_store** out);
/* Waits for every stream that was handed a build reading the store. */
int csm_scan_store_destroy(csm_scan_store* s);
const char* csm_scan_store_last_error(const csm_scan_store* s);
/* SensorDataManager::AddSensorData: sensor-frame end points in metres, the sensor pose; *id = 0, 1, ...
 * points_m is free when the call returns. */
int csm_scan_store_add(csm_scan_store* s, const double* points_m, int32_t n_points, const double sensor_pose[3], int32_t* id);
int csm_scan_store_set_pose(csm_scan_store* s, int32_t id, const double sensor_pose[3]);   /* UpdateRangeData */
int csm_scan_store_count(const csm_scan_store* s, int32_t* n_scans, int64_t* n_points);

typedef struct csm_chain_map_param {
  double resolution;            /* cell length (m): GridMapBase scale 1/resolution        */
  double deviation;             /* GaussianBlur deviation (m), occu_grid_map.h:40-105     */
  double gaussian_blur_offset;  /* cell_occu_prob_offset_                                 */
  int32_t size_x, size_y;       /* cells per submap                                       */
  int32_t use_blur, reserved;
  float default_cell_prob, reserved_f;  /* kMapUnknownCellProb = 0.3f for ScanMatchMaps   */
} csm_chain_map_param;

/* Grid g of the stack = a ScanMatchMap of this geometry whose every cell holds
 * default_cell_prob (a map that has been Reset(), grid_map_base.h:95-103, as the
 * back-end maps are by CreateScanMatchMapWithRangeVec's InitMapWithRangeVec,
 * slam_processor.cpp:443 -> occu_grid_map.h:230), after
 * ResetScanMatchMapWithRangeVec (:448-462: map_offset, no auto resize,
 * just_update_occu) with the scans chain_ids[chain_offsets[g] .. chain_offsets[g+1])
 * at their stored poses, scaled by CreateFrom(raw, 1/resolution).
 *
 * Replaces the context's grid with a stack of n_grids grids that share
 * map_offset; info_out->update_index = min over g of (chain length) - 1 (an
 * empty chain is a grid of default_cell_prob alone). A failed call leaves the
 * previous grid in service.
 * CSM_ERR_INVALID_ARG: a store on another device, an id of no kept scan,
 * offsets that do not start at 0 or decrease, n_grids < 1, a non-positive
 * size or resolution. CSM_ERR_UNSUPPORTED (csm_last_error says which):
 * use_blur == 0, or a deviation outside GaussianBlur's accepted range
 * (0.5 resolution < deviation < 10 resolution) -- the reference then draws
 * SetCellOccu, whose result depends on how many distinct scans hit a cell;
 * csm_gridmap remains for that mode. */
int csm_set_grid_stack_chains(csm_ctx* ctx, csm_scan_store* store, const csm_chain_map_param* mp,
                              int32_t n_grids, const int32_t* chain_offsets, const int32_t* chain_ids,
                              const double map_offset[2], csm_map_info* info_out);
/* Test hook: grid grid_index of the resident stack (or the single grid, index 0) as size_y*size_x floats. */
int csm_grid_download(csm_ctx* ctx, int32_t grid_index, float* out, int64_t n_out);

#ifdef __cplusplus
}
#endif

#endif /* ROBORTS_CSM_CHAIN_MAPS_H */
