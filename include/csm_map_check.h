/*
 * csm_map_check.h — C-ABI of the batched map check: MapCheckPenalize for many
 * poses on one map in one launch.
 *
 * Reference: SlamProcessor::ScanMatchInterface multiplies every scan-match
 * response by MapCheckPenalize(pub_map_range_data, best_pose, true) and clamps
 * to 1 (slam/slam_processor.cpp:312-317, :573-595) before TryCloseLoop and
 * LinkNearChains compare it with their thresholds
 * (pose_graph/range_scan_pose_graph.cpp:159,322,333). The check itself is
 * OccuGridMap::MapFeedbackResponsePenalty (map/occu_grid_map.h:331-392) with
 * CheckOccuLineVisitorCallback (:447-471): a Bresenham line from the sensor
 * cell to every checked beam's end cell through the PubMap, counting the beams
 * that cross an occupied cell farther than bound_tolerance cells from their
 * end. csm_gridmap_feedback_penalty (csm_gridmap.h) is one such call; the
 * entry points here answer n_poses of them with one upload, one launch and one
 * synchronise. Every coefficient equals the single call's bit for bit.
 *
 * The sensor origin is (0, 0), as roborts_slam_node.cpp:293 sets it for every
 * scan. Paths are relative to the reference repository root.
 */
#ifndef ROBORTS_CSM_MAP_CHECK_H
#define ROBORTS_CSM_MAP_CHECK_H

#include <stdint.h>

#include "csm_chain_maps.h"
#include "csm_gridmap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* map_check_point_num / map_check_bound_tolerance / map_check_penalty_gain
 * (slam_processor.cpp:584-586); use_blur is MapFeedbackResponsePenalty's last
 * argument (occu_grid_map.h:334; MapCheckPenalize passes false, :587);
 * use_logistic is MapCheckPenalize's (:589-591). */
typedef struct csm_map_check_param {
  int32_t check_point_num, use_blur, use_logistic, reserved;
  double bound_tolerance, penalty_gain;
} csm_map_check_param;

/* n_poses MapCheckPenalize calls on one map (slam_processor.cpp:573-595 ->
 * occu_grid_map.h:331-392). Scans as CSR in metres (sensor frame, before CreateFrom;
 * the map's own 1/resolution is applied on the device); pose k checks scan scan_index[k]
 * (NULL: scan k, n_poses == n_scans). coeff[k]: the penalty (after the logistic when use_logistic);
 * counts[k] (may be NULL): the rays that hit, -1 for a pose outside the map (coefficient 0.0).
 * With arguments the reference's guard (:337-341) answers, every penalty is 1.0, every
 * count 0 and nothing is launched; the logistic, when asked for, applies to every
 * penalty, the guard's 1.0 and an outside pose's 0.0 included, as :589-591 does.
 * check_point_num == 1 with a checked scan of two points or more (:368 divides by zero),
 * a scan_index outside the scans, offsets that decrease or a scan of 2^31 points and more:
 * CSM_ERR_INVALID_ARG before any launch. n_poses == 0 is CSM_OK. */
int csm_gridmap_feedback_penalty_batch(csm_gridmap* map, int32_t n_scans, const double* points_m,
                                       const int64_t* point_offsets, int32_t n_poses, const int32_t* scan_index,
                                       const double* poses, const csm_map_check_param* param,
                                       double* coeff, int32_t* counts);
/* The same (occu_grid_map.h:331-392) with the scans read from a resident store on the
 * map's device: no points cross the bus. Pose k checks the kept scan scan_ids[k] at poses[3k..3k+2]
 * (the store's own poses are not read). A store on another device or an id of no kept
 * scan: CSM_ERR_INVALID_ARG. */
int csm_gridmap_feedback_penalty_store(csm_gridmap* map, csm_scan_store* store, int32_t n_poses,
                                       const int32_t* scan_ids, const double* poses,
                                       const csm_map_check_param* param, double* coeff, int32_t* counts);

/* Diagnostics (no reference counterpart). *launches: the batch kernel's launches on
 * this map since it was made (one per batch or store call that got past the guard). */
int csm_gridmap_map_check_launches(csm_gridmap* map, int64_t* launches);
/* The batch kernel of that store call alone (occu_grid_map.h:372-385 for every pose):
 * `repeats` launches back to back on the map's stream between two HIP events;
 * *ms = their mean time. These launches are not counted above. Arguments the guard
 * answers launch nothing: CSM_ERR_INVALID_ARG. */
int csm_gridmap_feedback_penalty_store_kernel_ms(csm_gridmap* map, csm_scan_store* store, int32_t n_poses,
                                                 const int32_t* scan_ids, const double* poses,
                                                 const csm_map_check_param* param, int32_t repeats, double* ms);

#ifdef __cplusplus
}
#endif

#endif /* ROBORTS_CSM_MAP_CHECK_H */
