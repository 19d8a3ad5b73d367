/*
 * csm_loop_closure.h — C-ABI of the sharded loop-closure search (SURVEY.md 8e,
 * BASELINE config 3): one query scan against many submaps, the submaps
 * sharded over the GPUs of ONE process, the best candidate agreed over RCCL.
 *
 * Reference: the pose-graph back end closes loops by matching a scan against
 * the map around older chain candidates, one ScanMatchInterface call at a
 * time (pose_graph/range_scan_pose_graph.cpp:299-355 TryCloseLoop, :120-167
 * LinkNearChains -> slam/slam_processor.cpp:301 -> ScanMatchers::ScanMatch).
 * This entry point is what TryCloseLoop can call from C++ instead: every
 * submap window in one search per device, no Python, no torch.
 *
 *   devices            submaps [r*S/G, (r+1)*S/G) resident on device r only
 *                      (csm_set_grid_stack of that device's context)
 *   search             per device: csm_search_windows (admissible multi-
 *                      resolution branch and bound) or the exhaustive
 *                      csm_best_windows, run concurrently from host threads
 *   exchange           three ncclAllReduce over one communicator per device
 *                      (ncclCommInitAll, in-process): MAX of the 8-byte score,
 *                      MIN of the 8-byte global index among devices holding
 *                      that score, SUM of the winner's one-hot (submap, x, y,
 *                      angle) row; the selections between them run as tiny
 *                      device kernels, so the host waits once, at the end
 *
 * global index = submap * n_cand + flat index (reference enumeration order);
 * the result is what one device holding every submap returns (max score,
 * lowest global index), whatever the device count.
 *
 * RCCL is loaded at csm_loop_closure_create (dlopen of librccl.so.1, private
 * symbols), so the matcher library itself does not depend on it.
 */
#ifndef ROBORTS_CSM_LOOP_CLOSURE_H
#define ROBORTS_CSM_LOOP_CLOSURE_H

#include <stdint.h>

#include "csm.h"
#include "csm_chain_maps.h"
#include "csm_map_check.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct csm_loop_closure csm_loop_closure;

typedef struct csm_loop_closure_result {
  double score;           /* best response (-DBL_MAX: no submap)                  */
  int64_t global_index;   /* submap * n_cand + flat index; -1: nothing scored     */
  int32_t submap;
  int32_t n_devices;
  double x, y, angle;     /* candidate pose in the submap's map cells / rad       */
  double pose_world[3];   /* the same pose in world coordinates (GetWorldCoordsPose,
                             grid_map_base.h:83-87, with the submap's offset)      */
  double search_ms;       /* host wall time of the concurrent per-device searches */
  double exchange_ms;     /* host wall time of the exchange: staging up, the three
                             all-reduces and two selections, result down, every
                             stream drained                                         */
} csm_loop_closure_result;

enum csm_loop_closure_search { CSM_LC_PYRAMID = 0, CSM_LC_EXHAUSTIVE = 1 };

/* n_devices HIP devices (devices == NULL: 0 .. n_devices-1), one matcher
 * context and one RCCL communicator each. */
int csm_loop_closure_create(int32_t n_devices, const int32_t* devices, csm_loop_closure** out);
int csm_loop_closure_destroy(csm_loop_closure* lc);
const char* csm_loop_closure_last_error(const csm_loop_closure* lc);

/* The submaps: n_submaps packed fp32 grids of one size (host memory,
 * n_submaps * size_y * size_x floats, kept alive by the caller while
 * resident), info->resolution their cell length, offsets[2i..2i+1] submap
 * i's map_offset_ (m). version as csm_set_grid_stack (unchanged: no upload). */
int csm_loop_closure_set_submaps(csm_loop_closure* lc, const float* cells, int32_t n_submaps,
                                 const csm_map_info* info, const double* offsets, int64_t version);

/* The submaps drawn on the devices from chains of kept scans
 * (csm_chain_maps.h) instead of uploaded: what TryCloseLoop and LinkNearChains
 * need per query, since ScanMatchInterface (slam/slam_processor.cpp:250-326)
 * rebuilds each chain's map at the poses the pose graph holds at that moment.
 * add_scan keeps a scan (its end points in metres and its sensor pose) on
 * every device -- the scans are small, the stores replicated -- and returns
 * id = 0, 1, ...; set_scan_pose is UpdateRangeData after a graph solve. */
int csm_loop_closure_add_scan(csm_loop_closure* lc, const double* points_m, int32_t n_points, const double sensor_pose[3], int32_t* id);
int csm_loop_closure_set_scan_pose(csm_loop_closure* lc, int32_t id, const double sensor_pose[3]);
/* Submap i = the chain's map centred on current_pose: map_offset = -(current_pose - 0.5 * size * resolution), :452-454
 * Device r draws only its shard [r*S/G, (r+1)*S/G) (csm_set_grid_stack_chains
 * on its context), the devices concurrently; every submap's offset is equal,
 * and the match entry points below run unchanged. Arguments and statuses as
 * csm_set_grid_stack_chains. A failed call leaves no submaps, as a failed
 * csm_loop_closure_set_submaps. */
int csm_loop_closure_set_submaps_chains(csm_loop_closure* lc, const csm_chain_map_param* mp, int32_t n_submaps,
                                        const int32_t* chain_offsets, const int32_t* chain_ids, const double current_pose[3]);

/* One query: points_xy in map cells (sensor frame, as csm_scan_match), the
 * window param (e.g. +-8 m / +-pi at one-cell steps), pose_world the centre
 * of every submap's window. search: enum csm_loop_closure_search. */
int csm_loop_closure_match(csm_loop_closure* lc, const double* points_xy, int32_t n_points,
                           const csm_param* param, const double pose_world[3], int32_t search,
                           csm_loop_closure_result* result);

/* csm_loop_closure_match, then the full ScanMatch result of the winning
 * submap's window -- what TryCloseLoop gates on and hands to LinkChainToScan
 * (pose_graph/range_scan_pose_graph.cpp:299-355: response, covariance(0,0) and
 * (1,1), best_pose, covariance). The match and the exchange run unchanged;
 * then the device that holds the winning submap runs csm_search_match on that
 * one window of its resident stack (default options; the pooled levels are
 * cached there). result: every field as csm_loop_closure_match fills it,
 * except pose_world = GetWorldCoordsPose (grid_map_base.h:83-87) of
 * match->pose_map, FindBestCandidate's averaged pose
 * (correlate_scan_matcher.h:670-710), with the submap's offset. match->window
 * is the submap. cov: row-major 3x3 in/out, as csm_search_match writes it.
 * The finish runs with collect_capacity = CSM_COLLECT_AUTO: a loop-closure
 * window holds far more than 10240 candidates at or above the threshold, and
 * the default capacity sent every such call through the exhaustive path 2.
 * The outputs are the same bits either way; match->path and the time differ.
 * param->type == CSM_FAST: CSM_ERR_INVALID_ARG. */
int csm_loop_closure_match_full(csm_loop_closure* lc, const double* points_xy, int32_t n_points,
                                const csm_param* param, const double pose_world[3], int32_t search,
                                double cov[9], csm_loop_closure_result* result, csm_match_result* match);

/* Every submap at or above a response, not only the best: TryCloseLoop
 * (:299-355) gates each candidate chain on its own response and links every
 * one that passes, LinkNearChains (:120-167) likewise. Every device runs
 * csm_search_gated (csm.h) on its shard concurrently; there is no collective:
 * the answer is per submap and the shards are disjoint contiguous ranges, so
 * the host concatenates them. results[k], k < min(*n_pass, capacity), in
 * ascending submap order, each filled as csm_loop_closure_match fills the
 * winner's (score, global_index, submap, n_devices, x / y / angle, pose_world;
 * search_ms the concurrent phase, exchange_ms 0); *n_pass counts every submap
 * whose best score is >= min_response (unclamped, inclusive). The result does
 * not depend on the device count. capacity == 0 only counts. NaN min_response,
 * capacity < 0 or param->type == CSM_FAST: CSM_ERR_INVALID_ARG. */
int csm_loop_closure_match_gated(csm_loop_closure* lc, const double* points_xy, int32_t n_points,
                                 const csm_param* param, const double pose_world[3], double min_response,
                                 csm_loop_closure_result* results, int32_t capacity, int32_t* n_pass);

/* csm_loop_closure_match_gated, then for each written entry the full ScanMatch
 * result of that submap's window, exactly as csm_loop_closure_match_full's
 * second half (csm_search_match with CSM_COLLECT_AUTO on the device that holds
 * the submap): matches[k], covs[9k..9k+8] (in/out per entry, as
 * csm_search_match writes it), results[k].pose_world the averaged pose's world
 * coordinates. Devices finish in parallel, a device's own submaps in order. */
int csm_loop_closure_match_gated_full(csm_loop_closure* lc, const double* points_xy, int32_t n_points,
                                      const csm_param* param, const double pose_world[3], double min_response,
                                      csm_loop_closure_result* results, int32_t capacity, int32_t* n_pass,
                                      double* covs, csm_match_result* matches);

/* The reference's gate on a gated result: TryCloseLoop and LinkNearChains compare
 * response * MapCheckPenalize(pub range data, best_pose, true), clamped to 1
 * (slam/slam_processor.cpp:312-317, :573-595; range_scan_pose_graph.cpp:159,322,333).
 * penalties[k] = that penalty of the kept scan scan_id at results[k].pose_world, k < n,
 * on pub_map: csm_gridmap_feedback_penalty_store (csm_map_check.h) over this handle's
 * store on pub_map's device, one launch for all n. Only penalties is written: the
 * score the reference multiplies it with is the mean of three levels, which
 * csm_loop_closure_scan_match (below) computes, penalty and clamp included.
 * CSM_ERR_INVALID_ARG when none of the handle's devices is the map's, or scan_id is
 * no kept scan. */
int csm_loop_closure_map_check(csm_loop_closure* lc, csm_gridmap* pub_map, int32_t scan_id,
                               const csm_map_check_param* param, const csm_loop_closure_result* results,
                               int32_t n, double* penalties);

/* SlamProcessor::ScanMatchInterface (slam/slam_processor.cpp:250-326) for every
 * gated submap: the number TryCloseLoop and LinkNearChains compare with their
 * thresholds (pose_graph/range_scan_pose_graph.cpp:153,312,329), with the pose
 * and covariance the call leaves. The Gauss-Newton matcher is off, as both
 * reference YAMLs have it (with it on, csm_backend.h remains). */
typedef struct csm_loop_closure_interface_param {
  csm_param levels[3];          /* the ScanMatchParam set of the call; levels[0] is the (wide) coarse window   */
  int32_t use_fine_scan_match;  /* ScanMatchInterface's argument (scan_matchers.h:247)                          */
  int32_t use_map_check;        /* 0: penalty 1, pub_map may be NULL                                            */
  double range_max;             /* the range finder's, for MapSizeCheck (scan_matchers.h:365-390)               */
  double min_response;          /* gate on level 0's unclamped best, inclusive, as csm_loop_closure_match_gated */
  csm_map_check_param check;    /* use_logistic = 1 is what ScanMatchInterface passes (:315)                    */
} csm_loop_closure_interface_param;

typedef struct csm_loop_closure_interface_result {
  int32_t submap, levels_run;   /* 1 or 3 */
  double pose[3];               /* best_pose out (world)                        */
  double cov[9];                /* cov_matrix out, row-major                    */
  double score;                 /* ScanMatchInterface's return value            */
  double response[3];           /* each level's clamped response (not run: 0)   */
  double map_penalty;
  csm_loop_closure_result wide; /* what csm_loop_closure_match_gated_full writes for this submap */
  csm_match_result wide_match;
} csm_loop_closure_interface_result;

/* The query is the kept scan scan_id (csm_loop_closure_add_scan; the handle
 * keeps its raw points on the host too): its matcher points are raw * (1 /
 * resolution) with the submaps' resolution, rounded once, as CreateFrom does
 * (sensor_data_manager.h:99-115). The submaps come from
 * csm_loop_closure_set_submaps_chains, or from csm_loop_closure_set_submaps
 * with every submap's offset equal to info->offset_x / offset_y (the fine
 * levels convert poses with the stack's one geometry; otherwise
 * CSM_ERR_UNSUPPORTED when use_fine_scan_match is set).
 *
 * For every submap whose level-0 best is >= param->min_response, results[k] is
 * what ScanMatchInterface(range_data(scan_id), ., chain k, best_pose =
 * pose_world, cov = cov_init (NULL: identity), use_fine_scan_match, .) returns
 * and writes, k < min(*n_pass, capacity), in ascending submap order; *n_pass
 * counts every passing submap. The steps:
 *   1. level 0 as csm_loop_closure_match_gated_full: the same shards, finish and
 *      paths, cov_init going in for every entry;
 *   2. the next level's start pose: the averaged pose's world coordinates when
 *      wide_match.accepted, else pose_world unchanged
 *      (correlate_scan_matcher.h:866-869);
 *   3. with use_fine_scan_match, levels 1 and 2 (scan_matchers.h:247-261): each
 *      device runs all its passers in one seeded batch over its resident stack
 *      (the driver behind csm_scan_matchers_batch_grids_seeded, first_level = 1,
 *      the clamped level-0 responses as the seed, poses and covariances as level
 *      0 left them), the devices concurrently;
 *   4. with use_map_check, MapCheckPenalize of the kept scan at every entry's
 *      final pose on pub_map: one csm_gridmap_feedback_penalty_store, the path
 *      of csm_loop_closure_map_check;
 *   5. score = min(mean * penalty, 1.0), the mean over the levels run
 *      (scan_matchers.h:281, slam_processor.cpp:316-317).
 * The strict > / < comparisons of the pose graph stay with the caller. A final
 * score above T needs a level-0 best above 3 T - 2 with three levels (every
 * response is clamped to 1 and the logistic penalty never exceeds 1), above T
 * with one: min_response = 3 T - 2 loses nothing (csrc/csm_lc_interface.hpp
 * interface_wide_gate; not with check.use_logistic = 0, whose penalty reaches
 * 1 + 2 * penalty_gain).
 *
 * MapSizeCheck cannot grow a submap here: the reference's box, pose_world in
 * map cells +- (range_max + levels[0].search_space_size) / cell length, is
 * tested against every submap with UpdateBound's criterion
 * (grid_map_base.h:247-264) before anything is launched; where the reference
 * would grow its map the call returns CSM_ERR_UNSUPPORTED and
 * csm_loop_closure_last_error names the submap size that would have fit.
 * CSM_ERR_INVALID_ARG: levels[*].type == CSM_FAST, a NaN gate, capacity < 0,
 * scan_id of no kept scan, use_map_check without a map on one of the handle's
 * devices. A failed call leaves the handle usable and its submaps resident. */
int csm_loop_closure_scan_match(csm_loop_closure* lc, csm_gridmap* pub_map, int32_t scan_id,
                                const csm_loop_closure_interface_param* param, const double pose_world[3],
                                const double cov_init[9] /* NULL: identity */,
                                csm_loop_closure_interface_result* results, int32_t capacity, int32_t* n_pass);

/* The largest min_response that loses no submap whose final score exceeds `threshold` (the caller's
 * strict >), for levels_run = 3 (3 * threshold - 2, lowered by the roundings in between) or 1
 * (threshold itself); csrc/csm_lc_interface.hpp interface_wide_gate. Holds for a penalty <= 1: the
 * logistic map check or none, not check.use_logistic = 0. Host only. */
double csm_loop_closure_wide_gate(double threshold, int32_t levels_run);

/* Borrow the matcher context of the handle's device `shard` (0 .. n_devices - 1),
 * e.g. for csm_set_profiling / csm_kernel_stats around a call (as
 * csm_backend_matcher). The handle keeps owning it. */
int csm_loop_closure_matcher(csm_loop_closure* lc, int32_t shard, csm_ctx** ctx);

#ifdef __cplusplus
}
#endif

#endif /* ROBORTS_CSM_LOOP_CLOSURE_H */
