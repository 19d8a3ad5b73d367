// csm_chain_maps.hpp — the host plan of a stack of chain maps
// (include/csm_chain_maps.h), stated once and free of HIP calls: the driver
// (csm_chain_maps.cpp) uploads what plan_chains returns, the kernels
// (csm_chain_maps.hip) read it, tests/cpp/chain_plan_check.cpp checks it
// against a restatement on the host alone.
//
//   arguments   what csm_set_grid_stack_chains rejects, and with which status
//   kernel      GaussianBlur's table (occu_grid_map.h:40-105) as
//               csm_gridmap_create computes it, narrowed as upload_ktab does:
//               (float)(kernel * cell_occu_prob_offset_) (:567)
//   placements  one per (grid, chain position): the scan's point range and the
//               map-frame pose of GetMapCoordsPose (grid_map_base.h:89-93) with
//               the host's sincos, the arithmetic of update_by_range
//               (csm_gridmap.cpp)
//
// Compiled with -ffp-contract=off like every host unit: each double
// expression rounds as the reference's does.
#pragma once

#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "csm_chain_maps.h"
#include "host_math.hpp"

namespace csm {

// A kept scan as the store holds it on the host: where its points start in the
// store's device buffer (in points), how many, and its sensor pose.
struct ChainScan {
  int64_t pt_begin = 0;
  int32_t n_points = 0;
  double pose[3] = {0.0, 0.0, 0.0};
};

// A store as another unit reads it in place (the map check, csm_gridmap.cpp):
// its device, its points buffer (x, y in metres, back to back) and its scans.
struct ScanStoreView {
  int device = 0;
  const double* pts = nullptr;
  const ChainScan* scans = nullptr;
  int32_t n_scans = 0;
};
// Locks the store and fills the view, valid while the returned lock lives: no
// scan is added and the buffer is not replaced meanwhile, so a reader that
// drains its stream before it lets go never outlives the buffer.
std::unique_lock<std::mutex> scan_store_lock(csm_scan_store* s, ScanStoreView* v);

// One scan drawn into one grid. 48 bytes, read by the splat kernel as it is.
struct ChainPlacement {
  int64_t pt_begin;  // first point in the store's buffer
  int32_t n_points;
  int32_t grid;      // grid of the stack
  double c, s;       // cos / sin of the scan's pose angle
  double tx, ty;     // the pose's position in map cells
};
static_assert(sizeof(ChainPlacement) == 48, "the kernel reads placements as the host wrote them");

struct ChainPlan {
  int half_kernel = 0;
  std::vector<float> ktab;  // (2 hk + 1)^2 values, index (i + hk) + ks * (j + hk)
  std::vector<ChainPlacement> place;
  int32_t update_index = -1;  // min over grids of (chain length) - 1
  int32_t max_points = 0;     // most points of any placement
};

// GaussianBlur accepts the deviation (occu_grid_map.h:47: otherwise blur_states_ stays false)
inline bool chain_blur_ok(double resolution, double deviation) {
  return deviation > 0.5 * resolution && deviation < 10 * resolution && resolution > 0;
}

// half_kernel_size_ and the kernel values times the offset, narrowed to float
inline void chain_kernel_table(double resolution, double deviation, double offset, int* half_kernel,
                               std::vector<float>& ktab) {
  const int hk = (int)((deviation / resolution) * std::sqrt(std::log(2)));
  const int ks = 2 * hk + 1;
  ktab.assign((size_t)ks * ks, 0.0f);
  for (int i = -hk; i <= hk; ++i)
    for (int j = -hk; j <= hk; ++j) {
      const double d = std::hypot(i * resolution, j * resolution);
      const double q = d / deviation;
      const double kernel = std::exp(-0.5 * (q * q));
      ktab[(size_t)((i + hk) + ks * (j + hk))] = (float)(kernel * offset);
    }
  *half_kernel = hk;
}

// The map-frame pose of a scan (GetMapCoordsPose) and its sincos.
inline void chain_place(const csm_chain_map_param& mp, const double map_offset[2], const ChainScan& sc, int32_t grid,
                        ChainPlacement* p) {
  const double s = 1.0 / mp.resolution;  // scale_factor_ (grid_map_base.h:50)
  p->pt_begin = sc.pt_begin;
  p->n_points = sc.n_points;
  p->grid = grid;
  p->tx = s * sc.pose[0] + s * map_offset[0];
  p->ty = s * sc.pose[1] + s * map_offset[1];
  host_sincos(sc.pose[2], &p->s, &p->c);
}

// The plan of a call, or the status it fails with (CSM_ERR_INVALID_ARG,
// CSM_ERR_UNSUPPORTED) and why. Invalid arguments are reported before
// unsupported modes.
inline int plan_chains(const csm_chain_map_param* mp, int32_t n_grids, const int32_t* chain_offsets,
                       const int32_t* chain_ids, const double map_offset[2], const ChainScan* scans, int32_t n_scans,
                       ChainPlan* plan, std::string* err) {
  if (!mp || !chain_offsets || !map_offset || !plan || !err) {
    if (err) *err = "chain maps: null argument";
    return CSM_ERR_INVALID_ARG;
  }
  if (n_grids < 1) {
    *err = "chain maps: n_grids < 1";
    return CSM_ERR_INVALID_ARG;
  }
  if (mp->size_x <= 0 || mp->size_y <= 0 || !(mp->resolution > 0.0)) {
    *err = "chain maps: grid size and resolution must be positive";
    return CSM_ERR_INVALID_ARG;
  }
  if (chain_offsets[0] != 0) {
    *err = "chain maps: chain_offsets[0] must be 0";
    return CSM_ERR_INVALID_ARG;
  }
  for (int32_t g = 0; g < n_grids; ++g)
    if (chain_offsets[g + 1] < chain_offsets[g]) {
      *err = "chain maps: chain_offsets decrease at grid " + std::to_string(g);
      return CSM_ERR_INVALID_ARG;
    }
  const int32_t n_place = chain_offsets[n_grids];
  if (n_place > 0 && !chain_ids) {
    *err = "chain maps: null chain_ids";
    return CSM_ERR_INVALID_ARG;
  }
  for (int32_t k = 0; k < n_place; ++k)
    if (chain_ids[k] < 0 || chain_ids[k] >= n_scans) {
      *err = "chain maps: chain_ids[" + std::to_string(k) + "] = " + std::to_string(chain_ids[k]) +
             " is no kept scan of the store";
      return CSM_ERR_INVALID_ARG;
    }
  if (!mp->use_blur) {
    *err = "chain maps: use_blur == 0 (SetCellOccu counts the scans that hit a cell: build it per map, csm_gridmap)";
    return CSM_ERR_UNSUPPORTED;
  }
  if (!chain_blur_ok(mp->resolution, mp->deviation)) {
    *err = "chain maps: deviation outside GaussianBlur's range (0.5 resolution, 10 resolution): the reference "
           "draws SetCellOccu (build it per map, csm_gridmap)";
    return CSM_ERR_UNSUPPORTED;
  }
  chain_kernel_table(mp->resolution, mp->deviation, mp->gaussian_blur_offset, &plan->half_kernel, plan->ktab);
  plan->place.resize((size_t)n_place);
  plan->max_points = 0;
  int32_t min_len = INT32_MAX;
  for (int32_t g = 0; g < n_grids; ++g) {
    const int32_t len = chain_offsets[g + 1] - chain_offsets[g];
    if (len < min_len) min_len = len;
    for (int32_t k = chain_offsets[g]; k < chain_offsets[g + 1]; ++k) {
      const ChainScan& sc = scans[chain_ids[k]];
      chain_place(*mp, map_offset, sc, g, &plan->place[(size_t)k]);
      if (sc.n_points > plan->max_points) plan->max_points = sc.n_points;
    }
  }
  plan->update_index = min_len - 1;
  return CSM_OK;
}

}  // namespace csm
