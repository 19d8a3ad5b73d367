// csm_chain_maps_launch.hpp — the launchers of csm_chain_maps.hip, called by
// the driver (csm_chain_maps.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "csm_chain_maps.hpp"

namespace csm {

// Bytes of the hit mask of n_cells cells: a byte a cell, in whole dwords.
inline size_t chain_hits_bytes(int64_t n_cells) { return ((size_t)n_cells + 3) & ~(size_t)3; }

// Every cell of n_cells (n_grids grids back to back) = value, and their hit
// mask (chain_hits_bytes(n_cells), 4-byte aligned) cleared.
hipError_t launch_chain_fill(float* grids, uint8_t* hits, int64_t n_cells, float value, hipStream_t s);

// The placements' scans drawn into their grids through the hit mask: pts the
// store's points (raw metres, x then y), inv_res = 1 / resolution, ktab
// (2 hk + 1)^2 floats on the device, max_points the most points of any
// placement. After launch_chain_fill on the same stream.
hipError_t launch_chain_splat(const ChainPlacement* place, int32_t n_place, int32_t max_points, const double* pts,
                              double inv_res, float* grids, uint8_t* hits, int64_t n_cells, int32_t size_x,
                              int32_t size_y, int32_t hk, const float* ktab, hipStream_t s);

}  // namespace csm
