// csm_driver_levels.hpp — the 3-level driver with each level's responses handed out
// (csm_driver.cpp), declared once for the units that call it without the context's internals
// (csm_loop_closure.cpp) and for csm_host.hpp.
#pragma once

#include <cstdint>

#include "csm.h"

namespace csmh {

// csm_scan_matchers_batch_grids_seeded that also hands out each level's responses: level
// first_level + l's to level_resp[l * n_scans + s] (nullable; csm_loop_closure_scan_match reports
// them per level)
int scan_matchers_batch_grids_levels(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                     const int32_t* grid_index, const csm_param levels[3], int32_t first_level,
                                     int32_t use_fine, const double* score_seed, double* poses, double* covs,
                                     double* scores, double* level_resp);

}  // namespace csmh
