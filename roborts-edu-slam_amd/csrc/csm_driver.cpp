// csm_driver.cpp — the matching entry points: BasedCorrelationScanMatch::ScanMatch
// over a batch of scans (csm_scan_match*, csm_level.cpp) and the 3-level
// ScanMatchers driver over the resident batch (csm_scan_matchers*, synchronous
// or submitted; csm_pipeline.cpp, csm_batch.cpp).
#include "csm_driver_internal.hpp"
#include "csm_submit_order.hpp"

using namespace csmh;

namespace {

// The context's batch exchanged with a parked one for a scope, whole
// (csm_ctx::swap_batch), and exchanged back on every way out of it.
struct BorrowedBatch {
  csm_ctx* c;
  ScanBatch* b;  // null: nothing parked
  BorrowedBatch(csm_ctx* cc, ScanBatch* bb) : c(cc), b(bb) {
    if (b) c->swap_batch(*b);
  }
  ~BorrowedBatch() {
    if (b) c->swap_batch(*b);
  }
  BorrowedBatch(const BorrowedBatch&) = delete;
  BorrowedBatch& operator=(const BorrowedBatch&) = delete;
};

}  // namespace

// csm_scan_matchers_loaded once locked, nothing pending, the staged batch taken.
// The seeded form (ScanMatchers::ScanMatch after its Gauss-Newton step,
// scan_matchers.h:205-281): the levels from first_level on, each scan's running
// sum started from score_seed and the seed counted as one term of the mean.
int csmh::matchers_loaded_locked(csm_ctx* c, const csm_param all_levels[3], int32_t use_fine, double* poses,
                                 double* covs, double* scores, int32_t first_level, const double* score_seed,
                                 double* level_resp) {
  if (c->n_scans < 0) return c->fail(CSM_ERR_INVALID_ARG, "no scans loaded (csm_load_scans)");
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  const int32_t n_scans = c->n_scans;
  if (n_scans == 0) return CSM_OK;
  const double t_call = now_ms();
  c->t_call = t_call;
  if (c->profiling && c->t_exit > 0.0) c->account("host:between_calls", (float)(t_call - c->t_exit), 0.0, 0.0);
  // ScanMatchers::ScanMatch (scan_matchers.h:179-289), use_optimize = false:
  // coarse, then (use_fine) fine and super-fine, pose fed forward in place.
  std::vector<double> resp((size_t)n_scans, 0.0), sum((size_t)n_scans, 0.0);
  if (score_seed) sum.assign(score_seed, score_seed + n_scans);  // :211
  const csm_param* levels = all_levels + first_level;
  const int n_levels = use_fine ? 3 - first_level : 1;
  const int times = n_levels + (score_seed ? 1 : 0);
  int st;
  bool fast = false;
  for (int l = 0; l < n_levels; ++l) fast |= levels[l].type == CSM_FAST;
  const int32_t* grid = c->scan_grid.empty() ? nullptr : c->scan_grid.data();
  for (int32_t s = 0; grid && s < n_scans; ++s)
    if (grid[s] < 0 || grid[s] >= c->n_grids) return c->fail(CSM_ERR_INVALID_ARG, "scan grid outside the resident stack");
  if (fast && grid) return c->fail(CSM_ERR_UNSUPPORTED, "FAST windows read grid 0 only");
  if (n_scans >= c->pipeline_min && !fast) {
    if ((st = match_levels_pipelined(c, n_scans, c->scan_off.data(), levels, n_levels, poses, covs,
                                     sum.data(), grid, level_resp)) != CSM_OK)
      return st;
  } else {
    for (int l = 0; l < n_levels; ++l) {
      if ((st = match_level(c, n_scans, c->scan_off.data(), levels[l], poses, covs, resp.data(), nullptr,
                            grid, c->skip_dead_lists ? live_lists(levels, n_levels, l) : 0)) != CSM_OK)
        return st;
      for (int s = 0; s < n_scans; ++s) sum[(size_t)s] += resp[(size_t)s];
      if (level_resp) std::copy(resp.begin(), resp.end(), level_resp + (size_t)l * n_scans);
    }
  }
  for (int s = 0; s < n_scans; ++s) scores[s] = sum[(size_t)s] / times;  // :281
  if (c->profiling) {
    c->t_exit = now_ms();
    c->account("host:call", (float)(c->t_exit - t_call), 0.0, 0.0);
  }
  return CSM_OK;
}

int csmh::scan_matchers_batch_grids_levels(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                           const int32_t* grid_index, const csm_param levels[3], int32_t first_level,
                                           int32_t use_fine, const double* score_seed, double* poses, double* covs,
                                           double* scores, double* level_resp) {
  if (!c || !levels || !poses || !covs || !scores) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (first_level < 0 || first_level > 1 || (first_level == 1 && !use_fine))
    return c->fail(CSM_ERR_INVALID_ARG, "first_level must be 0, or 1 with use_fine");
  int st = load_scans_locked(c, n_scans, pts, offsets);
  if (st != CSM_OK) return st;
  if (grid_index) c->scan_grid.assign(grid_index, grid_index + n_scans);
  return matchers_loaded_locked(c, levels, use_fine, poses, covs, scores, first_level, score_seed, level_resp);
}

extern "C" {

int csm_scan_match_batch(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                         const csm_param* param, double* poses, double* covs, double* responses,
                         int64_t* argmax_flat) {
  if (!c || !param || !poses || !covs || !responses) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  int st;
  if ((st = check_offsets(c, n_scans, offsets)) != CSM_OK) return st;
  if (n_scans == 0) return CSM_OK;
  const int64_t n_total = offsets[n_scans] - offsets[0];
  if ((st = check_points(c, pts, n_total)) != CSM_OK) return st;
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  std::vector<int64_t> off(offsets, offsets + n_scans + 1);
  for (auto& o : off) o -= offsets[0];
  if ((st = upload_points(c, pts + 2 * offsets[0], n_total)) != CSM_OK) return st;
  return match_level(c, n_scans, off.data(), *param, poses, covs, responses, argmax_flat);
}

int csm_scan_match(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param,
                   double pose[3], double cov[9], double* response, int64_t* argmax_flat) {
  if (!c || !response) return CSM_ERR_INVALID_ARG;
  const int64_t off[2] = {0, n_points < 0 ? 0 : n_points};
  if (n_points < 0) return c->fail(CSM_ERR_INVALID_ARG, "negative point count");
  return csm_scan_match_batch(c, 1, pts, off, param, pose, cov, response, argmax_flat);
}

int csm_scan_matchers_submit(csm_ctx* c, const csm_param levels[3], int32_t use_fine, double* poses, double* covs,
                             double* scores) {
  if (!c || !levels || !poses || !covs || !scores) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st;
  // A queued batch (csm_load_scans_async) becomes the loaded one without
  // completing the pending batch: the swap parks the pending batch's points
  // in a staging slot, its last launch below borrows them back, and the next
  // upload into that slot comes after this call, which completes the pending
  // batch (its completion reads no points or offsets).
  // (checked before the swap: an early return after it would leave a pending
  // batch's last hand-off to launch on the new batch's points)
  if (c->staged_count == 0 && c->n_scans < 0) return c->fail(CSM_ERR_INVALID_ARG, "no scans loaded (csm_load_scans)");
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  ScanBatch* parked = nullptr;
  if (c->staged_count > 0) {
    parked = &c->staged[c->staged_head].batch;  // the slot take_staged swaps the current batch into
    if ((st = take_staged(c)) != CSM_OK) return st;
  }
  // the pending batch's last launch (its last part's last hand-off), on its own batch
  auto prior_last_launches = [&]() {
    BorrowedBatch own(c, parked);
    return pipe_last_launches(c);
  };
  const int32_t n_scans = c->n_scans;
  const int n_levels = use_fine ? 3 : 1;
  bool fast = false;
  for (int l = 0; l < n_levels; ++l) fast |= levels[l].type == CSM_FAST;
  const int32_t* grid = c->scan_grid.empty() ? nullptr : c->scan_grid.data();
  // one part where the other batch's launches cover the host (submit_parts), else the driver's parts
  const int K = submit_parts(c->submit_parts, c->pipeline_parts_set, std::min(c->pipeline_parts, csm_ctx::kMaxParts),
                             coarse_device_bound(c, levels, n_levels));
  if (n_scans == 0 || fast || grid || n_scans < c->pipeline_min || K > PipeState::kParts) {
    // nothing to overlap (or no second set of buffer slots): the batch completes here
    if ((st = prior_last_launches()) != CSM_OK || (st = pipe_drain(c)) != CSM_OK) return st;
    return matchers_loaded_locked(c, levels, use_fine, poses, covs, scores);
  }
  const double t_call = now_ms();
  c->t_call = t_call;
  PipeState& PS = pipe_of(c);
  PipeJob& J = PS.job[PS.next];
  PipeJob& P = PS.job[PS.next ^ 1];
  if (J.pending && ((st = prior_last_launches()) != CSM_OK || (st = pipe_drain(c)) != CSM_OK))
    return st;  // (cannot happen: submits alternate)
  PipeMode mode(c);
  job_setup(c, J, n_scans, c->scan_off.data(), levels, n_levels, poses, covs, nullptr, nullptr, K,
            PS.next * PipeState::kParts, true);
  J.own_sum.assign((size_t)n_scans, 0.0);
  J.sum = J.own_sum.data();
  J.scores = scores;
  // this batch's first part's first level, the previous batch's last launch
  // (its last part's last hand-off), then this batch's other levels around the
  // previous batch's completion, up to its own last part's last hand-off: the
  // order is csm_submit_order.hpp's, by the two batches' parts
  const SubmitOrder order = submit_order(K, P.pending ? P.K : 0, n_levels, c->defer_last_handoff);
  for (int i = 0; i < order.n; ++i) {
    const SubmitOp& op = order.op[i];
    switch (op.step) {
      case SubmitStep::kBegin: st = job_begin(c, J, op.part); break;
      case SubmitStep::kHandoff: st = job_handoff(c, J, op.level, op.part); break;
      case SubmitStep::kPriorLast: st = prior_last_launches(); break;
      case SubmitStep::kPriorFinish: st = job_finish(c, P); break;
    }
    if (st != CSM_OK) return pipe_abort(c, st);
  }
  job_launched(c, J);
  PS.next ^= 1;
  if (c->profiling) {
    c->t_exit = now_ms();
    c->account("host:submit", (float)(c->t_exit - t_call), 0.0, 0.0);
  }
  return CSM_OK;
}

int csm_scan_matchers_wait(csm_ctx* c) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return pipe_drain(c);
}

int csm_scan_matchers_loaded(csm_ctx* c, const csm_param levels[3], int32_t use_fine, double* poses,
                             double* covs, double* scores) {
  if (!c || !levels || !poses || !covs || !scores) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st0;
  if ((st0 = pipe_drain(c)) != CSM_OK || (st0 = take_staged(c)) != CSM_OK) return st0;
  return matchers_loaded_locked(c, levels, use_fine, poses, covs, scores);
}

int csm_scan_matchers_batch(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                            const csm_param levels[3], int32_t use_fine, double* poses, double* covs,
                            double* scores) {
  if (!c || !levels || !poses || !covs || !scores) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int st = load_scans_locked(c, n_scans, pts, offsets);
  if (st != CSM_OK) return st;
  return matchers_loaded_locked(c, levels, use_fine, poses, covs, scores);
}

int csm_scan_matchers(csm_ctx* c, const double* pts, int32_t n_points, const csm_param levels[3],
                      int32_t use_fine, double pose[3], double cov[9], double* score) {
  if (!c || !score) return CSM_ERR_INVALID_ARG;
  if (n_points < 0) return c->fail(CSM_ERR_INVALID_ARG, "negative point count");
  const int64_t off[2] = {0, n_points};
  return csm_scan_matchers_batch(c, 1, pts, off, levels, use_fine, pose, cov, score);
}

int csm_scan_matchers_batch_grids(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                  const int32_t* grid_index, const csm_param levels[3], int32_t use_fine,
                                  double* poses, double* covs, double* scores) {
  if (!c || !levels || !poses || !covs || !scores) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st = load_scans_locked(c, n_scans, pts, offsets);
  if (st != CSM_OK) return st;
  if (grid_index) c->scan_grid.assign(grid_index, grid_index + n_scans);
  return matchers_loaded_locked(c, levels, use_fine, poses, covs, scores);
}

int csm_scan_matchers_batch_grids_seeded(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                         const int32_t* grid_index, const csm_param levels[3], int32_t first_level,
                                         int32_t use_fine, const double* score_seed, double* poses, double* covs,
                                         double* scores) {
  return scan_matchers_batch_grids_levels(c, n_scans, pts, offsets, grid_index, levels, first_level, use_fine,
                                          score_seed, poses, covs, scores, nullptr);
}

}  // extern "C"
