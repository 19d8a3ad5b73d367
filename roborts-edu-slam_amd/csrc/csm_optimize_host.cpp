// csm_optimize_host.cpp — the Gauss-Newton matcher's host side
// (BasedOptimizeScanMatch, optimize_scan_matcher.h:60-237). Two forms of the
// same solve: the host loop (optimize_batch: per-iteration control flow and
// glibc sincos around optimize_cost_kernel, one round trip per iteration) and
// the one-launch form (optimize_batch_device: optimize_solve_kernel, the loop
// inside the kernel). Both take their steps from csm_optimize_step.hpp.
#include "csm_host.hpp"
#include "csm_optimize_step.hpp"

namespace csmh {

// ---- Gauss-Newton scan matcher ------------------------------------------------
// BasedOptimizeScanMatch (optimize_scan_matcher.h:60-237; SURVEY.md 8f row
// f3). Host loop: the device evaluates UpdateCost for every active scan per
// launch (csm_optimize.hip); the host keeps the reference's per-iteration
// control flow and glibc cos/sin, and takes the step (csm_optimize_step.hpp).

using csm::opt::kDone;
using csm::opt::kHost;
using csm::opt::kNan;
using csm::opt::kRun;
using csm::opt::kSkip;

namespace {

csm::opt::StepParam step_param(const csm_optimize_param& P, double mres) {
  // map_resolution_ = GetCellLength() (:82); UpdatePose's max_update_distance / map_resolution_ (:146-147)
  return csm::opt::StepParam{P.cost_decrease_threshold, P.cost_min_threshold, P.max_update_distance / mres,
                             P.max_update_angle};
}

}  // namespace

// util::NormalizeAngle (util/slam_util.h:103-111)
double normalize_angle(double a) {
  double n = std::fmod(std::fmod(a, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI);
  if (n > M_PI) n -= 2.0 * M_PI;
  return n;
}

// n_scans scans whose points are resident in c->pts at offsets off (n+1,
// relative). poses world in/out, costs out; iters (nullable) = UpdateCost
// evaluations per scan. Scan s reads grid grid_index[s] of the resident stack
// (null: grid 0). only (nullable): the scans to run; the others' outputs are
// left as they are.
int optimize_batch(csm_ctx* c, int32_t n_scans, const int64_t* off, const int32_t* grid_index,
                   const csm_optimize_param& P, double* poses, double* costs, int32_t* iters, const uint8_t* only) {
  const Geometry geo(c->info);
  const bool ready = map_ready(c);
  std::vector<double> est((size_t)n_scans * 3), cost((size_t)n_scans, 0.0);
  std::vector<int32_t> state((size_t)n_scans, kSkip);
  int n_active = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    if (only && !only[s]) continue;
    if (iters) iters[s] = 0;
    if (!ready || off[s + 1] == off[s]) continue;  // :73-76
    geo.to_map(poses + 3 * s, &est[(size_t)3 * s]);  // GetMapCoordsPose (:79-80)
    // cost_ starts at 0.0 here; the reference returns its stale member when
    // iterate_max_times <= 0 (no iteration) — defined as 0.0
    state[(size_t)s] = (P.iterate_max_times > 0) ? kRun : kDone;
    n_active += state[(size_t)s] == kRun;
  }
  std::vector<uint8_t> active((size_t)n_scans);
  for (int32_t s = 0; s < n_scans; ++s) active[(size_t)s] = state[(size_t)s] == kRun;
  hipError_t e;
  if ((e = c->opt_off.ensure(sizeof(int64_t) * (size_t)(n_scans + 1))) != hipSuccess ||
      (e = c->opt_scans.ensure(sizeof(csm::OptScan) * (size_t)n_scans)) != hipSuccess ||
      (e = c->opt_sums.ensure(sizeof(csm::OptSums) * (size_t)n_scans)) != hipSuccess ||
      (e = c->h_opt_scans.ensure(sizeof(csm::OptScan) * (size_t)n_scans)) != hipSuccess ||
      (e = c->h_opt_sums.ensure(sizeof(csm::OptSums) * (size_t)n_scans)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(optimize)");
  if ((e = hipMemcpyAsync(c->opt_off.p, off, sizeof(int64_t) * (size_t)(n_scans + 1), hipMemcpyHostToDevice,
                          c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(optimize offsets)");
  csm::OptArgs A{};
  A.grid = c->d_grid;
  A.size_x = c->info.size_x;
  A.size_y = c->info.size_y;
  A.outside = c->outside;
  A.pts = (const double*)c->pts.p;
  A.offsets = (const int64_t*)c->opt_off.p;
  A.scans = (const csm::OptScan*)c->opt_scans.p;
  A.out = (csm::OptSums*)c->opt_sums.p;
  auto* hs = (csm::OptScan*)c->h_opt_scans.p;
  auto* hr = (const csm::OptSums*)c->h_opt_sums.p;
  const csm::opt::StepParam SP = step_param(P, geo.mres);
  for (int iter = 0; iter < P.iterate_max_times && n_active > 0; ++iter) {
    for (int32_t s = 0; s < n_scans; ++s) {
      csm::OptScan& o = hs[s];
      o.active = active[(size_t)s];
      o.grid = grid_index ? grid_index[s] : 0;
      if (!o.active) continue;
      const double* m = &est[(size_t)3 * s];
      csm::host_sincos(m[2], &o.s, &o.c);  // rotation (:96-97), de_s (:200-201)
      o.tx = m[0];
      o.ty = m[1];
    }
    if ((e = hipMemcpyAsync(c->opt_scans.p, hs, sizeof(csm::OptScan) * (size_t)n_scans, hipMemcpyHostToDevice,
                            c->stream)) != hipSuccess)
      return c->hip_fail(e, "hipMemcpyAsync(optimize state)");
    if (c->profiling && (e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return c->hip_fail(e, "hipEventRecord");
    if ((e = csm::launch_optimize_cost(A, n_scans, c->stream)) != hipSuccess)
      return c->hip_fail(e, "optimize_cost_kernel");
    if (c->profiling && (e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return c->hip_fail(e, "hipEventRecord");
    if ((e = hipMemcpyAsync(c->h_opt_sums.p, c->opt_sums.p, sizeof(csm::OptSums) * (size_t)n_scans,
                            hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
      return c->hip_fail(e, "hipMemcpyAsync(optimize sums)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "hipStreamSynchronize(optimize)");
    if (c->profiling) {
      float ms = 0.0f;
      (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
      double in_map = 0.0;
      for (int32_t s = 0; s < n_scans; ++s)
        if (active[(size_t)s]) in_map += hr[s].valid;
      c->account("optimize_cost_kernel", ms, 16.0 * in_map, 0.0);  // 4 fp32 corners per point in the map
    }
    for (int32_t s = 0; s < n_scans; ++s) {
      if (!active[(size_t)s]) continue;
      const csm::OptSums& r = hr[s];
      if (iters) iters[s] = iter + 1;
      // the cost, CalculateDet, the NaN and stop tests, UpdatePose (:88-118, :144-152)
      const int32_t next = csm::opt::step(r.v, r.valid, iter, SP, &est[(size_t)3 * s], &cost[(size_t)s]);
      if (next != kRun) {
        state[(size_t)s] = next;
        active[(size_t)s] = 0;
        --n_active;
      }
    }
  }
  for (int32_t s = 0; s < n_scans; ++s) {
    if (only && !only[s]) continue;
    if (state[(size_t)s] == kSkip || state[(size_t)s] == kNan) {
      costs[s] = kOptMaxCost;  // pose untouched
      continue;
    }
    double* m = &est[(size_t)3 * s];
    m[2] = normalize_angle(m[2]);    // :126
    geo.to_world(m, poses + 3 * s);  // GetWorldCoordsPose (:128)
    costs[s] = cost[(size_t)s];
  }
  return CSM_OK;
}

// optimize_batch with the whole solve in one launch (optimize_solve_kernel):
// one copy up (states, offsets, grid indices), one launch, one copy down, one
// synchronize. Fail closed: without the device sincos (CSM_DEVICE_TRIG=0, no
// libm table) the whole call is the host loop's, and a scan whose angle left
// the restated sincos' domain (kHost) is run again by the host loop from its
// initial pose. The host loop is deterministic, so either way the bits are
// optimize_batch's.
int optimize_batch_device(csm_ctx* c, int32_t n_scans, const int64_t* off, const int32_t* grid_index,
                          const csm_optimize_param& P, double* poses, double* costs, int32_t* iters) {
  if (!c->device_trig || libm_sincos_table() == nullptr) {
    c->account_count("optimize:host_batches", 1);
    return optimize_batch(c, n_scans, off, grid_index, P, poses, costs, iters, nullptr);
  }
  const Geometry geo(c->info);
  const bool ready = map_ready(c);
  int n_active = 0;
  for (int32_t s = 0; s < n_scans; ++s) n_active += ready && off[s + 1] != off[s];
  // nothing to launch (:73-76, or no iteration): the host loop's early returns
  if (n_active == 0 || P.iterate_max_times <= 0)
    return optimize_batch(c, n_scans, off, grid_index, P, poses, costs, iters, nullptr);
  // one staging block: OptSolveScan[n] | offsets[n + 1] | grid_index[n]
  const size_t o_off = sizeof(csm::OptSolveScan) * (size_t)n_scans;
  const size_t o_grid = o_off + sizeof(int64_t) * (size_t)(n_scans + 1);
  const size_t bytes = o_grid + sizeof(int32_t) * (size_t)n_scans;
  hipError_t e;
  int st;
  if ((e = c->opt_solve.ensure(bytes)) != hipSuccess || (e = c->h_opt_solve.ensure(bytes)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(optimize solve)");
  if ((st = ensure_trig_table(c, c->stream)) != CSM_OK) return st;
  auto* hs = (csm::OptSolveScan*)c->h_opt_solve.p;
  for (int32_t s = 0; s < n_scans; ++s) {
    csm::OptSolveScan& o = hs[s];
    o = csm::OptSolveScan{};
    o.state = kSkip;
    if (!ready || off[s + 1] == off[s]) continue;  // :73-76
    geo.to_map(poses + 3 * s, o.est);              // GetMapCoordsPose (:79-80)
    o.state = kRun;
  }
  std::memcpy((char*)c->h_opt_solve.p + o_off, off, sizeof(int64_t) * (size_t)(n_scans + 1));
  if (grid_index) std::memcpy((char*)c->h_opt_solve.p + o_grid, grid_index, sizeof(int32_t) * (size_t)n_scans);
  csm::OptSolveArgs A{};
  A.grid = c->d_grid;
  A.size_x = c->info.size_x;
  A.size_y = c->info.size_y;
  A.outside = c->outside;
  A.iterate_max_times = P.iterate_max_times;
  A.pts = (const double*)c->pts.p;
  A.offsets = (const int64_t*)((const char*)c->opt_solve.p + o_off);
  A.grid_index = grid_index ? (const int32_t*)((const char*)c->opt_solve.p + o_grid) : nullptr;
  A.tab = (const double*)c->trig_tab.p;
  A.P = step_param(P, geo.mres);
  A.scans = (csm::OptSolveScan*)c->opt_solve.p;
  if ((e = hipMemcpyAsync(c->opt_solve.p, c->h_opt_solve.p, bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(optimize solve state)");
  if (c->profiling && (e = hipEventRecord(c->ev0, c->stream)) != hipSuccess) return c->hip_fail(e, "hipEventRecord");
  if ((e = csm::launch_optimize_solve(A, n_scans, c->stream)) != hipSuccess)
    return c->hip_fail(e, "optimize_solve_kernel");
  if (c->profiling && (e = hipEventRecord(c->ev1, c->stream)) != hipSuccess) return c->hip_fail(e, "hipEventRecord");
  if ((e = hipMemcpyAsync(c->h_opt_solve.p, c->opt_solve.p, o_off, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(optimize solve results)");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "hipStreamSynchronize(optimize solve)");
  if (c->profiling) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    double reads = 0.0;  // at most 4 fp32 corners per point and UpdateCost
    for (int32_t s = 0; s < n_scans; ++s) reads += (double)hs[s].iters * (double)(off[s + 1] - off[s]);
    c->account("optimize_solve_kernel", ms, 16.0 * reads, 0.0);
  }
  std::vector<uint8_t> host((size_t)n_scans, 0);
  int32_t n_host = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    csm::OptSolveScan& r = hs[s];
    if (r.state == kHost) {
      host[(size_t)s] = 1;
      ++n_host;
      continue;
    }
    if (iters) iters[s] = r.iters;
    if (r.state != kDone) {  // kSkip, kNan
      costs[s] = kOptMaxCost;  // pose untouched
      continue;
    }
    r.est[2] = normalize_angle(r.est[2]);  // :126
    geo.to_world(r.est, poses + 3 * s);    // GetWorldCoordsPose (:128)
    costs[s] = r.cost;
  }
  c->account_count("optimize:host_scans", n_host);
  if (n_host == 0) return CSM_OK;
  return optimize_batch(c, n_scans, off, grid_index, P, poses, costs, iters, host.data());
}

}  // namespace csmh

using namespace csmh;

extern "C" {

int csm_optimize_scan_match_batch_grids(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                        const int32_t* grid_index, const csm_optimize_param* param, double* poses,
                                        double* costs, int32_t* iterations) {
  if (!c || !param || (n_scans > 0 && (!poses || !costs))) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  int st;
  if ((st = check_offsets(c, n_scans, offsets)) != CSM_OK) return st;
  if (n_scans == 0) return CSM_OK;
  const int64_t n_total = offsets[n_scans] - offsets[0];
  if ((st = check_points(c, pts, n_total)) != CSM_OK) return st;
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  for (int32_t s = 0; grid_index && s < n_scans; ++s)
    if (grid_index[s] < 0 || grid_index[s] >= c->n_grids)
      return c->fail(CSM_ERR_INVALID_ARG, "scan grid outside the resident stack");
  std::vector<int64_t> off(offsets, offsets + n_scans + 1);
  for (auto& o : off) o -= offsets[0];
  if ((st = upload_points(c, pts + 2 * offsets[0], n_total)) != CSM_OK) return st;
  return optimize_batch_device(c, n_scans, off.data(), grid_index, *param, poses, costs, iterations);
}

int csm_optimize_scan_match_batch(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                                  const csm_optimize_param* param, double* poses, double* costs,
                                  int32_t* iterations) {
  if (!c || !param || (n_scans > 0 && (!poses || !costs))) return CSM_ERR_INVALID_ARG;
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
  return optimize_batch(c, n_scans, off.data(), nullptr, *param, poses, costs, iterations, nullptr);
}

int csm_optimize_scan_match(csm_ctx* c, const double* pts, int32_t n_points, const csm_optimize_param* param,
                            double pose[3], double* cost) {
  if (!c || !cost || !pose) return CSM_ERR_INVALID_ARG;
  if (n_points < 0) return c->fail(CSM_ERR_INVALID_ARG, "negative point count");
  const int64_t off[2] = {0, n_points};
  return csm_optimize_scan_match_batch(c, 1, pts, off, param, pose, cost, nullptr);
}

int csm_optimize_update_cost(csm_ctx* c, const double* pts, int32_t n_points, const double est_map[3],
                             double* cost, double H[9], double b[3]) {
  if (!c || !est_map || !cost || !H || !b) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  int st;
  if (n_points < 0) return c->fail(CSM_ERR_INVALID_ARG, "negative point count");
  if ((st = check_points(c, pts, n_points)) != CSM_OK) return st;
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  if ((st = upload_points(c, pts, n_points)) != CSM_OK) return st;
  const int64_t off[2] = {0, n_points};
  hipError_t e;
  if ((e = c->opt_off.ensure(sizeof(off))) != hipSuccess || (e = c->opt_scans.ensure(sizeof(csm::OptScan))) != hipSuccess ||
      (e = c->opt_sums.ensure(sizeof(csm::OptSums))) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(optimize)");
  csm::OptScan o{};
  csm::host_sincos(est_map[2], &o.s, &o.c);
  o.tx = est_map[0];
  o.ty = est_map[1];
  o.active = 1;
  o.grid = 0;
  csm::OptArgs A{};
  A.grid = c->d_grid;
  A.size_x = c->info.size_x;
  A.size_y = c->info.size_y;
  A.outside = c->outside;
  A.pts = (const double*)c->pts.p;
  A.offsets = (const int64_t*)c->opt_off.p;
  A.scans = (const csm::OptScan*)c->opt_scans.p;
  A.out = (csm::OptSums*)c->opt_sums.p;
  csm::OptSums r{};
  if ((e = hipMemcpyAsync(c->opt_off.p, off, sizeof(off), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(c->opt_scans.p, &o, sizeof(o), hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (e = csm::launch_optimize_cost(A, 1, c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&r, c->opt_sums.p, sizeof(r), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "optimize_cost_kernel");
  *cost = csm::opt::normalized_cost(r.v[0], r.valid);
  const double h[9] = {r.v[1], r.v[2], r.v[4], r.v[2], r.v[3], r.v[5], r.v[4], r.v[5], r.v[6]};
  std::memcpy(H, h, sizeof(h));
  b[0] = r.v[7];
  b[1] = r.v[8];
  b[2] = r.v[9];
  return CSM_OK;
}

}  // extern "C"
