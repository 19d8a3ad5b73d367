// csm_level.cpp — one level (BasedCorrelationScanMatch::ScanMatch,
// correlate_scan_matcher.h:784-875) over a batch of scans: its windows
// planned, launched, joined and completed, whole or in spans, and one level's
// end fused with the next one's beginning (LevelRun, csm_driver_internal.hpp).
#include "csm_driver_internal.hpp"
#include "libm_sincos.hpp"

namespace csmh {

// Which covariance lists of level l a caller of the 3-level driver can see,
// as the finish's skip mask (bit 0 positional, bit 1 angular: skipped).
// ComputePositionalCovariance resets the whole matrix (correlate_scan_matcher.h:891)
// and ComputeAngularCovariance writes (2,2) only (:1018), by type (:835-858); a
// later level that writes the same entries makes this level's value dead (the
// reference's coarse covariance is always overwritten by the fine level).
int live_lists(const csm_param* levels, int n_levels, int l) {
  auto pos = [](int t) { return t == CSM_COARSE || t == CSM_FAST || t == CSM_FINE; };
  auto ang = [](int t) { return t == CSM_COARSE || t == CSM_FAST || t == CSM_SUPER; };
  int skip = 0;
  for (int k = l + 1; k < n_levels; ++k) {
    if (pos(levels[k].type)) return 3;
    if (ang(levels[k].type)) skip |= 2;
  }
  return skip;
}

namespace {

// Seals (csm_internal.hpp) are waited for at most this long: they land within
// microseconds of the flag; a seal that never matches is a failure, not a hang.
constexpr double kSealWaitMs = 2000.0;

// Window i's FinishOut from the pinned host memory the finish wrote, whole:
// spin until its seal names a final writer for this launch and the copy's
// pieces match it (the pieces can land after the launch's flag).
// Returns the writer (kSealFast / kSealExact), kSealPending when `pending_ok`
// and the fast pass left the window to the exact pass, 0 on a timeout.
uint32_t sealed_copy(const LevelRun& R, int i, csm::FinishOut& out, bool pending_ok) {
  const double t0 = now_ms();
  for (uint32_t spin = 1;; ++spin) {
    const uint32_t w = read_sealed(R.fin + i, R.pend.flag_value, out);
    if (w == csm::kSealFast || w == csm::kSealExact || (pending_ok && w == csm::kSealPending)) return w;
    if ((spin & 255) == 0 && now_ms() - t0 > kSealWaitMs) return 0u;
    __builtin_ia32_pause();
  }
}

// Which scans of a level have windows, and its dimensions (no planning yet).
// `reset`: responses (and argmaxes) of the batch start at kMinResponse.
int level_prepare(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P, double* responses,
                  int64_t* argmax_flat, LevelRun& R, const int32_t* scan_grid, int skip_lists, bool reset) {
  R.P = P;
  R.skip_lists = skip_lists;
  R.scan_of.clear();
  R.grid.clear();
  int st = window_dims(P, R.D);
  if (st != CSM_OK) return c->fail(st, "invalid search window parameters");
  R.scan_of.reserve((size_t)n_scans);
  const bool ready = map_ready(c);
  R.shape = LevelSummary{};
  R.range_preset = false;
  int last_n = -1;  // the beam rule's verdict for the last point count (scans mostly share one)
  for (int k = 0; k < n_scans; ++k) {
    const int s = R.order ? R.order[k] : k;
    if (reset) {
      responses[s] = 0.0;  // kMinResponse (:1034)
      if (argmax_flat) argmax_flat[s] = -1;
    }
    const int n = (int)(offsets[s + 1] - offsets[s]);
    if (!ready || n == 0) continue;  // :792-795
    if (n != last_n) {
      int step, use, n_used;
      if (!beam_rule(n, P.use_point_size, step, use, n_used))
        return c->fail(CSM_ERR_INVALID_ARG, "use_point_size <= 1 with n_points >= 2*use_point_size");
      last_n = n;
      // the level's beam and point maxima: a count already seen changes neither
      level_summary_add(R.shape, n, step, n_used, true);
    }
    R.scan_of.push_back(s);
    if (scan_grid) R.grid.push_back(scan_grid[s]);
  }
  R.shape.n_windows = (int32_t)R.scan_of.size();  // (level_summary_add counted the distinct sizes)
  return CSM_OK;
}

// Device finish for the front-end windows (and enough of them to fill the
// chip); a handful of windows finish faster on the host's std::sort.
bool level_device_finish(const csm_ctx* c, const Dims& D, int nw) {
  return c->device_finish && D.n_cand <= csm::kFinishMaxCand && csm::finish_lds_bytes(D.n_cand) <= 160 * 1024 &&
         nw >= c->device_finish_min;
}

// Room for the level's plans and angle rows (pinned: uploaded by DMA).
// spans: the level goes out in spans, so its launches see window plans not
// planned yet: zeroed, for the traffic they account (beams summed over the
// level); no decision reads them (LevelRun::shape). Otherwise every plan is
// written before the launch and the old ones are only resized (value-initialising
// 2048 plans cost ~20 us of the serial chain, r06).
int level_alloc(csm_ctx* c, const int64_t* offsets, LevelRun& R, HostBuf& rows, bool spans) {
  const int nw = (int)R.scan_of.size();
  // the grid's fixed-point copy, whose pitch and value bound the plan pass's
  // range check reads (level_plan_one): before this, the first level after a
  // new grid was checked against the previous grid's (a fresh context: zeros,
  // which pass every window)
  int gst = ensure_int_grid(c);
  if (gst != CSM_OK) return gst;
  if (spans)
    R.plans.assign((size_t)nw, WindowPlan{});
  else
    R.plans.resize((size_t)nw);
  R.pt_off.resize((size_t)nw);
  for (int i = 0; i < nw; ++i) R.pt_off[(size_t)i] = offsets[R.scan_of[(size_t)i]];
  hipError_t he = rows.ensure((size_t)nw * (size_t)R.D.n_angles * sizeof(AngleEntry));
  if (he != hipSuccess) return c->hip_fail(he, "hipHostMalloc(angles)");
  R.rows = (AngleEntry*)rows.p;
  R.angles = R.rows;
  // this slot's ScanWork staging (run_windows uploads it from c->h_sw; the
  // slot's previous launch has read it: its level was joined before this plan)
  if ((he = c->h_sw.ensure((size_t)nw * sizeof(ScanWork))) != hipSuccess) return c->hip_fail(he, "hipHostMalloc(scans)");
  R.sw = (ScanWork*)c->h_sw.p;
  const bool dev = level_device_finish(c, R.D, nw);
  R.sw_stride = score_stride(c, R.D, dev ? Finish::kDevice : Finish::kScoresToHost);
  R.int_bad = 0;
  R.int_known = false;
  R.dev_trig = c->device_trig && dev && !small_launch(c, R.D, nw) && libm_sincos_table() != nullptr;
  R.trig_bad = 0;
  return CSM_OK;
}

// Plan window i of a prepared level around the scan's current pose: host
// libm cos/sin per angle (AngleSearchLookUpTable::UpdateLookUpTable :154-172).
// Its ScanWork goes straight into the slot's staging, and its fixed-point
// range is checked (LevelRun::sw, int_bad).
void level_plan_one(const csm_ctx* c, LevelRun& R, const Geometry& G, const int64_t* offsets, const double* poses,
                    int i) {
  const int s = R.scan_of[(size_t)i];
  double center[3];
  G.to_map(poses + 3 * s, center);
  WindowPlan& W = R.plans[(size_t)i];
  AngleEntry* rows = R.rows + (size_t)i * (size_t)R.D.n_angles;
  plan_window_into(R.P, R.D, G, (int)(offsets[s + 1] - offsets[s]), center, rows, W, !R.dev_trig);
  // (the angles grow with their index: both ends inside the domain, all are)
  if (R.dev_trig && R.D.n_angles > 0 &&
      !(csm::libm::sincos_device_ok(rows[0].angle) && csm::libm::sincos_device_ok(rows[R.D.n_angles - 1].angle)))
    __atomic_store_n(&R.trig_bad, 1, __ATOMIC_RELAXED);
  W.angle_off = (int64_t)i * R.D.n_angles;
  if (R.sw)
    fill_scan_work_one(R.D, W, R.pt_off[(size_t)i], R.grid.empty() ? 0 : R.grid[(size_t)i], (size_t)i, R.sw_stride,
                       R.sw[i]);
  if (!int_mode_window_ok(c, R.D, R.P.search_space_resolution / G.mres, W))
    __atomic_store_n(&R.int_bad, 1, __ATOMIC_RELAXED);
}

// Enqueue a planned level, or a span of it (nothing waits).
int level_launch(csm_ctx* c, LevelRun& R, WinSpan sp = WinSpan{}) {
  const int nw = (int)R.scan_of.size();
  const Dims& D = R.D;
  const Geometry G(c->info);
  R.dev = level_device_finish(c, D, nw);
  sp.sw_ready = R.sw;
  sp.sw_stride = R.sw_stride;
  // the level's fixed-point range: what the plan pass found once every window
  // is planned, or what was settled before the first span (range_preset: every
  // window in range, or the level would not go out in spans). A window the
  // plan then finds out of range after all contradicts the bound it was
  // launched under: an error, never a span scored by other kernels.
  const bool int_bad = __atomic_load_n(&R.int_bad, __ATOMIC_RELAXED) != 0;
  if (R.range_preset) {
    if (c->int_ok && int_bad)
      return c->fail(CSM_ERR_INVALID_ARG, "a window left the fixed-point range its level was launched for");
  } else {
    if (!R.int_known) return c->fail(CSM_ERR_INVALID_ARG, "level launched in spans without its range settled");
    R.shape.in_range = !int_bad;
  }
  sp.level = &R.shape;
  sp.dev_trig = R.dev_trig;
  sp.rows_gen = R.dev_trig && !__atomic_load_n(&R.trig_bad, __ATOMIC_RELAXED);
  const int st = run_windows(c, R.P, D, G, R.plans, R.pt_off, R.angles, (size_t)nw * (size_t)D.n_angles, R.grid,
                             nullptr, R.dev ? Finish::kDevice : Finish::kScoresToHost, &R.pend, R.skip_lists, sp);
  if (st != CSM_OK || !sp.finish) return st;
  R.fin = R.pend.fin_host ? R.pend.fin_host : (const csm::FinishOut*)c->h_fin.p;
  R.scores = (const double*)c->h_scores.p;
  return CSM_OK;
}

// Every window of a prepared level inside the fixed-point range, from the
// scans' poses alone, before any window is planned: what level_plan_one will
// find (the same x0, y0 as plan_window_into, the same check; level_in_range
// tries the windows' two extreme corners before going window by window).
RangeEnv range_env(const csm_ctx* c) { return RangeEnv{c->pts_maxabs, c->pitch, c->int_max_abs, c->int_exp}; }

bool level_range_from_poses(const csm_ctx* c, const LevelRun& R, const Geometry& G, const int64_t* offsets,
                            const double* poses) {
  const double half = (R.P.search_space_size / G.mres) * 0.5;
  const double far = (double)(R.D.n_space - 1) * (R.P.search_space_resolution / G.mres);
  int last_n = -1, last_used = 0;  // (level_prepare accepted every size)
  auto start = [&](int i, double& x0, double& y0, int& n_used) {
    const int s = R.scan_of[(size_t)i];
    double m[3];
    G.to_map(poses + 3 * (size_t)s, m);
    x0 = m[0] - half;
    y0 = m[1] - half;
    const int n = (int)(offsets[s + 1] - offsets[s]);
    if (n != last_n) {
      int step, use;
      (void)beam_rule(n, R.P.use_point_size, step, use, last_used);
      last_n = n;
    }
    n_used = last_used;
  };
  return level_in_range((int)R.scan_of.size(), start, far, range_env(c));
}

// The same for the level N a split hand-off launches while the second half
// of the previous level R is still being completed: N's windows bounded from
// R's (handoff_reach_bound over the hull of R's windows and centres) at N's
// most beams. False when the bound does not clear the range: the hand-off
// then launches N once, after every window is planned.
bool handoff_in_range(const csm_ctx* c, const LevelRun& R, const LevelRun& N, const Geometry& G) {
  const double pfar = (double)(R.D.n_space - 1) * (R.P.search_space_resolution / G.mres);
  const double half = (N.P.search_space_size / G.mres) * 0.5;
  const double far = (double)(N.D.n_space - 1) * (N.P.search_space_resolution / G.mres);
  Hull X, Y;
  for (const WindowPlan& W : R.plans) {
    X.add(W.x0, W.center[0], pfar);
    Y.add(W.y0, W.center[1], pfar);
  }
  return range_env(c).ok(handoff_reach_bound(X, Y, half, far), N.shape.max_n_used);
}

}  // namespace

int level_begin(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P,
                const double* poses, double* responses, int64_t* argmax_flat, LevelRun& R,
                const int32_t* scan_grid, int skip_lists) {
  int st = level_prepare(c, n_scans, offsets, P, responses, argmax_flat, R, scan_grid, skip_lists, true);
  if (st != CSM_OK) return st;
  const int nw = (int)R.scan_of.size();
  if (nw == 0) return CSM_OK;
  const double t0 = now_ms();
  if ((st = level_alloc(c, offsets, R, c->h_angles, false)) != CSM_OK) return st;
  const Geometry G(c->info);
  const int threads = (nw >= 64) ? c->host_threads : 1;
  if (c->profiling) c->account("host:plan:alloc", (float)(now_ms() - t0), 0.0, 0.0);
  c->parallel_for(nw, threads, [&](int i) { level_plan_one(c, R, G, offsets, poses, i); });
  R.int_known = true;
  if (threads > 1) c->account_pool("plan");
  const double t1 = now_ms();
  if ((st = level_launch(c, R)) != CSM_OK) return st;
  if (c->profiling) {  // per level (window size), and in all
    c->account("host:launch", (float)(now_ms() - t1), 0.0, 0.0);
    char nm[48];
    std::snprintf(nm, sizeof(nm), "host:plan<%lld>", (long long)R.D.n_cand);
    c->account("host:plan", (float)(t1 - t0), 0.0, 0.0);
    c->account(nm, (float)(t1 - t0), 0.0, 0.0);
  }
  return CSM_OK;
}

// level_begin with the plan in growing pieces: the pool plans the first
// `first` windows and their scoring goes out at once, then the next
// span_growth times as many while those score, and so on; the finish follows
// for all. For the 3-level driver's first part, where nothing else keeps the
// device busy while the host plans (a call's first ~0.3 ms with the whole
// level planned before one launch). The spans are whole-window
// ranges of one level: results are the one-launch level's.
int level_begin_split(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P, const double* poses,
                      double* responses, LevelRun& R, const int32_t* scan_grid, int skip_lists, int first) {
  const double t_in = now_ms();
  if (c->profiling && c->t_call > 0.0) c->account("host:first:entry->split", (float)(t_in - c->t_call), 0.0, 0.0);
  int st = level_prepare(c, n_scans, offsets, P, responses, nullptr, R, scan_grid, skip_lists, true);
  if (st != CSM_OK) return st;
  if (c->profiling) c->account("host:first:prepare", (float)(now_ms() - t_in), 0.0, 0.0);
  const int nw = (int)R.scan_of.size();
  // In spans only with the level's one decision settled before the first of
  // them (LevelRun::shape): the beam and point maxima are level_prepare's, and
  // every window must be in fixed-point range by its scan's pose; a level with
  // a window out of range goes out in one launch (fp64 columns for all of it).
  bool spans = first > 0 && nw >= 2 * first && level_device_finish(c, R.D, nw);
  const Geometry G(c->info);
  if (spans) {
    if ((st = ensure_int_grid(c)) != CSM_OK) return st;
    spans = !c->int_ok || level_range_from_poses(c, R, G, offsets, poses);
  }
  if (!spans) return level_begin(c, n_scans, offsets, P, poses, responses, nullptr, R, scan_grid, skip_lists);
  const double t0 = now_ms();
  if ((st = level_alloc(c, offsets, R, c->h_angles, true)) != CSM_OK) return st;
  R.shape.in_range = true;
  R.range_preset = true;
  if (c->profiling) c->account("host:first:prepare+alloc", (float)(now_ms() - t_in), 0.0, 0.0);
  int w0 = 0;
  for (int64_t sz = first; w0 < nw; sz *= std::max(2, c->span_growth)) {
    // the last span takes the rest when it would leave less than a span behind
    const int w1 = level_span_end(nw, w0, sz);
    const double tp = now_ms();
    c->parallel_for(w1 - w0, c->host_threads, [&](int i) { level_plan_one(c, R, G, offsets, poses, w0 + i); });
    R.int_known = w1 == nw;
    c->account_pool("plan");
    if (c->profiling && w0 == 0) c->account("host:first:plan", (float)(now_ms() - tp), 0.0, 0.0);
    if ((st = level_launch(c, R, WinSpan{w0, w1, true, false})) != CSM_OK) return st;
    if (w0 == 0 && c->profiling && c->t_call > 0.0)
      c->account("host:entry->first_launch", (float)(now_ms() - c->t_call), 0.0, 0.0);
    w0 = w1;
  }
  if ((st = level_launch(c, R, WinSpan{0, nw, false, true})) != CSM_OK) return st;
  if (c->profiling) {
    char nm[48];
    std::snprintf(nm, sizeof(nm), "host:plan+launch<%lld,split>", (long long)R.D.n_cand);
    c->account(nm, (float)(now_ms() - t0), 0.0, 0.0);
  }
  return CSM_OK;
}

namespace {

// Join a level's launch and check its device finish.
int level_join(csm_ctx* c, LevelRun& R) {
  const int nw = (int)R.scan_of.size();
  const double t1 = now_ms();
  const int st = wait_run(c, R.pend);
  if (st != CSM_OK) return st;
  if (c->profiling) {
    const float tw = (float)(now_ms() - t1);
    c->account("host:wait", tw, 0.0, 0.0);
    if (R.tag >= 0) {
      char nm[48];
      std::snprintf(nm, sizeof(nm), "host:wait<l%d,p%d>", R.tag / 8, R.tag % 8);
      c->account(nm, tw, 0.0, 0.0);
    }
  }
  if (R.dev && !R.pend.fin_host)  // (sealed windows are checked as they are completed)
    for (int i = 0; i < nw; ++i)
      if (R.fin[i].count < 0) return c->fail(CSM_ERR_HIP, "finish_kernel: work loop bound exceeded");
  return CSM_OK;
}

// After a level's windows are completed: a sealed window that never matched
// its seal (or carried the exact pass's overflow count) fails the call.
int level_check(csm_ctx* c, const LevelRun& R) {
  if (R.err) return c->fail(CSM_ERR_HIP, "finish: a window's FinishOut did not match its seal (or overflowed)");
  return CSM_OK;
}

// Complete window i of a joined level: pose, covariance and response
// (BasedCorrelationScanMatch::ScanMatch :815-869).
// defer (early completion): a window whose seal says the exact pass still owes
// it is not completed; returns false and the caller completes it after the join.
bool level_complete_one(const LevelRun& R, const Geometry& G, double* poses, double* covs, double* responses,
                        int64_t* argmax_flat, int i, bool defer = false) {
  thread_local std::vector<Entry> scratch;
  const Dims& D = R.D;
  const csm_param& P = R.P;
  const int s = R.scan_of[(size_t)i];
  const double f = P.search_space_resolution / G.mres;
  const CandGeom C{R.plans[(size_t)i], R.angles + R.plans[(size_t)i].angle_off, f, D.n_space,
                   (int64_t)D.n_space * D.n_space};
  csm::FinishOut local;
  const csm::FinishOut* o = nullptr;
  if (R.dev && R.pend.fin_host) {  // pinned host memory the finish wrote: a sealed copy
    const uint32_t w = sealed_copy(R, i, local, defer);
    if (w == csm::kSealPending) {
      if (R.how) (*R.how)[(size_t)i] = 2;
      return false;
    }
    if (w == 0 || local.count < 0) {
      __atomic_store_n(&R.err, 1, __ATOMIC_RELAXED);
      return true;
    }
    o = &local;
    if (R.snap) (*R.snap)[(size_t)i] = local;
    if (R.how && (*R.how)[(size_t)i] != 2) (*R.how)[(size_t)i] = 1;
  } else if (R.dev) {
    o = R.fin + i;
  } else {
    host_sort_finish(R.scores + (size_t)i * (size_t)D.n_cand, D, C, P, G, scratch, local);
    o = &local;
  }
  if (argmax_flat) argmax_flat[s] = o->front_idx;
  responses[s] = complete_window(*o, C, P, G, poses + 3 * s, covs + 9 * s, R.skip_lists);
  return true;
}

// A signalled level with the fast pass's early signal: wait for it. The
// windows it settled are then completed while the exact pass sorts the rest;
// which are which, each window's seal says (level_complete_one's defer).
int level_wait_fast(csm_ctx* c, const LevelRun& R) {
  const double t1 = now_ms();
  const int st = wait_flag(c, R.pend, R.pend.fast_flag);
  if (st != CSM_OK) return st;
  if (c->profiling) c->account("host:wait_fast", (float)(now_ms() - t1), 0.0, 0.0);
  return CSM_OK;
}

// Windows [w0, w1) of R through body(i, defer), on the pool. joined: the level
// is joined, every window is whole. Otherwise its fast pass has signalled
// (level_wait_fast): the windows it settled while the exact pass sorts the
// rest (body returns false for a window the exact pass still owes), then the
// join, then the owed ones.
template <class Body>
int level_complete(csm_ctx* c, LevelRun& R, bool joined, int w0, int w1, int threads, Body&& body) {
  if (joined) {
    c->parallel_for(w1 - w0, threads, [&](int i) { body(w0 + i, false); });
    return CSM_OK;
  }
  std::vector<int> owed((size_t)(w1 - w0));
  int n_owed = 0;
  c->parallel_for(w1 - w0, threads, [&](int i) {
    if (!body(w0 + i, true)) owed[(size_t)__atomic_fetch_add(&n_owed, 1, __ATOMIC_RELAXED)] = w0 + i;
  });
  const int st = level_join(c, R);
  if (st != CSM_OK) return st;
  c->parallel_for(n_owed, n_owed >= 32 ? threads : 1, [&](int k) { body(owed[(size_t)k], false); });
  return CSM_OK;
}

}  // namespace

int level_end(csm_ctx* c, LevelRun& R, double* poses, double* covs, double* responses,
              int64_t* argmax_flat) {
  const int nw = (int)R.scan_of.size();
  if (nw == 0) return CSM_OK;
  int st;
  const Geometry G(c->info);
  const int threads = (nw >= 64) ? c->host_threads : 1;
  const bool early = R.dev && R.pend.fast_flag;  // settled windows while the exact pass runs
  if ((st = early ? level_wait_fast(c, R) : level_join(c, R)) != CSM_OK) return st;
  const double t2 = now_ms();
  if ((st = level_complete(c, R, !early, 0, nw, threads, [&](int i, bool defer) {
         return level_complete_one(R, G, poses, covs, responses, argmax_flat, i, defer);
       })) != CSM_OK)
    return st;
  if ((st = level_check(c, R)) != CSM_OK) return st;
  if (threads > 1) c->account_pool("complete");
  if (c->profiling) {
    const float tc = (float)(now_ms() - t2);
    char nm[48];
    std::snprintf(nm, sizeof(nm), "host:complete<%lld>", (long long)R.D.n_cand);
    c->account("host:complete", tc, 0.0, 0.0);
    c->account(nm, tc, 0.0, 0.0);
  }
  return CSM_OK;
}

// level_end of R followed by level_begin of the next level N over the same
// scans, fused: one pass of the host pool completes window i (its new pose)
// and plans its next window right away, so the pool wakes once per level
// transition instead of twice and the next launch goes out one pool round
// trip earlier (the 3-level driver's critical path). `sum`
// accumulates each scan's response (ScanMatchers::ScanMatch :252-256) before
// the next level overwrites it. N's angle rows go to the other pinned buffer
// of the slot: R's rows are still being read.
// split: N goes out in two spans, its first half as soon as R's first half is
// completed (owed windows included, after the join), then the second half --
// for the hand-off nothing else on the device hides (the last part's
// fine -> super-fine: the device has only the other part's short super-fine
// level to run meanwhile).
int level_end_begin(csm_ctx* c, LevelRun& R, LevelRun& N, int32_t n_scans, const int64_t* offsets,
                    const csm_param& P, double* poses, double* covs, double* responses, double* sum,
                    const int32_t* scan_grid, int skip_lists, bool split) {
  const double tq = c->profiling ? now_ms() : 0.0;
  int st = level_prepare(c, n_scans, offsets, P, responses, nullptr, N, scan_grid, skip_lists, false);
  if (st != CSM_OK) return st;
  if (c->profiling) c->account("host:transition:prepare", (float)(now_ms() - tq), 0.0, 0.0);
  const int nw = (int)R.scan_of.size();
  if (N.scan_of != R.scan_of || nw == 0) {  // not the same windows: one after the other
    if ((st = level_end(c, R, poses, covs, responses, nullptr)) != CSM_OK) return st;
    for (int s = 0; s < n_scans; ++s) sum[s] += responses[s];
    return level_begin(c, n_scans, offsets, P, poses, responses, nullptr, N, scan_grid, skip_lists);
  }
  const bool early = R.dev && R.pend.fast_flag;
  if ((st = early ? level_wait_fast(c, R) : level_join(c, R)) != CSM_OK) return st;
  const double t2 = now_ms();
  std::swap(c->h_angles, c->h_angles_next);
  const Geometry G(c->info);
  // (in two spans only when N's one decision is settled before its first: its
  // maxima are level_prepare's, its windows are bounded in fixed-point range
  // from R's; otherwise one launch after completion)
  split = split && early && nw >= c->split_handoff_min && level_device_finish(c, N.D, nw) &&
          (!c->int_ok || handoff_in_range(c, R, N, G));
  if ((st = level_alloc(c, offsets, N, c->h_angles, split)) != CSM_OK) return st;
  if (split) {
    N.shape.in_range = true;
    N.range_preset = true;
  }
  const int threads = (nw >= 64) ? c->host_threads : 1;
  auto one = [&](int i, bool defer) {
    if (!level_complete_one(R, G, poses, covs, responses, nullptr, i, defer)) return false;
    const int s = R.scan_of[(size_t)i];
    sum[s] += responses[s];
    level_plan_one(c, N, G, offsets, poses, i);
    return true;
  };
  if (split) {  // [0, h) completed, planned and scored while [h, nw) is completed and planned
    const int h = nw / 2;
    if ((st = level_complete(c, R, false, 0, h, threads, one)) != CSM_OK) return st;
    if ((st = level_check(c, R)) != CSM_OK) return st;
    if ((st = level_launch(c, N, WinSpan{0, h, true, false})) != CSM_OK) return st;
    st = level_complete(c, R, true, h, nw, threads, one);
  } else {
    st = level_complete(c, R, !early, 0, nw, threads, one);
  }
  if (st != CSM_OK || (st = level_check(c, R)) != CSM_OK) return st;
  N.int_known = true;  // every window of N planned
  if (threads > 1) c->account_pool("complete+plan");
  const double t3 = now_ms();
  if (split) {
    if ((st = level_launch(c, N, WinSpan{nw / 2, nw, true, false})) != CSM_OK ||
        (st = level_launch(c, N, WinSpan{0, nw, false, true})) != CSM_OK)
      return st;
  } else if ((st = level_launch(c, N)) != CSM_OK) {
    return st;
  }
  if (c->profiling) {
    c->account("host:launch", (float)(now_ms() - t3), 0.0, 0.0);
    c->account("host:complete+plan", (float)(t3 - t2), 0.0, 0.0);
    char nm[48];
    std::snprintf(nm, sizeof(nm), "host:complete+plan<l%d,p%d>", R.tag / 8, R.tag % 8);
    if (R.tag >= 0) c->account(nm, (float)(t3 - t2), 0.0, 0.0);
  }
  return CSM_OK;
}

int match_level(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P,
                double* poses, double* covs, double* responses, int64_t* argmax_flat,
                const int32_t* scan_grid, int skip_lists) {
  if (P.type == CSM_FAST) return match_level_fast(c, n_scans, offsets, P, poses, covs, responses, argmax_flat);
  LevelRun R;
  int st = level_begin(c, n_scans, offsets, P, poses, responses, argmax_flat, R, scan_grid, skip_lists);
  if (st != CSM_OK) return st;
  return level_end(c, R, poses, covs, responses, argmax_flat);
}

}  // namespace csmh
