// csm_search_entry.cpp — the C-ABI's pooled-search entry points (include/csm.h):
// csm_search_windows, csm_search_match, csm_search_gated, and the test hooks csm_search_collect,
// csm_search_bounds and csm_list_select, each under staged_call (csm_host.hpp).
// Here: the plan and the staging they share, the profiling accounts, and
// csm_search_match's paths. The search itself is PyramidSearch (csm_search.cpp,
// csm_pyramid.hip), the finish over a collected list csm_search_match.cpp.
#include "csm_host.hpp"
#include "csm_search_gate.hpp"

using namespace csmh;

namespace {

// csm_search_windows' fallback: the exhaustive per-window argmax, reduced to
// the lowest (window, flat) among the best scores.
int search_exhaustive(csm_ctx* c, const csm_param& P, const Dims& D, const Geometry& G,
                      const std::vector<WindowPlan>& plans, const std::vector<AngleEntry>& angles,
                      const std::vector<int32_t>& gidx, BestPartial* out) {
  std::vector<BestPartial> bp(plans.size());
  std::vector<int64_t> pt_off(plans.size(), 0);
  int st = run_windows(c, P, D, G, plans, pt_off, angles.data(), angles.size(), gidx, bp.data());
  if (st != CSM_OK) return st;
  BestPartial b{-DBL_MAX, INT64_MAX};
  for (size_t i = 0; i < bp.size(); ++i) {
    const int64_t gf = (int64_t)i * D.n_cand + bp[i].flat;
    if (bp[i].score > b.score || (bp[i].score == b.score && gf < b.flat)) b = BestPartial{bp[i].score, gf};
  }
  *out = b;
  return CSM_OK;
}

// What the entry points share. search_plan: the windows planned, the points
// on the device, the fixed-point grid in place, the top depth chosen and the
// pooled search's preconditions tested (ok, box_ok). search_stage: the windows
// and the angle table on the device and the pooled search's inputs filled in.
struct SearchPlan {
  Dims D;
  std::vector<WindowPlan> plans;
  std::vector<AngleEntry> angles;
  std::vector<int32_t> gidx;
  AngleEntry* h_ang = nullptr;  // the angle table in the pinned staging buffer
  double f = 1.0;               // window step in cells
  int depth = 0;
  bool ok = false, box_ok = true;
};

int search_plan(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                const int32_t* grid_index, const double* centers_map, int max_depth, const Geometry& G,
                SearchPlan& sp) {
  Dims& D = sp.D;
  std::vector<WindowPlan>& plans = sp.plans;
  std::vector<AngleEntry>& angles = sp.angles;
  std::vector<int32_t>& gidx = sp.gidx;
  int st = window_dims(*param, D);
  if (st != CSM_OK) return c->fail(st, "invalid search window parameters");
  if (n_points <= 0) return c->fail(CSM_ERR_INVALID_ARG, "no points");
  if ((st = check_points(c, pts, n_points)) != CSM_OK) return st;
  if (!c->has_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  gidx.assign((size_t)n_windows, 0);
  for (int i = 0; i < n_windows; ++i) {
    gidx[(size_t)i] = grid_index ? grid_index[i] : 0;
    if (gidx[(size_t)i] < 0 || gidx[(size_t)i] >= c->n_grids)
      return c->fail(CSM_ERR_INVALID_ARG, "grid_index outside the resident grid stack");
  }
  plans.assign((size_t)n_windows, WindowPlan{});
  if (!plan_windows_shared(*param, D, G, n_points, n_windows, centers_map, angles, plans))
    return c->fail(CSM_ERR_INVALID_ARG, "use_point_size <= 1 with n_points >= 2*use_point_size");
  // the points, then the angle table, staged in pinned memory (the last call
  // on this context has synchronised, so the staging buffer is free)
  const size_t pts_bytes = ((size_t)n_points * 2 * sizeof(double) + 255) & ~(size_t)255;
  hipError_t e0;
  if ((e0 = c->h_search.ensure(pts_bytes + angles.size() * sizeof(AngleEntry))) != hipSuccess)
    return c->hip_fail(e0, "hipHostMalloc(search staging)");
  sp.h_ang = (AngleEntry*)((char*)c->h_search.p + pts_bytes);
  std::memcpy(sp.h_ang, angles.data(), angles.size() * sizeof(AngleEntry));
  if ((st = upload_points(c, pts, n_points, c->h_search.p)) != CSM_OK) return st;
  if ((st = ensure_int_grid(c)) != CSM_OK) return st;
  const double f = sp.f = param->search_space_resolution / G.mres;
  const WindowPlan& W0 = plans[0];
  // the pooled search: one-cell steps, the exact fixed-point grid, the beams
  // staged in LDS (64 KB), every index int-castable, node fields in range
  bool ok = f == 1.0 && c->int_ok && W0.n_used <= 4096 && n_windows < (1 << 20) && D.n_angles < 4096 &&
            D.n_space < 65536 &&
            (double)W0.n_used * c->int_max_abs * std::ldexp(1.0, c->int_exp) <= std::ldexp(1.0, 53);
  int depth = max_depth;
  if (depth < 0) {  // the shallowest top level with at most 32 x 32 nodes per angle (measured
                    // best on configs 3 and 4: profiles/r02/search_depth_sweep.txt)
    depth = 0;
    while (((D.n_space + (1 << depth) - 1) >> depth) > 32 && depth < csm::kPyrMaxDepth) ++depth;
  }
  depth = std::min(depth, csm::kPyrMaxDepth);
  bool box_ok = true;
  for (const WindowPlan& W : plans) {
    if (!ok) break;
    const double far = (double)(D.n_space - 1) * f;
    const double span = std::max(std::max(std::fabs(W.x0), std::fabs(W.x0 + far)),
                                 std::max(std::fabs(W.y0), std::fabs(W.y0 + far)));
    const double R = c->pts_maxabs * (1.0 + 1e-9) + span + 2.0 + (double)(1 << depth);
    if (!(R < std::ldexp(1.0, 29))) ok = false;
    // the top kernel's box test: every |t| < 2^24 cells (csm_pyramid.hip)
    if (!(R < std::ldexp(1.0, 23))) box_ok = false;
  }
  sp.depth = depth;
  sp.ok = ok;
  sp.box_ok = box_ok;
  return CSM_OK;
}

int search_stage(csm_ctx* c, const csm_param* param, const Geometry& G, const SearchPlan& sp, int top_mode,
                 csm::PyrInputs& in) {
  const Dims& D = sp.D;
  const std::vector<WindowPlan>& plans = sp.plans;
  const WindowPlan& W0 = plans[0];
  hipError_t e;
  const int nw = (int)plans.size();
  if ((e = c->h_sw.ensure((size_t)nw * sizeof(ScanWork))) != hipSuccess) return c->hip_fail(e, "hipHostMalloc(scans)");
  ScanWork* sw = (ScanWork*)c->h_sw.p;
  for (int i = 0; i < nw; ++i) {
    const WindowPlan& W = plans[(size_t)i];
    ScanWork& s = sw[i];
    s = ScanWork{};
    s.angle_off = W.angle_off;
    s.out_off = (int64_t)i * D.n_cand;
    s.n_used = W.n_used;
    s.step = W.step;
    s.divisor = (double)W.use;
    s.x0 = W.x0;
    s.y0 = W.y0;
    s.cx = W.center[0];
    s.cy = W.center[1];
    s.ct = W.center[2];
    s.grid_index = sp.gidx[(size_t)i];
  }
  if ((e = c->scans.ensure((size_t)nw * sizeof(ScanWork))) != hipSuccess) return c->hip_fail(e, "hipMalloc(scans)");
  if ((e = c->angles.ensure(sp.angles.size() * sizeof(AngleEntry))) != hipSuccess) return c->hip_fail(e, "hipMalloc(angles)");
  if ((e = hipMemcpyAsync(c->scans.p, sw, (size_t)nw * sizeof(ScanWork), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(scans)");
  if ((e = hipMemcpyAsync(c->angles.p, sp.h_ang, sp.angles.size() * sizeof(AngleEntry), hipMemcpyHostToDevice,
                          c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(angles)");
  in = csm::PyrInputs{};
  in.stream = c->stream;
  LevelWork& L = in.L;
  L.n_angles = D.n_angles;
  L.n_space = D.n_space;
  L.n_cand = D.n_cand;
  L.n_scans = nw;
  L.step_cells = sp.f;
  L.use_penalty = param->use_center_penalty ? 1 : 0;
  L.dist_gain = (param->type == CSM_COARSE) ? 0.4 : 0.2;  // :759-761
  L.size = param->search_space_size;
  L.mres = G.mres;
  L.outside_i = c->outside_i;
  L.int_mode = 1;
  L.int_scale = std::ldexp(1.0, -c->int_exp);
  in.level0 = csm::PyrGrid{c->d_gridi, c->gridi_cells(), c->pitch, 0,
                           c->info.size_x, c->info.size_y, 0, c->info.size_x, 0, 0};
  in.n_grids = c->n_grids;
  in.grid_gen = c->grid_gen;
  in.scans = (const ScanWork*)c->scans.p;
  in.angles = (const AngleEntry*)c->angles.p;
  in.pts = (const double*)c->pts.p;
  in.n_used = W0.n_used;
  in.step = W0.step;
  in.depth = sp.depth;
  in.top_mode = top_mode;
  in.box_ok = sp.box_ok ? 1 : 0;
  in.timed = c->profiling ? 1 : 0;
  in.one_scan = 1;  // the windows share the one scan: check what the implicit top level relies on
  for (const WindowPlan& W : plans)
    if (W.use != W0.use || W.n_used != W0.n_used || W.step != W0.step) in.one_scan = 0;
  return CSM_OK;
}

// csm_search_windows once locked; sp and in are left as the search used them
// (in is filled only when sp.ok: the pooled search ran).
int search_windows_core(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                        const int32_t* grid_index, const double* centers_map, const csm_search_options* options,
                        const Geometry& G, SearchPlan& sp, csm::PyrInputs& in, csm_best* best, int32_t* best_window,
                        csm_search_stats* stats) {
  int st = search_plan(c, pts, n_points, param, n_windows, grid_index, centers_map, options ? options->max_depth : -1,
                       G, sp);
  if (st != CSM_OK) return st;
  const Dims& D = sp.D;
  const WindowPlan& W0 = sp.plans[0];
  csm_search_stats S{};
  S.candidates = (int64_t)n_windows * D.n_cand;
  BestPartial b{};
  if (!sp.ok) {
    S.exhaustive = 1;
    if ((st = search_exhaustive(c, *param, D, G, sp.plans, sp.angles, sp.gidx, &b)) != CSM_OK) return st;
    S.nodes[0] = S.candidates;
    S.beam_reads = S.candidates * W0.n_used;
  } else {
    hipError_t e;
    if ((st = search_stage(c, param, G, sp, options ? options->top_kernel : 0, in)) != CSM_OK) return st;
    c->pyramid.configure(options ? options->node_capacity : 0, options ? options->probe_min_nodes : 0);
    csm::PyrStats ps;
    std::string what;
    float ms = 0.f;
    if ((st = c->span_begin("hipEventRecord")) != CSM_OK) return st;
    if ((e = c->pyramid.run(in, &b, &ps, &what)) != hipSuccess) return c->hip_fail(e, what.c_str());
    if ((st = c->span_end(&ms, "pyramid timing")) != CSM_OK) return st;
    S.depth = ps.depth;
    int64_t scored = ps.probe_leaves;
    for (int d = 0; d <= csm::kPyrMaxDepth; ++d) {
      S.nodes[d] = ps.nodes[d];
      scored += ps.nodes[d];
    }
    S.probe_leaves = ps.probe_leaves;
    S.beam_reads = scored * W0.n_used;
    S.build_ms = ps.build_ms;
    S.syncs = ps.syncs;
    S.top_box = ps.top_box;
    // one grid read per beam per scored node (the pooled levels included)
    if (c->profiling) {
      c->account("pyramid_search", ms, (double)S.beam_reads * 4.0, (double)S.candidates);
      if (ps.top_name[0]) c->account(ps.top_name, (float)ps.top_ms, ps.top_bytes, 0.0);
      // the bound launches per depth (one int16 / int32 pooled value per node and beam)
      for (int d = 0; d <= csm::kPyrMaxDepth; ++d) {
        const int nl = ps.bound_launches[d];
        if (nl <= 0) continue;
        const double bytes = (double)ps.nodes[d] * W0.n_used * (d == 0 ? 4.0 : 2.0);
        for (int k = 0; k < nl; ++k)
          c->account(d == 0 ? "pyr_bound_kernel<int>" : "pyr_bound_kernel<short>", (float)(ps.bound_ms[d] / nl),
                     bytes / nl, 0.0);
      }
    }
  }
  if (b.flat == INT64_MAX) return c->fail(CSM_ERR_HIP, "search found no candidate");
  const int32_t w = (int32_t)(b.flat / D.n_cand);
  *best = best_of(D, sp.plans[(size_t)w], sp.angles.data(), sp.f, b.score, b.flat - (int64_t)w * D.n_cand);
  *best_window = w;
  if (stats) *stats = S;
  return CSM_OK;
}

// csm_search_match's winner window after phase 1, as its steps hand it on.
struct Winner {
  const SearchPlan& sp;
  const WindowPlan& W;
  int32_t w;               // its index among the call's windows
  csm::PyrInputs one;      // the search's inputs narrowed to it
  csm::FinishWindow FW;
  double best;             // its best score
  int64_t n_found = 0;     // collect_winner: its candidates at or above the bound ...
  int64_t capacity = 0;    // ... and the device list's room for them
};

// csm_search_match's paths 1-3: every score of the winner on its grid of the
// stack, then the reference's finish over all of them (std::sort, the three
// ordered scans: host_sort_finish) -- what csm_scan_match gives for the window.
int match_exhaustive(csm_ctx* c, const csm_param* param, const Geometry& G, const Winner& N, double cov[9],
                     csm::FinishOut& o, double pose_map[3], double* response) {
  const SearchPlan& sp = N.sp;
  const std::vector<WindowPlan> one{N.W};
  int st = run_windows(c, *param, sp.D, G, one, {0}, sp.angles.data(), sp.angles.size(), {sp.gidx[(size_t)N.w]}, nullptr);
  if (st != CSM_OK) return st;
  const int64_t ns = sp.D.n_space;
  const CandGeom C{one[0], sp.angles.data() + one[0].angle_off, sp.f, ns, ns * ns};
  thread_local std::vector<Entry> scratch;  // kept between calls, as level_complete_one's (16 bytes a candidate)
  host_sort_finish((const double*)c->h_scores.p, sp.D, C, *param, G, scratch, o);
  *response = csm::finish_complete(o, N.FW, 0, pose_map, cov);
  if (c->profiling) c->account("search_match:exhaustive", 0.f, 0.0, (double)sp.D.n_cand);  // launches: the count
  return CSM_OK;
}

// One descent of the winner for its candidates at or above R->threshold, left
// on the device in a list of `capacity` entries: N.n_found counts them all.
// growing: a list that cannot be allocated sets *no_room and is no error.
int collect_once(csm_ctx* c, Winner& N, int64_t capacity, bool growing, csm_match_result* R, bool* no_room) {
  csm::PyrStats ps;
  std::string what;
  hipError_t e;
  float ms = 0.f;
  int st = c->span_begin("hipEventRecord");
  if (st != CSM_OK) return st;
  if ((e = c->pyramid.collect_device(N.one, R->threshold, capacity, &N.n_found, &ps, &what)) != hipSuccess) {
    if (!growing || e != hipErrorOutOfMemory) return c->hip_fail(e, what.c_str());
    (void)hipGetLastError();
    *no_room = true;
    return CSM_OK;
  }
  int64_t bounded = 0;
  for (int d = 0; d <= csm::kPyrMaxDepth; ++d) bounded += (R->collect_nodes[d] = ps.collect_nodes[d]);
  if ((st = c->span_end(&ms, "collect timing")) != CSM_OK) return st;
  if (c->profiling) c->account("pyr_collect", ms, (double)bounded * N.W.n_used * 4.0, (double)N.sp.D.n_cand);
  return CSM_OK;
}

// Phase 2: the winner's candidates at or above T, by the same descent, left
// on the device. asked: csm_match_options::collect_capacity.
int collect_winner(csm_ctx* c, Winner& N, int64_t asked, csm_match_result* R) {
  const bool auto_cap = asked == CSM_COLLECT_AUTO;
  // automatic: the list as large as it ever grew on this context
  N.capacity = auto_cap ? std::max<int64_t>(csm::kFinishMaxCand, c->pyramid.list_capacity())
                        : (asked > 0 ? asked : csm::kFinishMaxCand);
  bool no_room = false;  // the grown list could not be allocated
  int st = collect_once(c, N, N.capacity, false, R, &no_room);
  if (st != CSM_OK) return st;
  constexpr int64_t kAutoMax = (int64_t)1 << 26;  // entries: 1 GiB
  if (auto_cap && N.n_found > N.capacity && N.n_found <= std::min<int64_t>(N.sp.D.n_cand, kAutoMax)) {
    // the list grows to what was counted (and stays so), one more descent
    const int64_t counted = N.n_found;
    if ((st = collect_once(c, N, counted, true, R, &no_room)) != CSM_OK) return st;
    if (no_room) {  // csm_search_match's path 2
      N.n_found = counted;
    } else {
      N.capacity = counted;
      if (c->profiling) c->account("search_match:regrown", 0.f, 0.0, (double)N.n_found);
    }
  }
  return CSM_OK;
}

// PyramidSearch::select over the first n entries of the device list, timed and
// accounted as one "list_select". run(select) makes the selections and says
// whether all went well: select(spec, out, cap) -> the selection's full count,
// < 0 when it failed (reduced_finish's contract, csm_search_match.hpp).
template <class Run>
int timed_select(csm_ctx* c, int64_t n, Run&& run) {
  std::string what;
  hipError_t e = hipSuccess;
  float ms = 0.f;
  int launches = 0;
  auto select = [&](const csm::SelectSpec& spec, csm::PyrHit* out, int64_t cap) -> int64_t {
    int64_t n_sel = 0;
    int nl = 0;
    if ((e = c->pyramid.select(spec, n, out, cap, &n_sel, &nl, c->stream, &what)) != hipSuccess) return -1;
    launches += nl;
    return n_sel;
  };
  int st = c->span_begin("hipEventRecord");
  if (st != CSM_OK) return st;
  if (!run(select)) return c->hip_fail(e, what.c_str());
  if ((st = c->span_end(&ms, "select timing")) != CSM_OK) return st;
  if (c->profiling) {
    // the events span the selections (the host's sort of A lies between them); every
    // histogram pass and the compaction read the list once: launches / 2 reads
    c->account("list_select", ms, (double)n * sizeof(csm::PyrHit) * (launches / 2.0), (double)n);
    if (launches > 1) c->account_count("list_select", launches - 1);
  }
  return CSM_OK;
}

// The finish over the collected list: from the device selection's subset when
// the list is longer than the context's reduce minimum (the reduced finish,
// csm_search_match.hpp), else -- or when a selection outgrew its room -- over
// the whole list fetched.
int finish_collected(csm_ctx* c, const Winner& N, double cov[9], csm::ListFinish* LF) {
  thread_local std::vector<csm::PyrHit> hits;  // kept between calls (16 bytes a candidate)
  const int64_t n_found = N.n_found;
  if (n_found > c->list_reduce_min) {
    const int64_t max_sel = csm::kFinishMaxCand;
    if (hits.size() < (size_t)(3 * max_sel)) hits.resize((size_t)(3 * max_sel));
    csm::Reduced red = csm::Reduced::kFailed;
    const int st = timed_select(c, n_found, [&](auto& select) {
      red = csm::reduced_finish(select, hits.data(), hits.data() + 2 * max_sel, max_sel, N.best, N.FW, cov, LF);
      return red != csm::Reduced::kFailed;
    });
    if (st != CSM_OK) return st;
    if (c->profiling)
      c->account(red == csm::Reduced::kDone ? "search_match:reduced" : "search_match:reduce_overflow", 0.f, 0.0,
                 (double)n_found);
    if (red == csm::Reduced::kDone) return CSM_OK;
  }
  std::string what;
  hipError_t e;
  if (hits.size() < (size_t)n_found) hits.resize((size_t)n_found);
  if ((e = c->pyramid.fetch(n_found, hits.data(), c->stream, &what)) != hipSuccess) return c->hip_fail(e, what.c_str());
  csm::list_finish(hits.data(), n_found, N.FW, cov, LF);
  return CSM_OK;
}

// csm_search_match once locked: paths 0-5 of csm.h, top to bottom.
int search_match_locked(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                        const int32_t* grid_index, const double* centers_map, const csm_match_options* options,
                        double cov[9], csm_match_result* R) {
  const Geometry G(c->info);
  SearchPlan sp;
  csm::PyrInputs in{};
  *R = csm_match_result{};
  // phase 1: the winner window and its argmax
  int st = search_windows_core(c, pts, n_points, param, n_windows, grid_index, centers_map,
                               options ? &options->search : nullptr, G, sp, in, &R->front, &R->window, &R->search);
  if (st != CSM_OK) return st;
  const WindowPlan& W = sp.plans[(size_t)R->window];
  const double best = R->front.score;
  R->response = best > 1.0 ? 1.0 : best;  // :861-863
  R->threshold = csm::cov_bound(best);
  R->pose_map[0] = R->front.x;
  R->pose_map[1] = R->front.y;
  R->pose_map[2] = R->front.angle;
  if (options && options->min_response != 0.0 && best < options->min_response) {
    R->path = CSM_MATCH_LOW_RESPONSE;
    return CSM_OK;
  }
  Winner N{sp, W, R->window, in,
           csm::FinishWindow{csm::CandGrid{W.x0, W.y0, sp.f, sp.D.n_space}, sp.angles.data() + W.angle_off, param->type,
                             G.mres, param->search_space_resolution, param->search_angle_resolution},
           best};
  N.one.L.n_scans = 1;
  N.one.scans = in.scans + R->window;
  N.one.one_scan = 1;
  csm::FinishOut o{};
  double response = 0.0;
  auto finished = [&](int path) {  // paths 0-3: the finish's outputs
    R->path = path;
    R->response = response;
    R->accepted = response > param->response_threshold ? 1 : 0;  // :866
    R->front = best_of(sp.D, W, sp.angles.data(), sp.f, o.best_score, o.front_idx);
    R->count = o.count;
    return CSM_OK;
  };
  auto exhaustive = [&](int path) {  // paths 1-3: the finish over every score of the window
    const int est = match_exhaustive(c, param, G, N, cov, o, R->pose_map, &response);
    return est != CSM_OK ? est : finished(path);
  };
  if (!sp.ok) return exhaustive(CSM_MATCH_UNPOOLED);
  if (best < kDoubleTolerance && !(R->response > param->response_threshold)) {
    // the covariances' early return (:894-899, :973-976) reads no candidate
    o.front_idx = (int32_t)R->front.flat_index;
    o.count = 1;
    o.best_score = best;
    o.best_x = R->front.x;
    o.best_y = R->front.y;
    double unused[3];
    (void)csm::finish_complete(o, N.FW, 0, unused, cov);
    R->path = CSM_MATCH_NO_RESPONSE;
    return CSM_OK;
  }
  // phase 2: the winner's candidates at or above T left on the device, then their finish
  if ((st = collect_winner(c, N, options ? options->collect_capacity : 0, R)) != CSM_OK) return st;
  R->collected = N.n_found;
  if (N.n_found < 1) return c->fail(CSM_ERR_HIP, "collect: the best candidate is not in its own set");
  if (N.n_found > N.capacity) return exhaustive(CSM_MATCH_OVERFLOW);
  csm::ListFinish LF;
  if ((st = finish_collected(c, N, cov, &LF)) != CSM_OK) return st;
  if (LF.tie_matters) return exhaustive(CSM_MATCH_TIE);
  o = LF.o;
  response = LF.response;
  for (int k = 0; k < 3; ++k) R->pose_map[k] = LF.pose_map[k];
  return finished(CSM_MATCH_PRUNED);
}

// csm_search_collect once locked: the search at `depth` (it builds the pooled
// levels), then the collect at `threshold`.
int search_collect_locked(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t grid_index,
                          const double center_map[3], int32_t depth, double threshold, int64_t* flat, double* score,
                          int64_t capacity, int64_t* n_found) {
  if (depth < 0 || depth > csm::kPyrMaxDepth) return c->fail(CSM_ERR_INVALID_ARG, "depth must be in [0, 10]");
  const Geometry G(c->info);
  SearchPlan sp;
  int st = search_plan(c, pts, n_points, param, 1, &grid_index, center_map, depth, G, sp);
  if (st != CSM_OK) return st;
  if (!sp.ok) return c->fail(CSM_ERR_UNSUPPORTED, "the window is outside the pooled search (step, grid or range)");
  csm::PyrInputs in{};
  if ((st = search_stage(c, param, G, sp, 0, in)) != CSM_OK) return st;
  in.timed = 0;
  c->pyramid.configure(0, 0);
  BestPartial b{};
  std::string what;
  hipError_t e;
  if ((e = c->pyramid.run(in, &b, nullptr, &what)) != hipSuccess) return c->hip_fail(e, what.c_str());
  const int64_t cap = std::max<int64_t>(capacity, 1);
  std::vector<csm::PyrHit> hits((size_t)cap);
  if ((e = c->pyramid.collect(in, threshold, cap, hits.data(), n_found, nullptr, &what)) != hipSuccess)
    return c->hip_fail(e, what.c_str());
  const int64_t n = std::min(*n_found, capacity);
  std::sort(hits.begin(), hits.begin() + n, [](const csm::PyrHit& a, const csm::PyrHit& b2) { return a.flat < b2.flat; });
  for (int64_t i = 0; i < n; ++i) {
    flat[i] = hits[(size_t)i].flat;
    score[i] = hits[(size_t)i].score;
  }
  return CSM_OK;
}

// csm_search_bounds once locked: the same plan, staging and pooled levels as
// csm_search_windows; no probe, no expand, no incumbent.
int search_bounds_locked(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                         const int32_t* grid_index, const double* centers_map, int32_t depth, int32_t kernel,
                         double* bounds, int64_t* sums, int64_t n_out) {
  if (depth < 1 || depth > csm::kPyrMaxDepth) return c->fail(CSM_ERR_INVALID_ARG, "depth must be in [1, 10]");
  const Geometry G(c->info);
  SearchPlan sp;
  int st = search_plan(c, pts, n_points, param, n_windows, grid_index, centers_map, depth, G, sp);
  if (st != CSM_OK) return st;
  if (!sp.ok) return c->fail(CSM_ERR_UNSUPPORTED, "the window is outside the pooled search (step, grid or range)");
  const int64_t nj = ((int64_t)sp.D.n_space + (1 << depth) - 1) >> depth;
  if (n_out != (int64_t)n_windows * sp.D.n_angles * nj * nj)
    return c->fail(CSM_ERR_INVALID_ARG, "n_out must be n_windows * n_angles * nj^2");
  csm::PyrInputs in{};
  if ((st = search_stage(c, param, G, sp, kernel == 0 ? 0 : 1, in)) != CSM_OK) return st;
  in.timed = 0;
  std::string what;
  bool unsupported = false;
  const hipError_t e = c->pyramid.top_bounds(in, kernel, bounds, sums, n_out, &unsupported, &what);
  if (unsupported) return c->fail(CSM_ERR_UNSUPPORTED, what.c_str());
  if (e != hipSuccess) return c->hip_fail(e, what.c_str());
  return CSM_OK;
}

// One passing window's entry, when there is room for it.
void gated_put(const SearchPlan& sp, const csm::GatePass& g, int64_t k, int32_t* windows_out, csm_best* best_out) {
  windows_out[k] = g.window;
  best_out[k] = best_of(sp.D, sp.plans[(size_t)g.window], sp.angles.data(), sp.f, g.score, g.flat);
}

// csm_search_gated's fallbacks: the exhaustive per-window argmax, filtered.
int gated_exhaustive(csm_ctx* c, const csm_param* param, const Geometry& G, const SearchPlan& sp, double T,
                     int32_t* windows_out, csm_best* best_out, int32_t capacity, int32_t* n_pass) {
  std::vector<BestPartial> bp(sp.plans.size());
  std::vector<int64_t> pt_off(sp.plans.size(), 0);
  int st = run_windows(c, *param, sp.D, G, sp.plans, pt_off, sp.angles.data(), sp.angles.size(), sp.gidx, bp.data());
  if (st != CSM_OK) return st;
  int32_t n = 0;
  for (size_t i = 0; i < bp.size(); ++i) {
    if (!(bp[i].score >= T)) continue;
    if (n < capacity) gated_put(sp, csm::GatePass{(int32_t)i, bp[i].score, bp[i].flat}, n, windows_out, best_out);
    ++n;
  }
  *n_pass = n;
  if (c->profiling) c->account("search_gated:exhaustive", 0.f, 0.0, (double)sp.plans.size() * sp.D.n_cand);
  return CSM_OK;
}

// csm_search_gated once locked.
int search_gated_locked(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                        const int32_t* grid_index, const double* centers_map, double T, const csm_gate_options* options,
                        int32_t* windows_out, csm_best* best_out, int32_t capacity, int32_t* n_pass,
                        csm_gate_stats* stats) {
  const Geometry G(c->info);
  SearchPlan sp;
  int st = search_plan(c, pts, n_points, param, n_windows, grid_index, centers_map,
                       options ? options->search.max_depth : -1, G, sp);
  if (st != CSM_OK) return st;
  csm_gate_stats S{};
  S.candidates = (int64_t)n_windows * sp.D.n_cand;
  auto fallback = [&](int path) {
    S.path = path;
    S.descents = 0;
    if (stats) *stats = S;
    return gated_exhaustive(c, param, G, sp, T, windows_out, best_out, capacity, n_pass);
  };
  if (!sp.ok) return fallback(CSM_GATE_UNPOOLED);
  csm::PyrInputs in{};
  if ((st = search_stage(c, param, G, sp, options ? options->search.top_kernel : 0, in)) != CSM_OK) return st;
  c->pyramid.configure(options ? options->search.node_capacity : 0, -1);  // a fixed threshold: no probes
  S.depth = sp.depth;
  const bool fixed = options && options->list_capacity > 0;
  int64_t cap = csm::gate_first_capacity(options ? options->list_capacity : 0, c->pyramid.list_capacity());
  if (cap > csm::kGateMaxList) return fallback(CSM_GATE_OVERFLOW);
  csm::PyramidSearch::GateOut out{};
  for (int descents = 1;; ++descents) {
    csm::PyrStats ps;
    std::string what;
    hipError_t e;
    float ms = 0.f;
    if ((st = c->span_begin("hipEventRecord")) != CSM_OK) return st;
    if ((e = c->pyramid.gate(in, T, cap, descents > 1, &out, &ps, &what)) != hipSuccess) {
      if (e != hipErrorOutOfMemory) return c->hip_fail(e, what.c_str());
      (void)hipGetLastError();  // the list could not be allocated: no error of the context's
      return fallback(CSM_GATE_OVERFLOW);
    }
    if ((st = c->span_end(&ms, "gate timing")) != CSM_OK) return st;
    int64_t bounded = 0;
    for (int d = 0; d <= csm::kPyrMaxDepth; ++d) {
      S.nodes[d] += ps.collect_nodes[d];
      bounded += ps.collect_nodes[d];
    }
    S.build_ms += ps.build_ms;
    S.listed = out.listed;
    S.descents = descents;
    if (c->profiling) {
      c->account("pyr_gate", ms, (double)bounded * sp.plans[0].n_used * 4.0, (double)S.candidates);
      c->account("gate_window_best", 0.f, (double)std::min(out.listed, cap) * sizeof(csm::PyrHit), 0.0);
    }
    int64_t grow_to = cap;
    const csm::GateNext next = csm::gate_after(descents, out.listed, cap, fixed, &grow_to);
    if (next == csm::GateNext::kDone) break;
    if (next == csm::GateNext::kFallback) return fallback(CSM_GATE_OVERFLOW);
    if (next == csm::GateNext::kRedescend && c->profiling)
      c->account("search_gated:redescended", 0.f, 0.0, (double)out.listed);
    cap = grow_to;
  }
  S.path = CSM_GATE_PRUNED;
  thread_local std::vector<csm::GatePass> pass;
  if (pass.size() < (size_t)capacity) pass.resize((size_t)capacity);
  const int64_t n = csm::gate_results(out.wkey, out.wflat, n_windows, sp.D.n_cand, pass.data(), capacity);
  for (int64_t k = 0; k < std::min<int64_t>(n, capacity); ++k) gated_put(sp, pass[(size_t)k], k, windows_out, best_out);
  *n_pass = (int32_t)n;
  if (stats) *stats = S;
  return CSM_OK;
}

}  // namespace

extern "C" {

int csm_search_gated(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                     const int32_t* grid_index, const double* centers_map, double min_response,
                     const csm_gate_options* options, int32_t* windows_out, csm_best* best_out, int32_t capacity,
                     int32_t* n_pass, csm_gate_stats* stats) {
  if (!c || !param || !centers_map || !n_pass || n_windows < 1 || capacity < 0 ||
      (capacity > 0 && (!windows_out || !best_out)) || !(min_response == min_response))
    return CSM_ERR_INVALID_ARG;
  if (param->type == CSM_FAST) return c->fail(CSM_ERR_INVALID_ARG, "csm_search_gated: not for the FAST matcher");
  return staged_call(c, [&] {
    return search_gated_locked(c, pts, n_points, param, n_windows, grid_index, centers_map, min_response, options,
                               windows_out, best_out, capacity, n_pass, stats);
  });
}

int csm_search_windows(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                       const int32_t* grid_index, const double* centers_map, const csm_search_options* options,
                       csm_best* best, int32_t* best_window, csm_search_stats* stats) {
  if (!c || !param || !centers_map || !best || !best_window || n_windows <= 0) return CSM_ERR_INVALID_ARG;
  return staged_call(c, [&] {
    const Geometry G(c->info);
    SearchPlan sp;
    csm::PyrInputs in{};
    return search_windows_core(c, pts, n_points, param, n_windows, grid_index, centers_map, options, G, sp, in, best,
                               best_window, stats);
  });
}

int csm_search_match(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                     const int32_t* grid_index, const double* centers_map, const csm_match_options* options,
                     double cov[9], csm_match_result* result) {
  if (!c || !param || !centers_map || !cov || !result || n_windows <= 0) return CSM_ERR_INVALID_ARG;
  if (param->type == CSM_FAST) return c->fail(CSM_ERR_INVALID_ARG, "csm_search_match: not for the FAST matcher");
  return staged_call(c, [&] {
    return search_match_locked(c, pts, n_points, param, n_windows, grid_index, centers_map, options, cov, result);
  });
}

int csm_search_collect(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t grid_index,
                       const double center_map[3], int32_t depth, double threshold, int64_t* flat, double* score,
                       int64_t capacity, int64_t* n_found) {
  if (!c || !param || !center_map || !n_found || capacity < 0 || (capacity > 0 && (!flat || !score)))
    return CSM_ERR_INVALID_ARG;
  return staged_call(c, [&] {
    return search_collect_locked(c, pts, n_points, param, grid_index, center_map, depth, threshold, flat, score,
                                 capacity, n_found);
  });
}

// Test hook: the search's top-level bounds at `depth`, read out of one of the
// three kernels that compute them (csm.h).
int csm_search_bounds(csm_ctx* c, const double* pts, int32_t n_points, const csm_param* param, int32_t n_windows,
                      const int32_t* grid_index, const double* centers_map, int32_t depth, int32_t kernel,
                      double* bounds, int64_t* sums, int64_t n_out) {
  if (!c || !param || !centers_map || n_windows <= 0 || kernel < 0 || kernel > 2 || (kernel == 0 ? !sums : !bounds))
    return CSM_ERR_INVALID_ARG;
  return staged_call(c, [&] {
    return search_bounds_locked(c, pts, n_points, param, n_windows, grid_index, centers_map, depth, kernel, bounds,
                                sums, n_out);
  });
}

// Test hook: the device selection (csm_select.hpp) over an uploaded list,
// through PyramidSearch::select's launches.
int csm_list_select(csm_ctx* c, const double* score, const int64_t* flat, int64_t n, int32_t k, int32_t band_on,
                    double best, int32_t near_on, const double* near, int64_t* out_flat, double* out_score,
                    int64_t capacity, int64_t* n_out) {
  if (!c || n < 0 || (n > 0 && (!score || !flat)) || k < 1 || capacity < 0 || (capacity > 0 && (!out_flat || !out_score)) ||
      !n_out || (near_on && !near))
    return CSM_ERR_INVALID_ARG;
  return staged_call(c, [&]() -> int {
    if (n > ((int64_t)1 << 26)) return c->fail(CSM_ERR_INVALID_ARG, "n must be at most 2^26");
    csm::SelectSpec spec{};
    spec.k = k;
    spec.band_on = band_on != 0;
    spec.best = best;
    spec.near_on = near_on != 0;
    if (near_on) {
      if (!(near[3] >= 1.0)) return c->fail(CSM_ERR_INVALID_ARG, "near[3] (n_space) must be at least 1");
      spec.grid = csm::CandGrid{near[0], near[1], near[2], (int)near[3]};
      spec.bx = near[4];
      spec.by = near[5];
      spec.tol = near[6];
    } else {
      spec.grid = csm::CandGrid{0.0, 0.0, 1.0, 1};
    }
    std::vector<csm::PyrHit> hits((size_t)std::max<int64_t>(n, capacity));
    for (int64_t i = 0; i < n; ++i) hits[(size_t)i] = csm::PyrHit{score[i], flat[i]};
    std::string what;
    hipError_t e;
    if ((e = c->pyramid.load_list(hits.data(), n, c->stream, &what)) != hipSuccess) return c->hip_fail(e, what.c_str());
    int64_t n_sel = 0;
    const int st = timed_select(c, n, [&](auto& select) { return (n_sel = select(spec, hits.data(), capacity)) >= 0; });
    if (st != CSM_OK) return st;
    *n_out = n_sel;
    const int64_t m = std::min(n_sel, capacity);
    std::sort(hits.begin(), hits.begin() + m, [](const csm::PyrHit& a, const csm::PyrHit& b) { return a.flat < b.flat; });
    for (int64_t i = 0; i < m; ++i) {
      out_flat[i] = hits[(size_t)i].flat;
      out_score[i] = hits[(size_t)i].score;
    }
    return CSM_OK;
  });
}

}  // extern "C"
