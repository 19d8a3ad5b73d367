// csm_pipeline.cpp — the 3-level ScanMatchers driver (scan_matchers.h:179-289)
// over a resident batch, its parts in flight together (PipeJob,
// csm_driver_internal.hpp), and submitted batches: one batch's last level
// pending while the next one's first launch scores.
#include "csm_driver_internal.hpp"
#include "csm_submit_order.hpp"

namespace csmh {
namespace {

// part h of J with its buffer slot swapped in (slot 0 is the context's own)
template <typename F>
int with_slot(csm_ctx* c, const PipeJob& J, int h, F&& f) {
  const int sidx = J.slot0 + h;
  if (sidx > 0) c->swap_slot(sidx);
  const int st = f();
  if (sidx > 0) c->swap_slot(sidx);
  return st;
}

// The order a part's windows take its scans in. Consecutive windows go to
// one XCD (dev::xcd_remap: XCD x takes the x-th eighth of the launch), so the
// scans are ranked by the Morton code of their initial map cell (64-cell
// tiles) and rank m goes to launch position (m % 8) * n / 8 + m / 8: every
// XCD's share spans the whole map (the same work mix on every XCD), and at
// any moment the eight XCDs score windows that lie close together, which
// their L2s and the MALL share. r05 A/B: the pair kernel 0.637
// -> 0.613 ms, the phase kernel 0.252 -> 0.245; ranks in contiguous eighths
// (each XCD one region of the map) made the pair kernel 0.848 ms, the XCDs'
// regions holding unequal work. Scans are independent: no result changes.
// (tests/test_gpu_mixed_batches.py restates this order and job_setup's split
// in Python, _window_order and _parts, to place scans of chosen lengths in
// chosen spans: keep them in step.)
#ifndef CSM_WINDOW_ORDER  // 0: scan order (A/B builds)
#define CSM_WINDOW_ORDER 1
#endif
// (ranked by a stable LSD radix sort of the 32-bit keys, ties in scan order:
// std::sort of 2 x 2048 (key, scan) pairs took ~0.1 ms of the submit's way to
// its first launch, r05)
void window_order(const Geometry& G, const double* poses, int32_t n, std::vector<int32_t>& out) {
  out.resize((size_t)n);
  thread_local std::vector<uint32_t> key, key2;
  thread_local std::vector<int32_t> idx2;
  key.resize((size_t)n);
  key2.resize((size_t)n);
  idx2.resize((size_t)n);
  auto spread = [](uint32_t v) {  // 16 bits -> every other bit
    v &= 0xFFFF;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
  };
  for (int32_t s = 0; s < n; ++s) {
    double m[3];
    G.to_map(poses + 3 * (size_t)s, m);
    const double qx = std::floor(m[0] / 64.0), qy = std::floor(m[1] / 64.0);
    const uint32_t ix = (uint32_t)((int32_t)std::max(-32768.0, std::min(32767.0, qx)) + 32768);
    const uint32_t iy = (uint32_t)((int32_t)std::max(-32768.0, std::min(32767.0, qy)) + 32768);
    key[(size_t)s] = spread(ix) | (spread(iy) << 1);
  }
  // rank[] in `out` (as scratch) then by 8-bit digits, least significant first
  std::vector<int32_t>& idx = out;
  for (int32_t s = 0; s < n; ++s) idx[(size_t)s] = s;
  for (int shift = 0; shift < 32; shift += 8) {
    size_t cnt[257] = {0};
    for (int32_t i = 0; i < n; ++i) ++cnt[((key[(size_t)i] >> shift) & 0xFF) + 1];
    for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
    for (int32_t i = 0; i < n; ++i) {
      const size_t o = cnt[(key[(size_t)i] >> shift) & 0xFF]++;
      key2[o] = key[(size_t)i];
      idx2[o] = idx[(size_t)i];
    }
    key.swap(key2);
    idx.swap(idx2);
  }
  // idx holds the ranked scans (4 swaps: back in `out`); rank m -> position (m % 8) * n / 8 + m / 8
  if (CSM_WINDOW_ORDER == 2) return;  // (A/B: contiguous Morton ranges, each XCD one region)
  idx2.assign(idx.begin(), idx.end());
  int32_t pos = 0;
  for (int x = 0; x < 8; ++x)
    for (int32_t m = x; m < n; m += 8) out[(size_t)pos++] = idx2[(size_t)m];
}

int job_skip(const csm_ctx* c, const PipeJob& J, int l) {
  return c->skip_dead_lists ? live_lists(J.levels, J.n_levels, l) : 0;
}

}  // namespace

PipeState& pipe_of(csm_ctx* c) {
  if (!c->pipe) c->pipe = new PipeState();
  return *static_cast<PipeState*>(c->pipe);
}

// The level transition (l -> l + 1) of part h.
int job_handoff(csm_ctx* c, PipeJob& J, int l, int h) {
  const int32_t s0 = J.first[h];
  J.R[(l + 1) & 1][h].tag = (l + 1) * 8 + h;
  // csm_set_profiling(ctx, 2): the later levels' launches go out without
  // timing events (their records cost ~50 us of kernel-stream gaps a config-2
  // step, profiles/r05/experiments/ab_profile_first_level.txt)
  const bool timed = c->profiling;
  c->profiling = timed && !c->profile_first_level;
  // the last part's last hand-off in two spans: with two parts only the other
  // part's short last level runs meanwhile; a single part's runs under the
  // next batch's whole coarse level (CSM_SINGLE_SPLIT_HANDOFF=1: split too)
  const bool split = (J.K > 1 ? c->split_last_handoff : c->single_split_handoff) && h == J.K - 1 && l + 2 == J.n_levels;
  const int st = with_slot(c, J, h, [&] {
    return level_end_begin(c, J.R[l & 1][h], J.R[(l + 1) & 1][h], J.count[h], J.offsets + s0, J.levels[l + 1],
                           J.poses + 3 * (size_t)s0, J.covs + 9 * (size_t)s0, J.resp.data() + s0, J.sum + s0,
                           J.scan_grid ? J.scan_grid + s0 : nullptr, job_skip(c, J, l + 1),
                           split);
  });
  c->profiling = timed;
  // level l's responses of this part: the next level overwrites them when it completes
  if (st == CSM_OK && J.level_resp)
    for (int s = s0; s < s0 + J.count[h]; ++s) J.level_resp[(size_t)l * J.n_scans + s] = J.resp[(size_t)s];
  return st;
}

// The last part's last level transition (the last launch of J).
static int job_last_handoff(csm_ctx* c, PipeJob& J) {
  if (!J.pending || J.last_handoff_done) return CSM_OK;
  J.last_handoff_done = true;
  return job_handoff(c, J, J.n_levels - 2, J.K - 1);
}

void job_setup(csm_ctx* c, PipeJob& J, int32_t n_scans, const int64_t* offsets, const csm_param* levels,
               int n_levels, double* poses, double* covs, double* sum, const int32_t* scan_grid, int K, int slot0,
               bool submitted) {
  J.K = K;
  // submitted batches split their first span only when the coarse level sums
  // many beams: below that the step is host-bound and the extra launch costs
  // more than the shorter planning at the batch boundary (csm_host.hpp)
  J.first_windows = !submitted ? c->first_windows : coarse_device_bound(c, levels, n_levels) ? c->first_windows_submit : 0;
  const int permille = submitted ? c->part0_permille_submit : c->part0_permille;
  J.n_levels = n_levels;
  J.slot0 = slot0;
  J.n_scans = n_scans;
  J.offsets = offsets;
  J.scan_grid = scan_grid;
  for (int l = 0; l < n_levels; ++l) J.levels[l] = levels[l];
  J.poses = poses;
  J.covs = covs;
  J.sum = sum;
  J.scores = nullptr;
  J.level_resp = nullptr;
  J.pending = false;
  J.last_handoff_done = false;
  // part 0 takes part0_permille of the scans, the others split the rest: a
  // larger first part shortens what nothing hides, the last part's
  // super-fine completion at the end of the call and its fine -> super-fine
  // hand-off (the device has only part 0's super-fine level to run meanwhile)
  // (a single part, submitted batches only, is the whole batch)
  const int64_t n0 = (K == 2 && permille > 0) ? (int64_t)n_scans * permille / 1000
                                                        : (int64_t)n_scans / K;
  J.first[0] = 0;
  J.count[0] = (int32_t)n0;
  for (int h = 1; h < K; ++h) {  // (K >= 2 here)
    J.first[h] = (int32_t)(n0 + (int64_t)(n_scans - n0) * (h - 1) / (K - 1));
    J.count[h] = (int32_t)(n0 + (int64_t)(n_scans - n0) * h / (K - 1)) - J.first[h];
  }
  J.resp.assign((size_t)n_scans, 0.0);
  for (auto& row : J.R)
    for (LevelRun& r : row) r.reset();
  for (int h = 0; h < K; ++h) J.order[h].clear();  // (job_begin ranks each part's windows)
}

// Level 0 of part h planned and launched (the first part in growing spans:
// the device waits for it).
int job_begin(csm_ctx* c, PipeJob& J, int h) {
  const int32_t s0 = J.first[h];
  J.R[0][h].tag = h;
  if (CSM_WINDOW_ORDER) {  // here, not in job_setup: part 0's launch goes out before the other parts are ranked
    window_order(Geometry(c->info), J.poses + 3 * (size_t)s0, J.count[h], J.order[h]);
    J.R[0][h].order = J.R[1][h].order = J.order[h].data();
  }
  return with_slot(c, J, h, [&] {
    const int32_t* g = J.scan_grid ? J.scan_grid + s0 : nullptr;
    if (h == 0)
      return level_begin_split(c, J.count[h], J.offsets + s0, J.levels[0], J.poses + 3 * (size_t)s0,
                               J.resp.data() + s0, J.R[0][h], g, job_skip(c, J, 0), J.first_windows);
    return level_begin(c, J.count[h], J.offsets + s0, J.levels[0], J.poses + 3 * (size_t)s0, J.resp.data() + s0,
                       nullptr, J.R[0][h], g, job_skip(c, J, 0));
  });
}

// Every level transition of J but the last part's last one, which is left to
// job_last_handoff (J.pending): when a submitted batch returns, the device
// still has the last part's previous level and the other parts' last level
// queued, enough to cover the host's way to the next batch's first launch.
int job_levels(csm_ctx* c, PipeJob& J) {
  const int K = J.K, n_levels = J.n_levels;
  int st;
  for (int l = 0; l + 1 < n_levels; ++l)
    for (int h = 0; h < K; ++h) {
      if (handoff_deferred(l, h, K, n_levels, c->defer_last_handoff)) continue;
      if ((st = job_handoff(c, J, l, h)) != CSM_OK) return st;
    }
  job_launched(c, J);
  return CSM_OK;
}

// J's launches are out up to the deferred hand-off: its completion is owed.
void job_launched(const csm_ctx* c, PipeJob& J) {
  J.pending = true;
  J.last_handoff_done = J.n_levels < 2 || !c->defer_last_handoff;
}

// J's last level: every part's windows completed, responses summed (and the
// submitted batch's scores written).
int job_finish(csm_ctx* c, PipeJob& J) {
  if (!J.pending) return CSM_OK;
  int st;
  if ((st = job_last_handoff(c, J)) != CSM_OK) return st;
  J.pending = false;
  const int K = J.K, last = J.n_levels - 1;
  for (int h = 0; h < K; ++h) {
    const int32_t s0 = J.first[h];
    LevelRun& cur = J.R[last & 1][h];
    if (c->debug_fin) {
      J.snaps[h].assign(cur.scan_of.size(), csm::FinishOut{});
      J.hows[h].assign(cur.scan_of.size(), (char)3);
      cur.snap = &J.snaps[h];
      cur.how = &J.hows[h];
    }
    if ((st = level_end(c, cur, J.poses + 3 * (size_t)s0, J.covs + 9 * (size_t)s0, J.resp.data() + s0, nullptr)) !=
        CSM_OK)
      return st;
    for (int s = s0; s < s0 + J.count[h]; ++s) J.sum[(size_t)s] += J.resp[(size_t)s];
    if (J.level_resp)
      for (int s = s0; s < s0 + J.count[h]; ++s) J.level_resp[(size_t)last * J.n_scans + s] = J.resp[(size_t)s];
  }
  if (J.scores)
    for (int s = 0; s < J.n_scans; ++s) J.scores[s] = J.sum[(size_t)s] / J.n_levels;  // :281
  if (c->debug_fin) {  // the device idle: what the finish left against what was completed
    (void)hipDeviceSynchronize();
    for (int h = 0; h < K; ++h) {
      const LevelRun& L = J.R[last & 1][h];
      if (!L.dev || !L.fin) continue;
      for (size_t i = 0; i < J.snaps[h].size(); ++i) {
        const csm::FinishOut& a = J.snaps[h][i];
        const csm::FinishOut& b = L.fin[i];
        // the pieces the final seal names (the completed copy holds only those)
        const int lists = (int)(b.seal_tag_kind >> 34) & 3;
        bool same = a.seal_tag_kind == b.seal_tag_kind;
        for (int t = 0, n = csm::finish_n_pieces(lists); same && t < n; ++t) {
          const int pc = csm::finish_piece(t, lists);
          same = std::memcmp(reinterpret_cast<const char*>(&a) + 16 * pc, reinterpret_cast<const char*>(&b) + 16 * pc,
                             16) == 0;
        }
        if (same) continue;
        std::fprintf(stderr,
                     "csm debug_fin: part %d window %zu (scan %d) how %d: completed count %d n_pos %d n_ang %d front %d "
                     "ang0 %.17g | final count %d n_pos %d n_ang %d front %d ang0 %.17g\n",
                     h, i, J.first[h] + L.scan_of[i], (int)J.hows[h][i], a.count, a.n_pos, a.n_ang, a.front_idx,
                     a.ang_score[0], b.count, b.n_pos, b.n_ang, b.front_idx, b.ang_score[0]);
      }
    }
  }
  return CSM_OK;
}

// After a failure with a batch in flight: nothing stays pending, and nothing
// enqueued may still touch the buffers.
int pipe_abort(csm_ctx* c, int st) {
  if (c->pipe)
    for (PipeJob& J : static_cast<PipeState*>(c->pipe)->job) J.pending = false;
  (void)hipStreamSynchronize(c->stream);
  if (c->x_stream) (void)hipStreamSynchronize(c->x_stream);
  (void)hipStreamSynchronize(c->h2d);
  (void)hipStreamSynchronize(c->d2h);
  return st;
}

// A submitted batch whose last level is still pending is completed (every
// entry point but submit itself calls this first: the pending kernels read
// the loaded scans, the grid and the buffer slots).
int pipe_drain(csm_ctx* c) {
  if (!c->pipe) return CSM_OK;
  PipeState& PS = *static_cast<PipeState*>(c->pipe);
  for (PipeJob& J : PS.job)
    if (J.pending) {
      DeviceGuard g(c->device);
      PipeMode mode(c);  // its last hand-off launches as the rest of the batch did
      const int st = job_finish(c, J);
      if (st != CSM_OK) return pipe_abort(c, st);
    }
  return CSM_OK;
}

// Every launch of a pending batch made (its last part's last hand-off): the
// loaded points may change after this.
int pipe_last_launches(csm_ctx* c) {
  if (!c->pipe) return CSM_OK;
  for (PipeJob& J : static_cast<PipeState*>(c->pipe)->job)
    if (J.pending && !J.last_handoff_done) {
      PipeMode mode(c);
      const int st = job_last_handoff(c, J);
      if (st != CSM_OK) return pipe_abort(c, st);
    }
  return CSM_OK;
}

void pipe_free(csm_ctx* c) {
  delete static_cast<PipeState*>(c->pipe);
  c->pipe = nullptr;
}

// ScanMatchers::ScanMatch over a resident batch (scan_matchers.h:179-289),
// parts in flight: while the device runs one part's level, the host
// completes another part's previous level and plans its next one
// (level_end_begin). Scans are independent, so the split changes no result.
int match_levels_pipelined(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param* levels,
                           int n_levels, double* poses, double* covs, double* sum,
                           const int32_t* scan_grid, double* level_resp) {
  const int K = std::max(2, std::min(c->pipeline_parts, csm_ctx::kMaxParts));
  PipeMode mode(c);
  PipeJob& J = pipe_of(c).job[0];
  job_setup(c, J, n_scans, offsets, levels, n_levels, poses, covs, sum, scan_grid, K, 0);
  J.level_resp = level_resp;
  int st;
  for (int h = 0; h < K; ++h)
    if ((st = job_begin(c, J, h)) != CSM_OK) return pipe_abort(c, st);
  if ((st = job_levels(c, J)) != CSM_OK || (st = job_finish(c, J)) != CSM_OK) return pipe_abort(c, st);
  return CSM_OK;
}

}  // namespace csmh
