// csm_driver_internal.hpp — what csm_level.cpp, csm_pipeline.cpp and
// csm_driver.cpp share beyond csm_host.hpp: one level's run, a pipelined
// batch's job, and the functions one of the three calls in another.
#pragma once

#include "csm_host.hpp"

namespace csmh {

// One level (BasedCorrelationScanMatch::ScanMatch) over a batch of scans,
// split in two so a pipelined caller can overlap the host work of one half
// with the device work of the other: level_begin plans the windows and
// enqueues them (nothing waits), level_end joins and completes them.
// Points must already be uploaded; offsets index them.
struct LevelRun {
  csm_param P{};
  Dims D;
  std::vector<int> scan_of;
  std::vector<WindowPlan> plans;
  std::vector<int64_t> pt_off;
  std::vector<int32_t> grid;             // resident grid of each window (empty: grid 0)
  const AngleEntry* angles = nullptr;    // pinned buffer of the slot that ran it
  AngleEntry* rows = nullptr;            // the same, writable while the level is planned
  const csm::FinishOut* fin = nullptr;   // ditto (device finish)
  const double* scores = nullptr;        // ditto (host finish)
  bool dev = false;
  int skip_lists = 0;  // live_lists
  PendingRun pend;
  int tag = -1;        // 3-level driver: level * 8 + part (per-phase host timings)
  // CSM_DEBUG_FIN: each window's FinishOut as completed, and how (1 settled
  // early, 2 owed by the exact pass, 3 joined)
  std::vector<csm::FinishOut>* snap = nullptr;
  std::vector<char>* how = nullptr;
  // a window's FinishOut never matched its seal (pinned host memory): 1
  mutable int err = 0;
  // the order its windows take the scans in (nullptr: scan order; the
  // 3-level driver's spatial order, window_order)
  const int32_t* order = nullptr;
  // the plan pass fills each window's ScanWork into the slot's pinned staging
  // at the launch's score stride (run_windows then skips its serial fill, ~15
  // us a 2048-window launch) and checks its fixed-point range (int_bad: some
  // window is out of range; int_known: every window has been planned)
  ScanWork* sw = nullptr;
  int64_t sw_stride = 0;
  int int_bad = 0;
  bool int_known = false;
  // The level summed up for its launches (csm_level_decision.hpp): beam and
  // point counts from level_prepare (they follow from the scans' sizes alone),
  // the fixed-point range from the plan pass once every window is planned
  // (int_known), or before any is when the level goes out in spans
  // (range_preset: level_range_from_poses, handoff_in_range). Every call of
  // the level carries it (WinSpan::level), so all decide alike.
  LevelSummary shape;
  bool range_preset = false;
  // the rows' cos/sin are left to the launch (csm_trig.hip): a device finish
  // (the host finish reads them), not the few-window path (its own copy)
  bool dev_trig = false;
  // some window has an angle outside the restated sincos's domain: its launch
  // copies the host's rows (the kernel fills the others in place)
  int trig_bad = 0;
  // back to a fresh run, the vectors' capacity kept
  void reset() {
    P = csm_param{};
    D = Dims{};
    scan_of.clear();
    // (plans keep their elements: level_alloc value-initialises them only for
    // a level launched in spans, whose unplanned windows the launch reads)
    pt_off.clear();
    grid.clear();
    angles = nullptr;
    rows = nullptr;
    fin = nullptr;
    scores = nullptr;
    dev = false;
    skip_lists = 0;
    pend = PendingRun{};
    tag = -1;
    snap = nullptr;
    how = nullptr;
    err = 0;
    order = nullptr;
    sw = nullptr;
    sw_stride = 0;
    int_bad = 0;
    int_known = false;
    shape = LevelSummary{};
    range_preset = false;
    dev_trig = false;
    trig_bad = 0;
  }
};

// One batch through the 3-level driver (match_levels_pipelined). With
// csm_scan_matchers_submit the batch's last level is launched but its
// completion deferred: the next submitted batch's first launch goes out first
// (into the other half of the buffer slots), then the deferred completion runs
// while that one scores -- the device no longer idles between batches.
struct PipeJob {
  int K = 2, n_levels = 0, slot0 = 0;  // parts (1: submitted batches only), levels, the parts' first buffer slot
  int first_windows = 0;                // the first part's first span (level_begin_split)
  int32_t n_scans = 0;
  // A submitted batch's are its ScanBatch::scan_off's data: the batch parks in
  // a staging slot while the job's last hand-off is pending, and these stay
  // valid because batches are swapped, never assigned across, until the next
  // batch is queued into that slot, after the job is complete
  // (tests/cpp/resources_check.cpp, submit_sequence).
  const int64_t* offsets = nullptr;
  const int32_t* scan_grid = nullptr;
  csm_param levels[3]{};
  double *poses = nullptr, *covs = nullptr, *sum = nullptr;
  double* scores = nullptr;  // submitted: scores[s] = sum[s] / n_levels when complete
  std::vector<double> resp, own_sum;
  double* level_resp = nullptr;  // nullable: level l's responses to level_resp[l * n_scans + s] (matchers_loaded_locked)
  int32_t first[csm_ctx::kMaxParts]{}, count[csm_ctx::kMaxParts]{};
  // by level parity: level l's run and level l + 1's, per part. Reused across
  // batches: a fresh run's window plans (64 B each, 128 KB per 2048 windows)
  // came from mmap and paid ~40 us of page faults at every level start (r04).
  LevelRun R[2][csm_ctx::kMaxParts];
  bool pending = false;  // levels launched up to the last part's last hand-off; that and the completion deferred
  bool last_handoff_done = false;
  std::vector<int32_t> order[csm_ctx::kMaxParts];  // each part's scans in window order (window_order)
  std::vector<csm::FinishOut> snaps[csm_ctx::kMaxParts];  // CSM_DEBUG_FIN
  std::vector<char> hows[csm_ctx::kMaxParts];
};

struct PipeState {
  PipeJob job[2];
  int next = 0;  // the job slot the next submit takes (its parts: buffer slots next * kParts ...)
  // buffer slots of a job slot: one- and two-part batches alternate in one
  // context, so a job's slots do not depend on its own parts
  static constexpr int kParts = csm_ctx::kMaxParts / 2;
};

// The driver's knobs for a pipelined batch: every part on the throughput
// kernels (parts in flight share no few-window buffers), early completion on.
struct PipeMode {
  csm_ctx* c;
  bool small_was;
  explicit PipeMode(csm_ctx* cc) : c(cc), small_was(cc->small_path) {
    c->small_path = false;
    c->early_now = true;
  }
  ~PipeMode() {
    c->small_path = small_was;
    c->early_now = false;
  }
};

// The coarse level sums enough beams for the device to bound the step: a
// submitted batch then sends its first span out early and may take one part
// (csm_submit_order.hpp); below that the step is host-bound (csm_host.hpp).
inline bool coarse_device_bound(const csm_ctx* c, const csm_param* levels, int n_levels) {
  return n_levels > 0 && levels[0].use_point_size > c->first_windows_submit_min_use;
}

// csm_level.cpp
int live_lists(const csm_param* levels, int n_levels, int l);
int level_begin(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P, const double* poses,
                double* responses, int64_t* argmax_flat, LevelRun& R, const int32_t* scan_grid, int skip_lists);
int level_begin_split(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param& P, const double* poses,
                      double* responses, LevelRun& R, const int32_t* scan_grid, int skip_lists, int first);
int level_end(csm_ctx* c, LevelRun& R, double* poses, double* covs, double* responses, int64_t* argmax_flat);
int level_end_begin(csm_ctx* c, LevelRun& R, LevelRun& N, int32_t n_scans, const int64_t* offsets,
                    const csm_param& P, double* poses, double* covs, double* responses, double* sum,
                    const int32_t* scan_grid, int skip_lists, bool split = false);

// csm_pipeline.cpp
PipeState& pipe_of(csm_ctx* c);
void job_setup(csm_ctx* c, PipeJob& J, int32_t n_scans, const int64_t* offsets, const csm_param* levels,
               int n_levels, double* poses, double* covs, double* sum, const int32_t* scan_grid, int K, int slot0,
               bool submitted = false);
int job_begin(csm_ctx* c, PipeJob& J, int h);
int job_handoff(csm_ctx* c, PipeJob& J, int l, int h);
int job_levels(csm_ctx* c, PipeJob& J);
void job_launched(const csm_ctx* c, PipeJob& J);
int job_finish(csm_ctx* c, PipeJob& J);
int pipe_abort(csm_ctx* c, int st);
int pipe_last_launches(csm_ctx* c);
int match_levels_pipelined(csm_ctx* c, int32_t n_scans, const int64_t* offsets, const csm_param* levels,
                           int n_levels, double* poses, double* covs, double* sum,
                           const int32_t* scan_grid = nullptr, double* level_resp = nullptr);

}  // namespace csmh
