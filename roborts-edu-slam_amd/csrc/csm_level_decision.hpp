// csm_level_decision.hpp — what a level's launches decide from its windows,
// as pure host arithmetic (no HIP, no context): the fixed-point range of a
// window, the level-wide summary of its beam and point counts, the kernel
// family and the fused finish chosen from that summary, the scoring kernel's
// shape and stats name that follow from the decision, the spans a level
// goes out in, and the bound on the next level's windows a split hand-off
// plans before their poses exist. run_windows, level_begin_split and
// level_end_begin call these; tests/test_level_decision.py compiles them into
// a stand-alone program.
//
// A level launched in spans (several scoring calls and a finish-only call)
// must reach ONE decision: the fused finish counts every window of the level
// in level_ctr and lists each for the exact pass once, so a span that
// finishes its windows inside the scoring kernel while a later call runs the
// separate fast pass over all of them finishes and lists the first span's
// windows twice and leaves the counters part-counted. The summary is
// therefore made from the whole level before its first span goes out, and
// every call decides from it; the span being launched changes nothing.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace csmh {

#ifndef CSM_TAIL_MAX_BEAMS
#define CSM_TAIL_MAX_BEAMS 512
#endif
// levels summing more beams in some window keep the separate fast pass
constexpr int kTailMaxBeams = CSM_TAIL_MAX_BEAMS;
// the box kernels' beam offsets are 24-bit products (BoxWave::point: the
// point index and step * 16 each under 2^24)
constexpr int64_t kBoxOffsetLimit = (int64_t)1 << 24;

// The farthest a window's search start or end lies from the map's origin, in
// cells: the window starts at (x0, y0) and reaches `far` cells.
inline double window_reach(double x0, double y0, double far) {
  return std::max(std::max(std::fabs(x0), std::fabs(x0 + far)), std::max(std::fabs(y0), std::fabs(y0 + far)));
}

// Exact fixed-point accumulation for a window of that reach summing n_used
// beams: no offset wrap (every endpoint within 2^30 bytes of a row), and the
// sum of n_used cells exact in fp64. Monotone: a window of smaller reach and
// fewer beams passes wherever a larger one does (NaN never passes).
inline bool fixed_point_range_ok(double reach, double pts_maxabs, int32_t pitch, int n_used, double int_max_abs,
                                 int int_exp) {
  const double R = pts_maxabs * (1.0 + 1e-9) + reach + 2.0;
  if (!(R * 4.0 * (double)pitch < std::ldexp(1.0, 30))) return false;
  return !((double)n_used * int_max_abs * std::ldexp(1.0, int_exp) > std::ldexp(1.0, 53));
}

// The fixed-point range of a grid and a batch of points, as the check reads it.
struct RangeEnv {
  double pts_maxabs = 0.0;  // max |x| + |y| of the resident points
  int32_t pitch = 0;        // gridi row pitch (cells)
  double int_max_abs = 0.0;
  int int_exp = 0;
  bool ok(double reach, int n_used) const {
    return fixed_point_range_ok(reach, pts_maxabs, pitch, n_used, int_max_abs, int_exp);
  }
};

// Every one of nw windows in range, from their search starts alone (before
// any is planned). start(i, x0, y0, n_used) gives window i's; all reach `far`.
// The two extreme corners at the most beams are tried first: the check is
// monotone in the reach and the beams, and every window's reach is at most
// the larger of the corners', so when both pass every window does; otherwise
// window by window.
template <class Start>
bool level_in_range(int nw, Start&& start, double far, const RangeEnv& E) {
  double lx = INFINITY, hx = -INFINITY, ly = INFINITY, hy = -INFINITY;
  int most = 0;
  bool finite = true;
  for (int i = 0; i < nw; ++i) {
    double x0, y0;
    int n_used;
    start(i, x0, y0, n_used);
    finite = finite && std::isfinite(x0) && std::isfinite(y0);
    lx = std::min(lx, x0);
    hx = std::max(hx, x0);
    ly = std::min(ly, y0);
    hy = std::max(hy, y0);
    most = std::max(most, n_used);
  }
  if (nw == 0) return true;
  if (finite && E.ok(window_reach(lx, ly, far), most) && E.ok(window_reach(hx, hy, far), most)) return true;
  for (int i = 0; i < nw; ++i) {
    double x0, y0;
    int n_used;
    start(i, x0, y0, n_used);
    if (!E.ok(window_reach(x0, y0, far), n_used)) return false;
  }
  return true;
}

// A level's windows, summed up once.
struct LevelSummary {
  int32_t n_windows = 0;
  int32_t max_n_used = 0;  // the most beams a window sums
  bool points_ok = true;   // every window's beam offsets fit the box kernels
  bool in_range = true;    // every window passes fixed_point_range_ok
};

inline bool box_points_fit(int n_points, int step) {
  return (int64_t)n_points < kBoxOffsetLimit && (int64_t)step * 16 < kBoxOffsetLimit;
}

inline void level_summary_add(LevelSummary& S, int n_points, int step, int n_used, bool in_range) {
  S.n_windows++;
  S.max_n_used = std::max(S.max_n_used, (int32_t)n_used);
  S.points_ok = S.points_ok && box_points_fit(n_points, step);
  S.in_range = S.in_range && in_range;
}

inline LevelSummary level_summary(const int32_t* n_used, const int32_t* n_points, const int32_t* step,
                                  const uint8_t* in_range, int nw) {
  LevelSummary S;
  for (int i = 0; i < nw; ++i) level_summary_add(S, n_points[i], step[i], n_used[i], in_range[i] != 0);
  return S;
}

// What does not depend on the windows: the grid (fixed-point copy present),
// the build and the finish mode (a signalled device finish that may be fused),
// and which kernel families the level's window shape and step admit.
struct LevelCaps {
  bool int_grid = false;
  bool tail_finish = false;
  bool box = false, phase = false, tiny = false;
};

struct LevelDecision {
  bool valid = false;  // the span lies inside the level
  bool use_int = false;
  bool box_points_ok = false;
  bool box = false, phase = false, tiny = false;
  bool tail = false;       // the scoring launches finish their windows themselves (csm_tail.hpp)
  int32_t max_n_used = 0;  // the kernels' short forms (LevelWork::max_n_used): level-wide
};

inline bool operator==(const LevelDecision& a, const LevelDecision& b) {
  return a.valid == b.valid && a.use_int == b.use_int && a.box_points_ok == b.box_points_ok && a.box == b.box &&
         a.phase == b.phase && a.tiny == b.tiny && a.tail == b.tail && a.max_n_used == b.max_n_used;
}
inline bool operator!=(const LevelDecision& a, const LevelDecision& b) { return !(a == b); }

// The decision of the call that launches windows [w0, w1) of the level (the
// finish-only call: every window). Made from the level's summary alone, so it
// is the one-launch level's in every call.
inline LevelDecision level_decide(const LevelSummary& S, const LevelCaps& K, int w0, int w1) {
  LevelDecision d;
  d.valid = 0 <= w0 && w0 < w1 && w1 <= S.n_windows;
  d.use_int = K.int_grid && S.in_range;
  d.box_points_ok = S.points_ok;
  d.box = d.use_int && d.box_points_ok && K.box;
  d.phase = !d.box && d.use_int && K.phase;
  d.tiny = !d.box && !d.phase && d.use_int && K.tiny;
  d.max_n_used = S.max_n_used;
  d.tail = K.tail_finish && (d.box || d.phase || d.tiny) && S.max_n_used <= kTailMaxBeams && d.use_int;
  return d;
}

// Which scoring kernel a level's launches run, and in what shape: one value,
// made once per call from the level's decision, so the stats name, the launch
// and the finish cannot disagree. In the order of precedence, last first.
enum class ScoreKernel { kCols, kRows, kBox, kBoxPair, kBoxTiled, kPhase, kTiny };

// What the choice needs from the context and the device code, as plain values.
struct ShapeFacts {
  int rows_sq = 0;        // the row-segment kernel's instantiation for this window and step (0: none)
  bool pair_ok = false;   // the grid's palette and its strip copies are usable (v11)
  bool tiled_ok = false;  // the box over 16 x 16 tiles is admissible: whole-cell step, padded grid, block count
  bool best = false;      // best-only mode (the argmax per window, no scores)
};

struct LaunchShape {
  ScoreKernel kernel = ScoreKernel::kCols;
  bool use_int = false, best = false;
  int n_space = 0;
  int rows_sq = 0;         // nonzero only for kRows
  // 16-wide tiles per window edge (the tiled box's; the v2 column kernel's,
  // with KT rows per lane, balanced so at most a few rows idle)
  int ktiles = 0, kt = 0;
  int64_t n_cols = 0, col_blocks = 0;
  int64_t bps = 0;  // blocks per window
};

// Precedence: pair box, box, tiled box, phase, tiny, row segments, columns.
// The tiled box (v6 over 16 x 16 tiles: the argmax of a one-cell-step window
// wider than 16, loop-closure windows, in place of the column kernel's dword
// gathers) only in best mode and only when the box is not taken; row segments
// only when none of the five before them is. The same for every span of a level.
inline LaunchShape launch_shape(const LevelDecision& d, int n_angles, int n_space, const ShapeFacts& F) {
  LaunchShape s;
  s.use_int = d.use_int;
  s.best = F.best;
  s.n_space = n_space;
  s.ktiles = (n_space + 15) / 16;
  s.kt = (n_space + s.ktiles - 1) / s.ktiles;
  s.n_cols = (int64_t)n_angles * n_space;
  s.col_blocks = (s.n_cols + 63) / 64;
  const bool tiled = !d.box && F.best && d.use_int && d.box_points_ok && F.tiled_ok && n_space > 16;
  s.kernel = d.box ? (F.pair_ok ? ScoreKernel::kBoxPair : ScoreKernel::kBox)
             : tiled ? ScoreKernel::kBoxTiled
             : d.phase ? ScoreKernel::kPhase
             : d.tiny ? ScoreKernel::kTiny
             : F.rows_sq && n_space <= 64 ? ScoreKernel::kRows
                         : ScoreKernel::kCols;
  s.rows_sq = s.kernel == ScoreKernel::kRows ? F.rows_sq : 0;
  const int64_t rows_groups = s.rows_sq ? 64 / n_space : 1;
  s.bps = s.kernel == ScoreKernel::kBoxTiled ? (int64_t)s.ktiles * s.ktiles * n_angles
          : s.kernel == ScoreKernel::kRows   ? (n_angles + rows_groups - 1) / rows_groups
          : s.kernel == ScoreKernel::kCols   ? s.col_blocks * s.ktiles
                                             : n_angles;
  return s;
}

// The launch's name in the kernel stats (tests, bench.py and tools/ match on these).
inline void score_kernel_name(const LaunchShape& s, char* out, size_t n) {
  const char* m = s.best ? "best" : "all";
  switch (s.kernel) {
    case ScoreKernel::kBoxPair: std::snprintf(out, n, "score_box_pair_kernel<%d,%s>", s.n_space, m); break;
    case ScoreKernel::kBox: std::snprintf(out, n, "score_box_kernel<%d,%s>", s.n_space, m); break;
    case ScoreKernel::kBoxTiled: std::snprintf(out, n, "score_box_kernel<16,best,tiles>"); break;
    case ScoreKernel::kPhase: std::snprintf(out, n, "score_phase_kernel<%d,%s>", s.n_space, m); break;
    case ScoreKernel::kTiny: std::snprintf(out, n, "score_tiny_kernel<%d,%s>", s.n_space, m); break;
    case ScoreKernel::kRows: std::snprintf(out, n, "score_rowsd_kernel<%d,%d,%s>", s.n_space, s.rows_sq, m); break;
    case ScoreKernel::kCols: std::snprintf(out, n, "score_cols_kernel<%d,%s,%s>", s.kt, s.use_int ? "int" : "f64", m); break;
  }
}

// level_begin_split's spans: the span that starts at w0 with nominal size sz
// ends here (the last span takes the rest when it would leave less than a
// span behind). The caller multiplies sz by the growth after each span.
inline int level_span_end(int nw, int w0, int64_t sz) { return (nw - w0 <= 2 * sz) ? nw : w0 + (int)sz; }

// The split hand-off plans the next level's first span before the windows of
// its second span have poses. A scan's next centre is its completed pose: its
// previous centre (response under the threshold), a candidate of the previous
// window, or a weighted mean of candidates — inside the previous window's
// extent [p0, p0 + pfar] joined with its centre (one axis; Hull::add, over
// one window or over all of a level's), plus one cell for the
// map -> world -> map round trip. The next window starts `half` cells before
// its centre and reaches `far`. handoff_reach_bound returns a reach
// (window_reach) no window planned from such a pose exceeds; NaN, which
// fixed_point_range_ok refuses, when a previous window was not finite.
struct Hull {
  double lo = INFINITY, hi = -INFINITY;
  bool finite = true;
  void add(double p0, double pc, double pfar) {
    const double a = std::min(p0, pc), b = std::max(p0 + pfar, pc);
    finite = finite && std::isfinite(p0) && std::isfinite(pc) && std::isfinite(pfar);
    lo = std::min(lo, a);
    hi = std::max(hi, b);
  }
};

inline double handoff_reach_bound(const Hull& X, const Hull& Y, double half, double far) {
  if (!(X.finite && Y.finite && X.lo <= X.hi && Y.lo <= Y.hi)) return std::nan("");
  const double lx = X.lo - 1.0 - half, hx = X.hi + 1.0 - half + far;
  const double ly = Y.lo - 1.0 - half, hy = Y.hi + 1.0 - half + far;
  return std::max(std::max(std::fabs(lx), std::fabs(hx)), std::max(std::fabs(ly), std::fabs(hy)));
}

}  // namespace csmh
