// level_decision_check.cpp — the level-wide launch decision
// (csrc/csm_level_decision.hpp) over random levels of mixed scan lengths, as
// the driver reaches it: the level summed up before its first span, every
// call (each span, the two-span hand-off, the finish-only call) deciding from
// that summary. Checks that every call of a level decides what the
// one-launch level decides, that the spans tile the level, that the range
// shortcuts (corner check, hand-off bound) never pass a window the
// window-by-window check refuses; and evaluates the rule run_windows had
// before (maxima over the plans written so far, zeros elsewhere, the range of
// the call's own span) to show it disagrees on levels with short scans first.
// Then the scoring kernel's shape and stats name over every combination of
// their inputs (check_shapes).
// Stand-alone (tests/test_level_decision.py builds and runs it, once under
// ASan + UBSan); no HIP, no library.
#include "csm_level_decision.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using namespace csmh;

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int in(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }  // inclusive
  double uni(double lo, double hi) { return lo + (hi - lo) * (next() / 2147483648.0); }
};

// the reference's beam subsampling (csm_launch.cpp beam_rule), restated
void beam_rule(int n, int U, int& step, int& n_used) {
  step = n < 2 * U ? 1 : n / (U - 1);
  n_used = (n + step - 1) / step;
}

struct Level {
  int nw = 0;
  std::vector<int32_t> n_points, step, n_used;
  std::vector<double> x0, y0;  // search starts
  std::vector<uint8_t> in_range;
  double far = 12.0;
};

const int kBeams[] = {1, 64, 127, 128, 129, 511, 512, 513, 1081};
const int kU = 1081;  // every beam of scans up to 2161 points

void fail(const char* what, int trial) {
  std::printf("FAIL trial %d: %s\n", trial, what);
  std::exit(1);
}

// The rule before: the call launching [w0, w1) with the plans of [0, planned)
// written and the others zero (n_used 0, n_points 0, step 1, start 0).
LevelDecision parent_decide(const Level& L, const LevelCaps& K, const RangeEnv& E, int planned, int w0, int w1) {
  auto window_ok = [&](int i) { return i < planned ? L.in_range[(size_t)i] != 0 : E.ok(window_reach(0, 0, L.far), 0); };
  LevelDecision d;
  d.valid = true;
  d.use_int = K.int_grid;  // over the call's own span
  for (int i = w0; i < w1 && d.use_int; ++i) d.use_int = window_ok(i);
  d.box_points_ok = true;
  for (int i = 0; i < planned; ++i) d.box_points_ok = d.box_points_ok && box_points_fit(L.n_points[(size_t)i], L.step[(size_t)i]);
  d.box = d.use_int && d.box_points_ok && K.box;
  d.phase = !d.box && d.use_int && K.phase;
  d.tiny = !d.box && !d.phase && d.use_int && K.tiny;
  for (int i = 0; i < planned; ++i) d.max_n_used = std::max(d.max_n_used, L.n_used[(size_t)i]);
  bool all = K.int_grid;
  for (int i = 0; i < L.nw && all; ++i) all = window_ok(i);
  d.tail = K.tail_finish && (d.box || d.phase || d.tiny) && d.max_n_used <= kTailMaxBeams && all;
  return d;
}

// A level's calls: (w0, w1, score, windows planned when it goes out).
struct Call {
  int w0, w1, planned;
};

std::vector<Call> split_calls(int nw, int first, int growth, int trial) {
  std::vector<Call> calls;
  int w0 = 0;
  for (int64_t sz = first; w0 < nw; sz *= std::max(2, growth)) {
    const int w1 = level_span_end(nw, w0, sz);
    if (!(w1 > w0 && w1 <= nw)) fail("a span does not advance inside the level", trial);
    if (w1 < nw && nw - w1 < sz) fail("a span left less than a span behind", trial);
    calls.push_back({w0, w1, w1});
    w0 = w1;
  }
  if (w0 != nw) fail("the spans do not tile the level", trial);
  calls.push_back({0, nw, nw});  // the finish-only call
  return calls;
}

std::vector<Call> handoff_calls(int nw) {
  const int h = nw / 2;
  return {{0, h, h}, {h, nw, nw}, {0, nw, nw}};
}

// The kernel's shape and its stats name (launch_shape, score_kernel_name)
// over every combination of the caps, fixed point or not, the box offsets,
// best or all, pair usable, tiled admissible, a row sq of 0 or 2 and these
// window widths. The names are the literals tests, bench.py and tools/ match.
const int kSpace[6] = {3, 11, 13, 16, 21, 65};
const int kKt[6] = {3, 11, 13, 16, 11, 13}, kTiles[6] = {1, 1, 1, 1, 2, 5};  // ceil(ns / ceil(ns / 16)), ceil(ns / 16)
#define SIX(p, s) {p "3" s, p "11" s, p "13" s, p "16" s, p "21" s, p "65" s}
const char* const kPairNames[2][6] = {SIX("score_box_pair_kernel<", ",all>"), SIX("score_box_pair_kernel<", ",best>")};
const char* const kBoxNames[2][6] = {SIX("score_box_kernel<", ",all>"), SIX("score_box_kernel<", ",best>")};
const char* const kPhaseNames[2][6] = {SIX("score_phase_kernel<", ",all>"), SIX("score_phase_kernel<", ",best>")};
const char* const kTinyNames[2][6] = {SIX("score_tiny_kernel<", ",all>"), SIX("score_tiny_kernel<", ",best>")};
const char* const kRowsNames[2][6] = {SIX("score_rowsd_kernel<", ",2,all>"), SIX("score_rowsd_kernel<", ",2,best>")};
#undef SIX
const char* const kColsNames[2][2][6] = {  // [int][best][width]: KT, not the width
    {{"score_cols_kernel<3,f64,all>", "score_cols_kernel<11,f64,all>", "score_cols_kernel<13,f64,all>",
      "score_cols_kernel<16,f64,all>", "score_cols_kernel<11,f64,all>", "score_cols_kernel<13,f64,all>"},
     {"score_cols_kernel<3,f64,best>", "score_cols_kernel<11,f64,best>", "score_cols_kernel<13,f64,best>",
      "score_cols_kernel<16,f64,best>", "score_cols_kernel<11,f64,best>", "score_cols_kernel<13,f64,best>"}},
    {{"score_cols_kernel<3,int,all>", "score_cols_kernel<11,int,all>", "score_cols_kernel<13,int,all>",
      "score_cols_kernel<16,int,all>", "score_cols_kernel<11,int,all>", "score_cols_kernel<13,int,all>"},
     {"score_cols_kernel<3,int,best>", "score_cols_kernel<11,int,best>", "score_cols_kernel<13,int,best>",
      "score_cols_kernel<16,int,best>", "score_cols_kernel<11,int,best>", "score_cols_kernel<13,int,best>"}}};

bool same_shape(const LaunchShape& a, const LaunchShape& b) {
  return a.kernel == b.kernel && a.use_int == b.use_int && a.best == b.best && a.n_space == b.n_space &&
         a.rows_sq == b.rows_sq && a.kt == b.kt && a.ktiles == b.ktiles && a.n_cols == b.n_cols &&
         a.col_blocks == b.col_blocks && a.bps == b.bps;
}

void check_shapes(long& n_shapes, long kernels_seen[7]) {
  const int nw = 48, na = 21;
  for (int bits = 0; bits < (1 << 11); ++bits)
    for (int si = 0; si < 6; ++si) {
      const int ns = kSpace[si];
      LevelCaps K;
      K.int_grid = bits & 1, K.tail_finish = bits & 2, K.box = bits & 4, K.phase = bits & 8, K.tiny = bits & 16;
      LevelSummary S;
      S.n_windows = nw, S.max_n_used = 128, S.in_range = bits & 32, S.points_ok = bits & 64;
      ShapeFacts F;
      F.best = bits & 128, F.pair_ok = bits & 256, F.tiled_ok = bits & 512, F.rows_sq = (bits & 1024) ? 2 : 0;
      const LevelDecision d = level_decide(S, K, 0, nw);
      const LaunchShape s = launch_shape(d, na, ns, F);
      // exactly one kernel, in the precedence: pair box, box, tiled box, phase, tiny, row segments, columns
      const bool tiled = !d.box && F.best && d.use_int && d.box_points_ok && F.tiled_ok && ns > 16;
      const bool rows = !d.box && !tiled && !d.phase && !d.tiny && F.rows_sq && ns <= 64;
      const ScoreKernel want = d.box && F.pair_ok ? ScoreKernel::kBoxPair
                               : d.box            ? ScoreKernel::kBox
                               : tiled            ? ScoreKernel::kBoxTiled
                               : d.phase          ? ScoreKernel::kPhase
                               : d.tiny           ? ScoreKernel::kTiny
                               : rows             ? ScoreKernel::kRows
                                                  : ScoreKernel::kCols;
      if (s.kernel != want) fail("the shape's kernel is not the precedence's", bits);
      if (s.kernel == ScoreKernel::kBoxTiled && !F.best) fail("the tiled box outside best mode", bits);
      if ((s.rows_sq != 0) != (s.kernel == ScoreKernel::kRows)) fail("rows_sq set for another kernel than the rows'", bits);
      if (s.kt != kKt[si] || s.ktiles != kTiles[si] || s.n_space != ns) fail("the column tiling", bits);
      // blocks per window, as run_windows had it
      const int64_t n_cols = (int64_t)na * ns, col_blocks = (n_cols + 63) / 64;
      const int64_t groups = s.rows_sq ? 64 / ns : 1;
      const bool wave_per_angle = s.kernel == ScoreKernel::kBox || s.kernel == ScoreKernel::kBoxPair ||
                                  s.kernel == ScoreKernel::kPhase || s.kernel == ScoreKernel::kTiny;
      const int64_t bps = s.kernel == ScoreKernel::kBoxTiled ? (int64_t)kTiles[si] * kTiles[si] * na
                          : wave_per_angle                   ? na
                          : s.rows_sq                        ? (na + groups - 1) / groups
                                                             : col_blocks * kTiles[si];
      if (s.bps != bps || s.n_cols != n_cols || s.col_blocks != col_blocks) fail("blocks per window", bits);
      const int b = F.best ? 1 : 0;
      const char* name = s.kernel == ScoreKernel::kBoxPair    ? kPairNames[b][si]
                         : s.kernel == ScoreKernel::kBox      ? kBoxNames[b][si]
                         : s.kernel == ScoreKernel::kBoxTiled ? "score_box_kernel<16,best,tiles>"
                         : s.kernel == ScoreKernel::kPhase    ? kPhaseNames[b][si]
                         : s.kernel == ScoreKernel::kTiny     ? kTinyNames[b][si]
                         : s.kernel == ScoreKernel::kRows     ? kRowsNames[b][si]
                                                              : kColsNames[d.use_int ? 1 : 0][b][si];
      char got[48];
      score_kernel_name(s, got, sizeof(got));
      if (std::strcmp(got, name) != 0) {
        std::printf("name %s, expected %s\n", got, name);
        fail("the kernel's stats name", bits);
      }
      // every span of the level, and its finish-only call, gets the same shape
      const int spans[4][2] = {{0, 5}, {5, nw}, {nw - 1, nw}, {0, nw}};
      for (const auto& sp : spans)
        if (!same_shape(launch_shape(level_decide(S, K, sp[0], sp[1]), na, ns, F), s)) fail("a span's shape differs", bits);
      ++n_shapes;
      ++kernels_seen[(int)s.kernel];
    }
}

}  // namespace

int main(int argc, char** argv) {
  const int trials = argc > 1 ? std::atoi(argv[1]) : 600;
  Rng rng{argc > 2 ? (uint64_t)std::atoll(argv[2]) : 20261019ull};
  // a 2000 x 2000 grid's pitch, points within 700 cells, unit cells
  const RangeEnv E{700.0, 2016, 1.0, 4};
  const double limit = std::ldexp(1.0, 30) / (4.0 * E.pitch);  // reaches beyond this are out of range
  long n_calls = 0, parent_bad_levels = 0, short_first_levels = 0, short_first_parent_bad = 0, one_launch = 0;
  long bound_checked = 0;

  for (int t = 0; t < trials; ++t) {
    Level L;
    L.nw = (t % 7 == 0) ? rng.in(2, 12) : rng.in(2, 300);
    const int first = rng.in(1, 8), growth = rng.in(2, 4);
    // the mix: 0 random, 1 short (<= 128) first then anything, 2 at most 512
    // first then one long, 3 homogeneous
    const int mix = t % 4;
    const int homog = kBeams[rng.in(0, 8)];
    const int lead = std::min(L.nw - 1, first + rng.in(0, 3));  // windows before the first long one
    const int bad_range = (rng.in(0, 3) == 0) ? rng.in(0, L.nw - 1) : -1;
    const int bad_points = (rng.in(0, 7) == 0) ? rng.in(0, L.nw - 1) : -1;
    for (int i = 0; i < L.nw; ++i) {
      int n;
      if (mix == 0) n = kBeams[rng.in(0, 8)];
      else if (mix == 1) n = i < lead ? kBeams[rng.in(0, 3)] : kBeams[rng.in(0, 8)];
      else if (mix == 2) n = i < lead ? kBeams[rng.in(0, 6)] : (i == lead ? kBeams[rng.in(7, 8)] : kBeams[rng.in(0, 6)]);
      else n = homog;
      if (i == bad_points) n = (1 << 24) + rng.in(0, 9);  // over the box kernels' 24-bit offsets
      int st, nu;
      beam_rule(n, kU, st, nu);
      L.n_points.push_back(n);
      L.step.push_back(st);
      L.n_used.push_back(nu);
      double cx = rng.uni(0.0, 2000.0), cy = rng.uni(0.0, 2000.0);
      if (i == bad_range) (rng.in(0, 1) ? cx : cy) = (rng.in(0, 1) ? 1.0 : -1.0) * (limit + rng.uni(0.0, 50.0));
      L.x0.push_back(cx - 6.0);
      L.y0.push_back(cy - 6.0);
      L.in_range.push_back(E.ok(window_reach(L.x0.back(), L.y0.back(), L.far), nu) ? 1 : 0);
    }
    if (bad_range >= 0 && L.in_range[(size_t)bad_range]) fail("the far window passed the range check", t);
    LevelCaps K;
    K.int_grid = rng.in(0, 9) != 0;
    K.tail_finish = rng.in(0, 9) != 0;
    const int fam = rng.in(0, 6);
    K.box = fam <= 2;
    K.phase = fam == 3 || fam == 4;
    K.tiny = fam == 5;

    // the one-launch level: every plan written, one call
    const LevelSummary S1 = level_summary(L.n_used.data(), L.n_points.data(), L.step.data(), L.in_range.data(), L.nw);
    const LevelDecision D1 = level_decide(S1, K, 0, L.nw);
    if (!D1.valid) fail("the whole level is not a valid span", t);
    if (level_decide(S1, K, 0, L.nw + 1).valid || level_decide(S1, K, 3, 3).valid || level_decide(S1, K, -1, 1).valid)
      fail("a span outside the level passed", t);

    // the level as level_begin_split sends it: summed up before the first span
    // (counts from the scans' sizes, range from their poses)
    LevelSummary S;
    for (int i = 0; i < L.nw; ++i) level_summary_add(S, L.n_points[(size_t)i], L.step[(size_t)i], L.n_used[(size_t)i], true);
    auto start = [&](int i, double& x0, double& y0, int& nu) {
      x0 = L.x0[(size_t)i];
      y0 = L.y0[(size_t)i];
      nu = L.n_used[(size_t)i];
    };
    const bool in_range = level_in_range(L.nw, start, L.far, E);
    if (in_range != S1.in_range) fail("level_in_range differs from the window-by-window check", t);
    S.in_range = in_range;
    std::vector<Call> calls;
    if (!K.int_grid || in_range) {
      calls = split_calls(L.nw, first, growth, t);
    } else {  // a window out of range: one launch
      calls.push_back({0, L.nw, L.nw});
      ++one_launch;
    }
    bool parent_bad = false;
    bool first_short = true;  // the first span holds only scans of at most kTailMaxBeams beams
    for (int i = 0; i < calls[0].w1; ++i) first_short = first_short && L.n_used[(size_t)i] <= kTailMaxBeams;
    for (const Call& c : calls) {
      ++n_calls;
      if (level_decide(S, K, c.w0, c.w1) != D1) fail("a call of the level decides otherwise than the one-launch level", t);
      if (parent_decide(L, K, E, c.planned, c.w0, c.w1) != D1) parent_bad = true;
    }
    const bool short_first = calls.size() > 1 && first_short && S1.max_n_used > kTailMaxBeams && D1.use_int &&
                             K.tail_finish && (D1.box || D1.phase || D1.tiny);
    parent_bad_levels += parent_bad;
    short_first_levels += short_first;
    short_first_parent_bad += short_first && parent_bad;
    if (short_first) {  // the defect itself: the first span fused its finish, the finish-only call does not
      const LevelDecision a = parent_decide(L, K, E, calls[0].planned, calls[0].w0, calls[0].w1);
      const LevelDecision z = parent_decide(L, K, E, L.nw, 0, L.nw);
      if (!(a.tail && !z.tail)) fail("the rule before did not split its decision on a short-first level", t);
    }

    // the same level reached by a split hand-off: its windows are planned from
    // poses anywhere in the previous level's windows (a wider window, `pfar`)
    {
      const double pfar = 26.0 + rng.in(0, 1) * 0.4, phalf = 13.0;
      Hull X, Y;
      Level N = L;
      for (int i = 0; i < L.nw; ++i) {
        // the previous window around the previous centre; the new centre: a
        // corner, the old centre or anywhere inside, moved by a round trip's error
        const double pcx = L.x0[(size_t)i] + 6.0, pcy = L.y0[(size_t)i] + 6.0;
        const double px0 = pcx - phalf, py0 = pcy - phalf;
        X.add(px0, pcx, pfar);
        Y.add(py0, pcy, pfar);
        auto pick = [&](double p0, double pc) {
          const int k = rng.in(0, 3);
          const double v = k == 0 ? p0 : k == 1 ? p0 + pfar : k == 2 ? pc : rng.uni(p0, p0 + pfar);
          return v + rng.uni(-1e-9, 1e-9) * std::max(1.0, std::fabs(v));
        };
        N.x0[(size_t)i] = pick(px0, pcx) - 6.0;
        N.y0[(size_t)i] = pick(py0, pcy) - 6.0;
        N.in_range[(size_t)i] = E.ok(window_reach(N.x0[(size_t)i], N.y0[(size_t)i], N.far), N.n_used[(size_t)i]) ? 1 : 0;
        // per window too: the bound from this window alone covers its successor
        Hull x1, y1;
        x1.add(px0, pcx, pfar);
        y1.add(py0, pcy, pfar);
        if (!(window_reach(N.x0[(size_t)i], N.y0[(size_t)i], N.far) <= handoff_reach_bound(x1, y1, 6.0, N.far)))
          fail("a hand-off window reaches beyond its bound", t);
        ++bound_checked;
      }
      const LevelSummary T1 = level_summary(N.n_used.data(), N.n_points.data(), N.step.data(), N.in_range.data(), N.nw);
      const LevelDecision H1 = level_decide(T1, K, 0, N.nw);
      LevelSummary T = S;
      T.in_range = E.ok(handoff_reach_bound(X, Y, 6.0, N.far), T.max_n_used);
      if (T.in_range && !T1.in_range) fail("the hand-off bound passed a level with a window out of range", t);
      if (N.nw >= 2 && (!K.int_grid || T.in_range)) {
        for (const Call& c : handoff_calls(N.nw)) {
          ++n_calls;
          if (level_decide(T, K, c.w0, c.w1) != H1) fail("a hand-off call decides otherwise than the one-launch level", t);
        }
      }
    }
    // not finite: refused, never passed
    if (t == 0) {
      Hull bx, by;
      bx.add(std::nan(""), 1.0, 2.0);
      by.add(0.0, 1.0, 2.0);
      if (E.ok(handoff_reach_bound(bx, by, 6.0, 12.0), 1)) fail("a NaN hull passed", t);
      if (E.ok(handoff_reach_bound(Hull{}, Hull{}, 6.0, 12.0), 1)) fail("an empty hull passed", t);
      auto nan_start = [&](int, double& x0, double& y0, int& nu) { x0 = std::nan(""), y0 = 5.0, nu = 1; };
      if (level_in_range(3, nan_start, 12.0, E)) fail("a NaN start passed", t);
    }
  }

  // The arrangement of the GPU tests' "short first": 5 windows of 128 beams
  // in the first span, then a full scan. Before: the first span fuses its
  // finish, the later spans and the finish-only call do not.
  {
    Level L;
    L.nw = 48;
    for (int i = 0; i < L.nw; ++i) {
      const int n = i == 7 ? 1081 : 128;
      int st, nu;
      beam_rule(n, kU, st, nu);
      L.n_points.push_back(n), L.step.push_back(st), L.n_used.push_back(nu);
      L.x0.push_back(1000.0), L.y0.push_back(1000.0), L.in_range.push_back(1);
    }
    LevelCaps K;
    K.int_grid = K.tail_finish = K.box = true;
    const LevelSummary S = level_summary(L.n_used.data(), L.n_points.data(), L.step.data(), L.in_range.data(), L.nw);
    const std::vector<Call> calls = split_calls(L.nw, 5, 4, -1);
    std::printf("short_first spans:");
    for (const Call& c : calls) {
      const LevelDecision p = parent_decide(L, K, E, c.planned, c.w0, c.w1), d = level_decide(S, K, c.w0, c.w1);
      std::printf(" [%d,%d) before tail=%d max=%d now tail=%d max=%d;", c.w0, c.w1, (int)p.tail, p.max_n_used, (int)d.tail,
                  d.max_n_used);
      if (d.tail || d.max_n_used != 1081) fail("the short-first level fused its finish", -1);
    }
    std::printf("\n");
    const LevelDecision p0 = parent_decide(L, K, E, calls[0].planned, calls[0].w0, calls[0].w1);
    const LevelDecision pz = parent_decide(L, K, E, L.nw, 0, L.nw);
    std::printf("short_first before: span1_tail=%d finish_tail=%d\n", (int)p0.tail, (int)pz.tail);
  }
  long n_shapes = 0, kernels_seen[7] = {0, 0, 0, 0, 0, 0, 0}, kernels_chosen = 0;
  check_shapes(n_shapes, kernels_seen);
  for (long k : kernels_seen) kernels_chosen += k > 0;
  std::printf("levels=%d calls=%ld one_launch=%ld bounds=%ld parent_disagrees=%ld short_first=%ld short_first_parent_disagrees=%ld "
              "shapes=%ld kernels_chosen=%ld\n",
              trials, n_calls, one_launch, bound_checked, parent_bad_levels, short_first_levels, short_first_parent_bad,
              n_shapes, kernels_chosen);
  std::printf("level_decision_check ok\n");
  return 0;
}
