// finish_rules_check.cpp — the finish's decision rules
// (csrc/csm_finish_rules.hpp) driven serially over one window the way the fast
// finish drives them (finish_fast_body, tail::finish): max, level counts,
// selected set, ranks and ties, find_best, near-best set, ranks and ties --
// with the two cap sets (128: the fused finish, 512: the separate pass) and
// the four skip_lists values. Compared with a plain finish written here,
// std::sort by score descending and the three ordered scans (host_sort_finish
// as it was before the header, none of the header's functions in it):
//   - a window the rules do not flag gives the plain finish's FinishOut bit
//     for bit (the header, and the lists want_lists selects);
//   - a window is flagged exactly when a reason this program finds on its own
//     holds: a NaN, a selected or near-best set above the cap, two equal
//     scores in FindBest's band or at a rank <= 20 of a live list;
//   - level_of equals eight explicit comparisons, select_level a direct count.
// Stand-alone (tests/test_finish_rules.py builds and runs it, once under
// ASan + UBSan); no HIP runtime, no library.
#include "csm_finish_rules.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int in(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }  // inclusive
  double uni() { return (next() + 0.5) / 2147483648.0; }                            // (0, 1)
};

const double kInf = std::numeric_limits<double>::infinity();
const int kCov = 20;  // kMaxVarianceUsePointSize (correlate_scan_matcher.h:1033)

struct Window {
  int na = 1, ns = 1;
  double x0 = 0, y0 = 0, f = 1, tol = 1;
  std::vector<double> sc;   // na * ns * ns scores, angle-major
  std::vector<double> cs;   // per angle: cosine, sine
  int planted_rank = -1;    // the sorted position a duplicate was planted at
  int planted_near = -1;    // ... or its position within the sorted near-best set
  int n() const { return (int)sc.size(); }
};

void fail(const char* what, int trial, int cap, int skip) {
  std::printf("FAIL trial %d cap %d skip_lists %d: %s\n", trial, cap, skip, what);
  std::exit(1);
}

// ---- the plain finish: std::sort and the three ordered scans --------------
bool plain_equal(double a, double b, double tol) {  // util::DoubleEqual (util/slam_util.h:70-73)
  const double d = a - b;
  return d < 0.0 ? d >= -std::fabs(tol) : d <= std::fabs(tol);
}
struct Entry {
  double score;
  int idx;
};
struct Plain {
  csm::FinishOut o;
  std::vector<Entry> e;  // sorted
};
void plain_finish(const Window& W, Plain& P) {
  const int n = W.n(), ns = W.ns;
  auto X = [&](int idx) { return W.x0 + ((idx / ns) % ns) * W.f; };
  auto Y = [&](int idx) { return W.y0 + (idx % ns) * W.f; };
  std::vector<Entry>& e = P.e;
  e.resize((size_t)n);
  for (int i = 0; i < n; ++i) e[(size_t)i] = Entry{W.sc[(size_t)i], i};
  std::sort(e.begin(), e.end(), [](const Entry& a, const Entry& b) { return a.score > b.score; });
  csm::FinishOut& o = P.o;
  std::memset(&o, 0, sizeof(o));
  const double best = e[0].score;
  double ax = 0.0, ay = 0.0, thx = 0.0, thy = 0.0, ssum = 0.0;
  int count = 0;
  for (int i = 0; i < n; ++i) {  // FindBestCandidate (:670-710)
    const double s = e[(size_t)i].score;
    if (!plain_equal(s, best, 1e-2)) break;
    const int idx = e[(size_t)i].idx, a = idx / (ns * ns);
    ax += X(idx) * s;
    ay += Y(idx) * s;
    thx += W.cs[2 * (size_t)a] * s;
    thy += W.cs[2 * (size_t)a + 1] * s;
    ssum += s;
    count++;
  }
  o.front_idx = e[0].idx;
  o.count = count;
  o.best_score = best;
  o.thx = thx;
  o.thy = thy;
  o.ssum = ssum;
  o.best_x = count > 1 ? ax / ssum : X(e[0].idx);
  o.best_y = count > 1 ? ay / ssum : Y(e[0].idx);
  const double bound = std::min(best - 0.1, 0.5);
  for (int i = 0; i < n && o.n_pos < kCov; ++i) {  // :915-928
    if (!(e[(size_t)i].score > bound)) break;
    o.pos_idx[o.n_pos] = e[(size_t)i].idx;
    o.pos_score[o.n_pos] = e[(size_t)i].score;
    o.n_pos++;
  }
  for (int i = 0; i < n && o.n_ang < kCov; ++i) {  // :990-1003
    if (!(e[(size_t)i].score >= bound)) break;
    const int idx = e[(size_t)i].idx;
    if (plain_equal(X(idx), o.best_x, W.tol) && plain_equal(Y(idx), o.best_y, W.tol)) {
      o.ang_idx[o.n_ang] = idx;
      o.ang_score[o.n_ang] = e[(size_t)i].score;
      o.n_ang++;
    }
  }
}

// ---- the rules, driven as the fast finish drives them --------------------
enum Why { kNone, kNan, kSetCap, kTiePos, kNearCap, kTieAng };
struct Scratch {  // the compacted sets: 16-byte aligned keys, -inf padded (+4)
  std::vector<csm::ScorePair> ck_store, nk_store;
  std::vector<double> sk;
  std::vector<int> ci, si, ni;
  double* ck = nullptr;
  double* nk = nullptr;
  void size(int cap) {
    ck_store.assign((size_t)cap / 2 + 2, csm::ScorePair{0.0, 0.0});
    nk_store.assign((size_t)cap / 2 + 2, csm::ScorePair{0.0, 0.0});
    ck = reinterpret_cast<double*>(ck_store.data());
    nk = reinterpret_cast<double*>(nk_store.data());
    sk.assign((size_t)cap, 0.0);
    ci.assign((size_t)cap, 0);
    si.assign((size_t)cap, 0);
    ni.assign((size_t)cap, 0);
  }
};
struct RulesOut {
  csm::FinishOut o;
  Why why = kNone;
  bool header = false;  // find_best ran
  int level = 0, n_selected = 0;
  int cnt[csm::kFinishLevels];
};
void rules_finish(const Window& W, int cap, int skip_lists, Scratch& S, RulesOut& R) {
  using namespace csm;
  const int n = W.n();
  std::memset(&R.o, 0, sizeof(R.o));
  R.why = kNone;
  R.header = false;
  S.size(cap);
  // 1. max, NaN
  double best = -kInf;
  bool nan = false;
  for (int i = 0; i < n; ++i) {
    const double v = W.sc[(size_t)i];
    nan |= v != v;
    best = v > best ? v : best;
  }
  if (nan) {
    R.why = kNan;
    return;
  }
  const double bound = cov_bound(best);
  // level counts: 64 lanes' packed words, added across the wave
  LevelCounts lane[64], sum;
  for (int i = 0; i < n; ++i) lane[i & 63].add(level_of(W.sc[(size_t)i], best, bound));
  for (int l = 0; l < 64; ++l) {
    sum.c0 += lane[l].c0;
    sum.c1 += lane[l].c1;
  }
  for (int k = 0; k < kFinishLevels; ++k) R.cnt[k] = sum.level(k);
  // 2. the selected set
  const WantLists want = want_lists(skip_lists);
  select_level(R.cnt, want.pos, &R.level, &R.n_selected);
  const int nC = R.n_selected;
  if (nC > cap) {
    R.why = kSetCap;
    return;
  }
  int at = 0;
  for (int i = 0; i < n; ++i)
    if (level_of(W.sc[(size_t)i], best, bound) <= R.level) {
      S.ck[at] = W.sc[(size_t)i];
      S.ci[(size_t)at++] = i;
    }
  if (at != nC) fail("the compacted set is not select_level's n_selected", -1, cap, skip_lists);
  for (int t = 0; t < 4; ++t) S.ck[nC + t] = -kInf;
  bool tie = false;
  for (int t = 0; t < nC; ++t) {
    const double x = S.ck[t];
    int r, eq;
    rank_among(S.ck, nC, x, &r, &eq);
    tie |= tie_matters_positional(eq, r, in_response_band(x, best), want.pos);
    S.sk[(size_t)r] = x;
    S.si[(size_t)r] = S.ci[(size_t)t];
  }
  if (tie) {
    R.why = kTiePos;
    return;
  }
  // 3. FindBest, positional list
  const CandGrid g{W.x0, W.y0, W.f, W.ns};
  auto cos_sin = [&](int a) { return CosSin{W.cs[2 * (size_t)a], W.cs[2 * (size_t)a + 1]}; };
  double bx, by;
  find_best(S.sk.data(), S.si.data(), nC, best, g, cos_sin, &R.o, &bx, &by);
  R.header = true;
  R.o.n_pos = want.pos ? std::min(nC, kCovPoints) : 0;
  for (int t = 0; want.pos && t < std::min(nC, kCovPoints); ++t) {
    R.o.pos_idx[t] = S.si[(size_t)t];
    R.o.pos_score[t] = S.sk[(size_t)t];
  }
  if (!want.ang) return;
  // 4. near-best set, angular list
  int nN = 0;
  for (int i = 0; i < n; ++i) {
    const double s = W.sc[(size_t)i];
    if (s >= bound && near_best(g.x(i), g.y(i), bx, by, W.tol)) {
      if (nN < cap) {
        S.nk[nN] = s;
        S.ni[(size_t)nN] = i;
      }
      nN++;
    }
  }
  if (nN > cap) {
    R.why = kNearCap;
    return;
  }
  for (int t = 0; t < 4; ++t) S.nk[nN + t] = -kInf;
  tie = false;
  for (int t = 0; t < nN; ++t) {
    const double x = S.nk[t];
    int r, eq;
    rank_among(S.nk, nN, x, &r, &eq);
    tie |= tie_matters_angular(eq, r);
    if (r < kCovPoints) {
      R.o.ang_idx[r] = S.ni[(size_t)t];
      R.o.ang_score[r] = x;
    }
  }
  R.o.n_ang = std::min(nN, kCovPoints);
  if (tie) R.why = kTieAng;
}

// ---- the reasons, found independently -----------------------------------
// level by eight explicit comparisons
int level_direct(double s, double best, double bound) {
  if (!(s > bound)) return 8;
  const double d = s - best;
  if (d >= -0.01) return 0;
  if (d >= -0.02) return 1;
  if (d >= -0.04) return 2;
  if (d >= -0.08) return 3;
  if (d >= -0.16) return 4;
  if (d >= -0.32) return 5;
  if (d >= -0.64) return 6;
  return 7;
}
// scores of levels 0..k, counted directly
int count_upto(const Window& W, double best, double bound, int k) {
  static const double thr[7] = {0.01, 0.02, 0.04, 0.08, 0.16, 0.32, 0.64};
  int c = 0;
  for (double s : W.sc) c += (s > bound && (k >= 7 || s - best >= -thr[k])) ? 1 : 0;
  return c;
}
// v sorted descending: a value held twice whose first position is <= kCov and
// below `live` (the positions the finish looks at)
bool tie_at_rank(const std::vector<double>& v, int live) {
  for (size_t p = 0; p + 1 < v.size() && (int)p <= kCov && (int)p < live; ++p)
    if (v[p] == v[p + 1]) return true;
  return false;
}

struct Reasons {
  bool nan = false, set_cap = false, tie_band = false, tie_pos = false, near_cap = false, tie_ang = false;
  int level = 0, n_selected = 0;
  bool distinct = true;  // no score held twice
};
// P: the plain finish of W (not when a score is NaN)
Reasons find_reasons(const Window& W, const Plain* P, int cap, int skip_lists) {
  Reasons Q;
  for (double s : W.sc) Q.nan |= std::isnan(s);
  if (Q.nan) return Q;
  const bool want_pos = !(skip_lists & 1), want_ang = !(skip_lists & 2);
  const std::vector<Entry>& e = P->e;
  const double best = e[0].score, bound = std::min(best - 0.1, 0.5);
  for (size_t i = 0; i + 1 < e.size(); ++i) Q.distinct &= e[i].score != e[i + 1].score;
  // the selected set: the smallest level reaching 20, or all above the bound
  Q.level = want_pos ? 7 : 0;
  for (int k = 0; want_pos && k < 8; ++k)
    if (count_upto(W, best, bound, k) >= kCov) {
      Q.level = k;
      break;
    }
  Q.n_selected = count_upto(W, best, bound, Q.level);
  Q.set_cap = Q.n_selected > cap;
  std::vector<double> above;
  for (const Entry& x : e) {
    if (!(x.score > bound)) break;
    above.push_back(x.score);
  }
  for (size_t i = 0; i + 1 < e.size() && std::fabs(e[i + 1].score - best) <= 1e-2; ++i)
    Q.tie_band |= e[i].score == e[i + 1].score;
  Q.tie_pos = want_pos && tie_at_rank(above, Q.n_selected);
  if (want_ang) {
    std::vector<double> near;  // sorted, as e is
    const int ns = W.ns;
    for (const Entry& x : e) {
      if (!(x.score >= bound)) break;
      const double cx = W.x0 + ((x.idx / ns) % ns) * W.f, cy = W.y0 + (x.idx % ns) * W.f;
      if (plain_equal(cx, P->o.best_x, W.tol) && plain_equal(cy, P->o.best_y, W.tol)) near.push_back(x.score);
    }
    Q.near_cap = (int)near.size() > cap;
    Q.tie_ang = tie_at_rank(near, (int)near.size());
  }
  return Q;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
bool same_header(const csm::FinishOut& a, const csm::FinishOut& b) {
  return a.front_idx == b.front_idx && a.count == b.count && same_bits(a.best_score, b.best_score) &&
         same_bits(a.best_x, b.best_x) && same_bits(a.best_y, b.best_y) && same_bits(a.thx, b.thx) &&
         same_bits(a.thy, b.thy) && same_bits(a.ssum, b.ssum);
}

// ---- windows --------------------------------------------------------------
const int kShapes[4][2] = {{30, 13}, {11, 11}, {21, 3}, {1, 1}};  // the three sim levels, one candidate
enum Kind { kDistinct, kPlanted, kPlantedNear, kPalette, kCrowd, kNanKind, kKinds };

// distinct scores, few near the best: best * (1 - (1 - lo) * u^(1/p))-like spread
void draw_distinct(Rng& R, Window& W, double best, int p) {
  const double lo = best * 0.1;
  for (int tries = 0;; ++tries) {
    if (tries == 100) fail("no distinct scores drawn", -1, 0, 0);
    for (double& s : W.sc) {
      double u = R.uni(), t = u;
      for (int k = 1; k < p; k <<= 1) t *= t;  // u^p: most scores low
      s = lo + (best - lo) * (0.98 * t + 0.02 * R.uni());  // (the second draw keeps the low ones apart)
    }
    W.sc[(size_t)R.in(0, W.n() - 1)] = best;
    std::vector<double> v = W.sc;
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) == v.end()) return;
  }
}

Window draw(Rng& R, int trial, Kind kind) {
  Window W;
  const int* shape = kShapes[kind == kCrowd ? R.in(0, 1) : (trial % 13 == 12 ? 3 : trial % 3)];
  W.na = shape[0];
  W.ns = shape[1];
  W.sc.assign((size_t)W.na * W.ns * W.ns, 0.0);
  W.f = (W.ns == 13) ? 1.0 : (W.ns == 11 ? 0.4 : 0.2);
  W.x0 = 100.0 + 50.0 * R.uni();
  W.y0 = 80.0 + 50.0 * R.uni();
  const double tols[3] = {1.0, 2.0, 3.5};
  W.tol = W.f * tols[R.in(0, 2)];
  for (int a = 0; a < W.na; ++a) {
    const double th = -0.3 + 0.02 * a + 0.01 * R.uni();
    W.cs.push_back(std::cos(th));
    W.cs.push_back(std::sin(th));
  }
  // best below 0.6: bound = best - 0.1; above: bound = 0.5
  const double best = R.in(0, 1) ? 0.25 + 0.3 * R.uni() : 0.65 + 0.4 * R.uni();
  const int n = W.n();
  switch (kind) {
    case kDistinct:
    case kNanKind:
      draw_distinct(R, W, best, 1 << R.in(0, 4));
      if (kind == kNanKind) W.sc[(size_t)R.in(0, n - 1)] = std::nan("");
      break;
    case kPlanted: {
      draw_distinct(R, W, best, 1 << R.in(1, 4));
      std::vector<Entry> e((size_t)n);
      for (int i = 0; i < n; ++i) e[(size_t)i] = Entry{W.sc[(size_t)i], i};
      std::sort(e.begin(), e.end(), [](const Entry& a, const Entry& b) { return a.score > b.score; });
      int band = 0;  // elements in FindBest's band
      while (band < n && std::fabs(e[(size_t)band].score - e[0].score) <= 1e-2) ++band;
      const int ranks[6] = {0, 19, 20, 21, band - 2, band};  // ..., the band's last two, the first two outside it
      const int r = ranks[(trial / 5) % 6];
      if (r >= 0 && r + 1 < n) {
        // the lower of the pair takes the upper's score (rank 0: the max stays the max)
        W.sc[(size_t)e[(size_t)r + 1].idx] = e[(size_t)r].score;
        W.planted_rank = r;
      }
      break;
    }
    case kPlantedNear: {  // a duplicate inside the near-best set, at its ranks 19, 20, 21
      draw_distinct(R, W, best, 1 << R.in(0, 2));
      W.tol = W.f * 3.5;  // a near-best set of more than 20
      Plain P;
      plain_finish(W, P);
      const double bound = std::min(P.o.best_score - 0.1, 0.5);
      std::vector<Entry> near;
      for (const Entry& x : P.e) {
        if (!(x.score >= bound)) break;
        const double cx = W.x0 + ((x.idx / W.ns) % W.ns) * W.f, cy = W.y0 + (x.idx % W.ns) * W.f;
        if (plain_equal(cx, P.o.best_x, W.tol) && plain_equal(cy, P.o.best_y, W.tol)) near.push_back(x);
      }
      const int r = 19 + (trial / 20) % 3;
      if ((int)near.size() > r + 1) {
        W.sc[(size_t)near[(size_t)r + 1].idx] = near[(size_t)r].score;
        W.planted_near = r;
      }
      break;
    }
    case kPalette: {
      const int m = R.in(3, 5);
      double pal[5];
      for (int k = 0; k < m; ++k) pal[k] = best * (k == 0 ? 1.0 : R.uni());
      for (double& s : W.sc) s = pal[R.in(0, m - 1)];
      W.sc[(size_t)R.in(0, n - 1)] = best;
      break;
    }
    case kCrowd: {  // hundreds of distinct scores inside level 0
      draw_distinct(R, W, best, 16);
      const int crowd = std::min(n - 1, R.in(0, 1) ? R.in(130, 400) : R.in(520, 700));
      for (int k = 0; k < crowd; ++k) W.sc[(size_t)k * (size_t)(n / crowd)] = best - 0.009 * (k + 1) / (crowd + 1);
      W.sc[(size_t)n - 1] = best;
      break;
    }
    default:
      break;
  }
  return W;
}

struct Counts {
  long windows = 0, runs = 0, flagged = 0;
  long why[6] = {0, 0, 0, 0, 0, 0};
  long tie_band = 0, tie_rank = 0;
  long unflagged_skip[4] = {0, 0, 0, 0};
  long plant20_flagged = 0, plant21_unflagged = 0;
  long near20_flagged = 0, near21_unflagged = 0;
  long level_checks = 0, select_checks = 0;
};

void check_level_of(Rng& R, Counts& C) {
  for (int t = 0; t < 2000; ++t) {
    const double best = 0.05 + 1.1 * R.uni();
    const double bound = std::min(best - 0.1, 0.5);
    std::vector<double> pts;
    for (int k = 0; k < 7; ++k) {
      const double s = best - 0.01 * (1 << k);  // exactly at a threshold, and either side
      pts.push_back(s);
      pts.push_back(std::nextafter(s, kInf));
      pts.push_back(std::nextafter(s, -kInf));
    }
    pts.push_back(bound);
    pts.push_back(std::nextafter(bound, kInf));
    pts.push_back(std::nextafter(bound, -kInf));
    pts.push_back(best);
    pts.push_back(-kInf);
    for (int k = 0; k < 8; ++k) pts.push_back(best * R.uni());
    for (double s : pts) {
      if (csm::level_of(s, best, bound) != level_direct(s, best, bound)) {
        std::printf("FAIL level_of(%.17g, best %.17g, bound %.17g) = %d, by comparisons %d\n", s, best, bound,
                    csm::level_of(s, best, bound), level_direct(s, best, bound));
        std::exit(1);
      }
      C.level_checks++;
    }
    if (!same_bits(csm::cov_bound(best), bound)) fail("cov_bound is not std::min(best - 0.1, 0.5)", t, 0, 0);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int trials = argc > 1 ? std::atoi(argv[1]) : 400;
  Rng R{argc > 2 ? (uint64_t)std::atoll(argv[2]) * 2654435761ull + 12345 : 20261019ull};
  Counts C;
  check_level_of(R, C);
  // the mix: more than half of the windows are distinct or planted low enough to stay unflagged
  const Kind mix[20] = {kDistinct, kDistinct, kPlanted, kDistinct, kPalette,  kDistinct, kDistinct, kPlanted, kDistinct, kCrowd,
                        kDistinct, kPlantedNear, kPlanted, kDistinct, kDistinct, kNanKind,  kDistinct, kPlanted, kPlantedNear, kDistinct};
  const int caps[2] = {128, 512};
  Scratch S;
  RulesOut Ru;
  Plain P;
  for (int trial = 0; trial < trials; ++trial) {
    const Window W = draw(R, trial, mix[trial % 20]);
    bool has_nan = false;
    for (double s : W.sc) has_nan |= std::isnan(s);
    if (!has_nan) plain_finish(W, P);
    C.windows++;
    for (int cap : caps)
      for (int skip = 0; skip < 4; ++skip) {
        rules_finish(W, cap, skip, S, Ru);
        const Reasons Q = find_reasons(W, has_nan ? nullptr : &P, cap, skip);
        const csm::WantLists want = csm::want_lists(skip);
        if (want.pos != !(skip & 1) || want.ang != !(skip & 2) || want.lists != (3 & ~skip))
          fail("want_lists", trial, cap, skip);
        C.runs++;
        if (!Q.nan) {  // select_level against the direct count (whatever the window's fate)
          if (Ru.level != Q.level || Ru.n_selected != Q.n_selected) fail("select_level differs from the direct count", trial, cap, skip);
          C.select_checks++;
        }
        // flagged exactly when a reason holds, in the fast finish's order
        Why expect = kNone;
        if (Q.nan) expect = kNan;
        else if (Q.set_cap) expect = kSetCap;
        else if (Q.tie_band || Q.tie_pos) expect = kTiePos;
        else if (Q.near_cap) expect = kNearCap;
        else if (Q.tie_ang) expect = kTieAng;
        if (Ru.why != expect) {
          std::printf("rules say %d, the reasons found say %d (band %d pos %d)\n", (int)Ru.why, (int)expect, (int)Q.tie_band,
                      (int)Q.tie_pos);
          fail("a window is flagged without its reason, or not flagged with one", trial, cap, skip);
        }
        if (Ru.why != kNone && Q.distinct && !Q.nan && !Q.set_cap && !Q.near_cap)
          fail("all-distinct scores, sets within the caps, and flagged", trial, cap, skip);
        if (Ru.header && !same_header(Ru.o, P.o)) fail("FindBest header differs from the plain finish", trial, cap, skip);
        const bool rank_decides = W.planted_rank >= 0 && want.pos && !Q.tie_band && !Q.set_cap;
        const bool near_decides = W.planted_near >= 0 && want.ang && !Q.set_cap && !Q.tie_band && !Q.tie_pos && !Q.near_cap;
        if (near_decides && W.planted_near == 20 && Ru.why == kTieAng) C.near20_flagged++;
        if (near_decides && W.planted_near == 21 && Ru.why == kNone) C.near21_unflagged++;
        if (Ru.why != kNone) {
          C.flagged++;
          C.why[Ru.why]++;
          if (Ru.why == kTiePos) (Q.tie_band ? C.tie_band : C.tie_rank)++;
          if (rank_decides && W.planted_rank == 20 && Ru.why == kTiePos) C.plant20_flagged++;
          continue;
        }
        if (rank_decides && W.planted_rank == 21) C.plant21_unflagged++;
        // unflagged: the plain finish's FinishOut, bit for bit
        C.unflagged_skip[skip]++;
        const csm::FinishOut &a = Ru.o, &b = P.o;
        if (want.pos) {
          if (a.n_pos != b.n_pos) fail("n_pos", trial, cap, skip);
          for (int t = 0; t < a.n_pos; ++t)
            if (a.pos_idx[t] != b.pos_idx[t] || !same_bits(a.pos_score[t], b.pos_score[t])) fail("positional list", trial, cap, skip);
        } else if (a.n_pos != 0) {
          fail("n_pos of a skipped list", trial, cap, skip);
        }
        if (want.ang) {
          if (a.n_ang != b.n_ang) fail("n_ang", trial, cap, skip);
          for (int t = 0; t < a.n_ang; ++t)
            if (a.ang_idx[t] != b.ang_idx[t] || !same_bits(a.ang_score[t], b.ang_score[t])) fail("angular list", trial, cap, skip);
        } else if (a.n_ang != 0) {
          fail("n_ang of a skipped list", trial, cap, skip);
        }
      }
  }
  const long flagged_pct = 100 * C.flagged / C.runs;
  if (2 * C.flagged > C.runs) {
    std::printf("FAIL %ld of %ld runs flagged: the equality check is starved\n", C.flagged, C.runs);
    return 1;
  }
  std::printf("windows=%ld runs=%ld flagged=%ld flagged_pct=%ld nan=%ld set_cap=%ld tie_band=%ld tie_rank=%ld near_cap=%ld "
              "tie_ang=%ld unflagged_skip0=%ld unflagged_skip1=%ld unflagged_skip2=%ld unflagged_skip3=%ld "
              "plant20_flagged=%ld plant21_unflagged=%ld near20_flagged=%ld near21_unflagged=%ld level_checks=%ld select_checks=%ld\n",
              C.windows, C.runs, C.flagged, flagged_pct, C.why[kNan], C.why[kSetCap], C.tie_band, C.tie_rank, C.why[kNearCap],
              C.why[kTieAng], C.unflagged_skip[0], C.unflagged_skip[1], C.unflagged_skip[2], C.unflagged_skip[3],
              C.plant20_flagged, C.plant21_unflagged, C.near20_flagged, C.near21_unflagged, C.level_checks, C.select_checks);
  std::printf("finish_rules_check ok\n");
  return 0;
}
