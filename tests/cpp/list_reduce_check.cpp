// list_reduce_check.cpp — the reduced finish (csrc/csm_search_match.hpp
// reduced_finish: list_finish over R = A u B, two selections out of the
// collected set H) against list_finish over all of H, bit for bit:
// tie_matters, FinishOut, CovSums, response, pose and cov.
//
// The selection here is a plain host restatement of csm_select.hpp's
// definition: a sort of the keys of the hits passing pred, the K-th largest
// (the lowest when fewer pass), then the definition's membership test.
//
// Random windows (5 x 21^2, 3 x 33^2, 9 x 13^2; COARSE / FINE / SUPER) with
// full score arrays thresholded at T, and on each of them the planted
// variants below. A class is counted when the variant's sorted H shows it,
// not when it was asked for:
//   tie2021      equal scores at ranks 20 and 21
//   tie2122      equal scores at ranks 21 and 22 (harmless: past both lists)
//   tie_across   a run of equal scores across the K-th that makes |A| > K + 1
//   band_long    FindBest's band longer than 22
//   near_lt      a near-best set of fewer than 22
//   near_eq      ... of exactly 22
//   near_gt_tie  ... of more than 22 with equal scores at its ranks 20 and 21
//   a_below_b    a member of A that is near-best and scores below B's K-th
//   small_h      |H| < 22
//   dup_ab       A and B share a member
//   signed_zero  H holds negative scores, +0.0 and -0.0
// Stand-alone (tests/test_list_reduce_host.py builds and runs it, once under
// ASan + UBSan); no HIP runtime, no GPU. -DCSM_REDUCE_K=20 is the mutation
// that must fail (tie2021).
#include "csm_search_match.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm.h"

namespace {

using csm::PyrHit;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int in(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }
  double uni() { return (next() + 0.5) / 2147483648.0; }
};

struct Window {
  int na = 1, ns = 1, type = 0;
  double x0 = 0, y0 = 0, f = 1, mres = 0.05, sres = 0.05, ares = 0.0349;
  std::vector<double> sc;
  std::vector<csm::AngleEntry> rows;
  int n() const { return (int)sc.size(); }
  csm::FinishWindow fw() const {
    return csm::FinishWindow{csm::CandGrid{x0, y0, f, ns}, rows.data(), type, mres, sres, ares};
  }
};

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

[[noreturn]] void fail(const char* what, int trial, const char* variant) {
  std::printf("FAIL trial %d variant %s: %s\n", trial, variant, what);
  std::exit(1);
}

// ---- the selection, restated --------------------------------------------
uint64_t plain_key(double score) {
  const double s = score + 0.0;
  uint64_t u;
  std::memcpy(&u, &s, sizeof(u));
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
bool plain_equal(double a, double b, double tol) {  // util::DoubleEqual (util/slam_util.h:70-73)
  const double d = a - b;
  return d < 0.0 ? d >= -std::fabs(tol) : d <= std::fabs(tol);
}
bool plain_pred(const csm::SelectSpec& sp, const PyrHit& h) {
  if (!sp.near_on) return true;
  const int idx = (int)h.flat;
  const double x = sp.grid.x0 + ((idx / sp.grid.n_space) % sp.grid.n_space) * sp.grid.step;
  const double y = sp.grid.y0 + (idx % sp.grid.n_space) * sp.grid.step;
  return plain_equal(x, sp.bx, sp.tol) && plain_equal(y, sp.by, sp.tol);
}
int64_t plain_select(const std::vector<PyrHit>& H, const csm::SelectSpec& sp, PyrHit* out, int64_t cap,
                     uint64_t* key_k_out = nullptr) {
  std::vector<uint64_t> keys;
  for (const PyrHit& h : H)
    if (plain_pred(sp, h)) keys.push_back(plain_key(h.score));
  std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
  const uint64_t key_k = keys.empty() ? 0 : keys[std::min<size_t>(keys.size(), (size_t)sp.k) - 1];
  if (key_k_out) *key_k_out = key_k;
  int64_t n = 0;
  for (const PyrHit& h : H) {
    if (!plain_pred(sp, h)) continue;
    if (plain_key(h.score) >= key_k || (sp.band_on && plain_equal(h.score, sp.best, 1e-2))) {
      if (n < cap) out[n] = h;
      ++n;
    }
  }
  return n;
}

// ---- H of a window, its sorted view and the classes it shows --------------
struct View {
  std::vector<PyrHit> H;       // score >= T, in flat order
  std::vector<PyrHit> sorted;  // by score descending
  double best = 0, T = 0;
  int band = 0;
};

View view_of(const Window& W) {
  View V;
  V.best = W.sc[0];
  for (double s : W.sc) V.best = std::max(V.best, s);
  V.T = std::min(V.best - 0.1, 0.5);
  for (int i = 0; i < W.n(); ++i)
    if (W.sc[(size_t)i] >= V.T) V.H.push_back(PyrHit{W.sc[(size_t)i], i});
  V.sorted = V.H;
  std::stable_sort(V.sorted.begin(), V.sorted.end(), [](const PyrHit& a, const PyrHit& b) { return a.score > b.score; });
  for (const PyrHit& h : V.sorted) {
    if (!plain_equal(h.score, V.best, 1e-2)) break;
    V.band++;
  }
  return V;
}

struct Counts {
  long trials = 0, variants = 0, equal = 0, ties = 0, by_type[3] = {0, 0, 0}, overflow = 0;
  long tie2021 = 0, tie2122 = 0, tie_across = 0, band_long = 0, near_lt = 0, near_eq = 0, near_gt_tie = 0, a_below_b = 0,
       small_h = 0, dup_ab = 0, signed_zero = 0;
};

struct Seen {
  bool tie2021 = false, tie2122 = false, tie_across = false, band_long = false, near_lt = false, near_eq = false,
       near_gt_tie = false, a_below_b = false, small_h = false, dup_ab = false, signed_zero = false;
};

void shuffle(std::vector<PyrHit>& v, Rng& R) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[(size_t)R.in(0, (int)i - 1)]);
}

// One variant: list_finish(H) against reduced_finish over the same H; what it shows goes to `seen`.
void check(const Window& W, Rng& R, Counts& C, Seen& seen, int trial, const char* variant) {
  static const double cov_in[9] = {7.0, -1.0, 2.0, 3.0, 8.0, -4.0, 5.0, 6.0, 9.0};
  const View V = view_of(W);
  const csm::FinishWindow FW = W.fw();
  const int K = csm::kCovPoints + 2;
  C.variants++;

  // the reference: the whole list
  std::vector<PyrHit> whole = V.H;
  shuffle(whole, R);
  double cov_h[9];
  std::memcpy(cov_h, cov_in, sizeof(cov_h));
  csm::ListFinish LH;
  csm::list_finish(whole.data(), (int64_t)whole.size(), FW, cov_h, &LH);

  // the reduced finish over a differently shuffled H
  std::vector<PyrHit> list = V.H;
  shuffle(list, R);
  const int64_t max_sel = (int64_t)list.size() + 1;
  std::vector<PyrHit> buf((size_t)(3 * max_sel));
  auto select = [&](const csm::SelectSpec& sp, PyrHit* out, int64_t cap) { return plain_select(list, sp, out, cap); };
  double cov_r[9];
  std::memcpy(cov_r, cov_in, sizeof(cov_r));
  csm::ListFinish LR;
  int64_t n_reduced = 0;
  const csm::Reduced red = csm::reduced_finish(select, buf.data(), buf.data() + 2 * max_sel, max_sel, V.best, FW, cov_r,
                                               &LR, &n_reduced);
  if (red != csm::Reduced::kDone) fail("the reduced finish did not finish", trial, variant);
  if (n_reduced > (int64_t)list.size()) fail("R is larger than H", trial, variant);

  if (LH.tie_matters != LR.tie_matters) fail(LH.tie_matters ? "a tie that matters on H is missed on R" : "a tie matters on R only", trial, variant);
  for (int k = 0; k < 9; ++k)
    if (!same_bits(cov_h[k], cov_r[k])) fail("covariance entry", trial, variant);
  if (LH.tie_matters) {
    C.ties++;
  } else {
    const csm::FinishOut &a = LH.o, &b = LR.o;
    if (a.front_idx != b.front_idx || a.count != b.count || a.n_pos != b.n_pos || a.n_ang != b.n_ang)
      fail("FinishOut header", trial, variant);
    if (!same_bits(a.best_score, b.best_score) || !same_bits(a.best_x, b.best_x) || !same_bits(a.best_y, b.best_y) ||
        !same_bits(a.thx, b.thx) || !same_bits(a.thy, b.thy) || !same_bits(a.ssum, b.ssum))
      fail("FindBest sums", trial, variant);
    for (int i = 0; i < csm::kCovPoints; ++i)
      if (a.pos_idx[i] != b.pos_idx[i] || a.ang_idx[i] != b.ang_idx[i] || !same_bits(a.pos_score[i], b.pos_score[i]) ||
          !same_bits(a.ang_score[i], b.ang_score[i]))
        fail("covariance lists", trial, variant);
    const csm::CovSums &s = LH.sums, &t = LR.sums;
    if (!same_bits(s.pos_norm, t.pos_norm) || !same_bits(s.vxx, t.vxx) || !same_bits(s.vxy, t.vxy) ||
        !same_bits(s.vyy, t.vyy) || !same_bits(s.ang_norm, t.ang_norm) || !same_bits(s.ang_acc, t.ang_acc))
      fail("CovSums", trial, variant);
    if (!same_bits(LH.response, LR.response)) fail("response", trial, variant);
    for (int k = 0; k < 3; ++k)
      if (!same_bits(LH.pose_map[k], LR.pose_map[k])) fail("pose", trial, variant);
    C.equal++;
  }

  // a selection that outgrows its buffer is reported, never truncated into a result
  {
    double cov_o[9];
    std::memcpy(cov_o, cov_in, sizeof(cov_o));
    csm::ListFinish LO;
    const int64_t tiny = csm::kReduceK - 1;
    std::vector<PyrHit> small((size_t)(3 * tiny));
    const csm::Reduced ro =
        csm::reduced_finish(select, small.data(), small.data() + 2 * tiny, tiny, V.best, FW, cov_o, &LO);
    if ((int64_t)V.H.size() > tiny) {
      if (ro != csm::Reduced::kOverflow) fail("a selection larger than its buffer was not reported", trial, variant);
      for (int k = 0; k < 9; ++k)
        if (!same_bits(cov_o[k], cov_in[k])) fail("cov written on overflow", trial, variant);
      C.overflow++;
    }
  }

  // ---- what this variant shows ----
  const std::vector<PyrHit>& S = V.sorted;
  const size_t n = S.size();
  if (n < 22) seen.small_h = true;
  if (n >= 22 && S[20].score == S[21].score) seen.tie2021 = true;
  if (n >= 23 && S[21].score == S[22].score && S[20].score != S[21].score) seen.tie2122 = true;
  if (V.band > 22) seen.band_long = true;
  bool neg = false, pz = false, nz = false;
  for (const PyrHit& h : S) {
    if (h.score < 0.0) neg = true;
    if (h.score == 0.0) (std::signbit(h.score) ? nz : pz) = true;
  }
  if (neg && pz && nz) seen.signed_zero = true;
  // A and B as the definition gives them, around the pose the whole list's find_best gives
  csm::SelectSpec sa{};
  sa.k = K;
  sa.band_on = 1;
  sa.best = V.best;
  sa.grid = FW.grid;
  std::vector<PyrHit> A(n), B(n);
  uint64_t key_a = 0, key_b = 0;
  A.resize((size_t)plain_select(V.H, sa, A.data(), (int64_t)n, &key_a));
  if (V.band <= 22 && A.size() > (size_t)K + 1) seen.tie_across = true;
  double bx, by;
  csm::sorted_best_xy(S.data(), (int64_t)n, FW, &bx, &by);
  csm::SelectSpec sb = sa;
  sb.band_on = 0;
  sb.near_on = 1;
  sb.bx = bx;
  sb.by = by;
  sb.tol = W.sres / W.mres;
  std::vector<PyrHit> near;
  for (const PyrHit& h : S)
    if (plain_pred(sb, h)) near.push_back(h);
  if (near.size() < 22) seen.near_lt = true;
  if (near.size() == 22) seen.near_eq = true;
  if (near.size() > 22 && near[20].score == near[21].score) seen.near_gt_tie = true;
  B.resize((size_t)plain_select(V.H, sb, B.data(), (int64_t)n, &key_b));
  for (const PyrHit& a : A) {
    if (plain_pred(sb, a) && plain_key(a.score) < key_b) seen.a_below_b = true;
    for (const PyrHit& b : B)
      if (a.flat == b.flat) seen.dup_ab = true;
  }
}

Window draw(Rng& R, int trial) {
  static const int shapes[3][2] = {{5, 21}, {3, 33}, {9, 13}};
  Window W;
  W.na = shapes[trial % 3][0];
  W.ns = shapes[trial % 3][1];
  W.type = (trial / 3) % 3;
  W.x0 = 30.0 + 20.0 * R.uni();
  W.y0 = 25.0 + 20.0 * R.uni();
  W.f = 1.0;
  W.sres = W.mres * (1.0 + (trial % 4));  // the near-best tolerance: 1 .. 4 cells
  for (int a = 0; a < W.na; ++a) {
    const double th = -0.07 + W.ares * a;
    W.rows.push_back(csm::AngleEntry{th, std::cos(th), std::sin(th)});
  }
  const int n = W.na * W.ns * W.ns;
  W.sc.assign((size_t)n, 0.0);
  const double best = R.in(0, 1) ? 0.3 + 0.3 * R.uni() : 0.65 + 0.5 * R.uni();
  // a peak away from the window's rim: scores fall off with the distance from a centre, plus noise
  const int ca = R.in(0, W.na - 1), cj = R.in(3, W.ns - 4), ck = R.in(3, W.ns - 4);
  const double width = 2.0 + 6.0 * R.uni();
  for (int i = 0; i < n; ++i) {
    const int a = i / (W.ns * W.ns), j = (i / W.ns) % W.ns, k = i % W.ns;
    const double d2 = (double)((j - cj) * (j - cj) + (k - ck) * (k - ck)) / (width * width) + 0.5 * (a - ca) * (a - ca);
    W.sc[(size_t)i] = best * (0.15 + 0.8 * std::exp(-d2)) * (0.9 + 0.1 * R.uni());
  }
  W.sc[(size_t)((ca * W.ns + cj) * W.ns + ck)] = best;
  return W;
}

}  // namespace

int main(int argc, char** argv) {
  const int trials = argc > 1 ? std::atoi(argv[1]) : 180;
  Rng R{argc > 2 ? (uint64_t)std::atoll(argv[2]) * 2654435761ull + 99 : 20261020ull};
  Counts C;
  for (int trial = 0; trial < trials; ++trial) {
    const Window W = draw(R, trial);
    const View V = view_of(W);
    const std::vector<PyrHit>& S = V.sorted;
    const int n = (int)S.size();
    Seen seen;
    C.trials++;
    C.by_type[W.type]++;
    check(W, R, C, seen, trial, "plain");
    auto tie_ranks = [&](int lo, int hi, const char* name) {  // ranks lo..hi take rank lo's score
      if (n <= hi) return;
      Window X = W;
      for (int r = lo + 1; r <= hi; ++r) X.sc[(size_t)S[(size_t)r].flat] = S[(size_t)lo].score;
      check(X, R, C, seen, trial, name);
    };
    tie_ranks(20, 21, "tie2021");
    tie_ranks(21, 22, "tie2122");
    tie_ranks(21, 24, "tie_across");
    tie_ranks(19, 23, "tie_over_both");
    // a long band: the next 29 candidates just below the best, distinct
    if (n > 30) {
      Window X = W;
      for (int r = 1; r < 30; ++r) X.sc[(size_t)S[(size_t)r].flat] = V.best - 0.0003 * r - 1e-7 * R.uni();
      check(X, R, C, seen, trial, "band_long");
    }
    // |H| < 22: everything below rank m leaves H
    {
      Window X = W;
      const int m = R.in(1, 21);
      for (int r = m; r < n; ++r) X.sc[(size_t)S[(size_t)r].flat] = V.T - 0.01 - 0.001 * R.uni();
      check(X, R, C, seen, trial, "small_h");
    }
    // the near-best set shaped: the candidates within the tolerance of the pose the band gives, by score;
    // `keep` of them stay in H (raised to just above T where they were below), the rest leave it
    {
      const csm::FinishWindow FW = W.fw();
      double bx, by;
      csm::sorted_best_xy(S.data(), (int64_t)n, FW, &bx, &by);
      const double tol = W.sres / W.mres;
      std::vector<PyrHit> geo;  // outside the band, so the pose stays
      for (int i = 0; i < W.n(); ++i)
        if (plain_equal(FW.grid.x(i), bx, tol) && plain_equal(FW.grid.y(i), by, tol) && !plain_equal(W.sc[(size_t)i], V.best, 1e-2))
          geo.push_back(PyrHit{W.sc[(size_t)i], i});
      std::sort(geo.begin(), geo.end(), [](const PyrHit& a, const PyrHit& b) { return a.score > b.score; });
      int in_band_near = 0;
      for (int r = 0; r < V.band; ++r)
        if (plain_equal(FW.grid.x((int)S[(size_t)r].flat), bx, tol) && plain_equal(FW.grid.y((int)S[(size_t)r].flat), by, tol))
          ++in_band_near;
      auto shaped = [&](int keep, bool tie, const char* name) {
        const int want = keep - in_band_near;
        if (want < 2 || want > (int)geo.size()) return;
        Window X = W;
        double low = V.T + 0.02;
        for (int g = 0; g < (int)geo.size(); ++g) {
          double s = geo[(size_t)g].score;
          if (g < want) {
            if (!(s >= V.T + 0.001)) s = low -= 1e-5 * (1.0 + R.uni());
          } else {
            s = V.T - 0.01 - 0.001 * R.uni();
          }
          X.sc[(size_t)geo[(size_t)g].flat] = s;
        }
        if (tie) {  // the near-best ranks 20 and 21
          const int g = 20 - in_band_near;
          if (g < 0 || g + 1 >= want) return;
          X.sc[(size_t)geo[(size_t)g + 1].flat] = X.sc[(size_t)geo[(size_t)g].flat];
        }
        check(X, R, C, seen, trial, name);
      };
      shaped(22, false, "near_eq");
      shaped(12, false, "near_lt");
      shaped(std::min(30, (int)geo.size() + in_band_near), true, "near_gt_tie");
    }
    // a band of the 3 x 3 cells around an interior centre at every angle: more than 22 near-best band
    // members, so A holds near-best candidates below B's K-th
    {
      Window X = W;
      const int cj = R.in(3, W.ns - 4), ck = R.in(3, W.ns - 4);
      for (double& s : X.sc) s = std::min(s, V.best - 0.02 - 0.001 * R.uni());
      int r = 0;
      for (int a = 0; a < W.na; ++a)
        for (int dj = -1; dj <= 1; ++dj)
          for (int dk = -1; dk <= 1; ++dk, ++r)
            X.sc[(size_t)((a * W.ns + cj + dj) * W.ns + ck + dk)] = V.best - 0.0001 * r;
      check(X, R, C, seen, trial, "a_below_b");
    }
    // negative scores, +0.0 and -0.0: a best below 0.1 puts T below zero
    {
      Window X = W;
      for (double& s : X.sc) s = s * (0.05 / V.best) - 0.02;
      const int p = R.in(0, W.n() - 4);
      int z = 0;
      for (int i = p; z < 4 && i < W.n(); ++i)
        if (X.sc[(size_t)i] < 0.02) X.sc[(size_t)i] = (z++ & 1) ? -0.0 : 0.0;
      check(X, R, C, seen, trial, "signed_zero");
      // ... and the two zeros at ranks 20 and 21: one key, one run
      Window Y = W;
      for (double& s : Y.sc) s = s * (0.05 / V.best) - 0.02;
      std::vector<PyrHit> o;
      for (int i = 0; i < Y.n(); ++i) o.push_back(PyrHit{Y.sc[(size_t)i], i});
      std::sort(o.begin(), o.end(), [](const PyrHit& a, const PyrHit& b) { return a.score > b.score; });
      if (o.size() > 24 && o[19].score > 0.0) {
        const double shift = o[20].score;  // ranks 20, 21 to zero, the rest keeps its order
        for (double& s : Y.sc) s -= shift;
        Y.sc[(size_t)o[20].flat] = 0.0;
        Y.sc[(size_t)o[21].flat] = -0.0;
        check(Y, R, C, seen, trial, "signed_zero_2021");
      }
    }
    C.tie2021 += seen.tie2021;
    C.tie2122 += seen.tie2122;
    C.tie_across += seen.tie_across;
    C.band_long += seen.band_long;
    C.near_lt += seen.near_lt;
    C.near_eq += seen.near_eq;
    C.near_gt_tie += seen.near_gt_tie;
    C.a_below_b += seen.a_below_b;
    C.small_h += seen.small_h;
    C.dup_ab += seen.dup_ab;
    C.signed_zero += seen.signed_zero;
  }
  std::printf("trials=%ld variants=%ld equal=%ld ties=%ld overflow=%ld coarse=%ld fine=%ld super=%ld tie2021=%ld tie2122=%ld "
              "tie_across=%ld band_long=%ld near_lt=%ld near_eq=%ld near_gt_tie=%ld a_below_b=%ld small_h=%ld dup_ab=%ld "
              "signed_zero=%ld\n",
              C.trials, C.variants, C.equal, C.ties, C.overflow, C.by_type[0], C.by_type[1], C.by_type[2], C.tie2021,
              C.tie2122, C.tie_across, C.band_long, C.near_lt, C.near_eq, C.near_gt_tie, C.a_below_b, C.small_h, C.dup_ab,
              C.signed_zero);
  std::printf("list_reduce_check ok\n");
  return 0;
}
