// search_match_check.cpp — the finish over a collected list
// (csrc/csm_search_match.cpp list_finish) against a plain finish written here:
// std::sort of the window's full score array by score descending, then
// FindBestCandidate, the two covariance lists and the covariances as the
// reference computes them (correlate_scan_matcher.h:670-710, 835-869,
// 887-1019), none of the library's functions in it. list_finish gets only the
// candidates with score >= min(best - 0.1, 0.5), shuffled.
//   - distinct scores: every output bit-equal, for COARSE, FINE and SUPER;
//   - planted ties that must give "a tie matters": inside FindBest's band, at
//     ranks 19/20 of the positional list, among the near-best angular
//     candidates;
//   - planted ties that must not: far below rank 20 and outside the near-best
//     set (the outputs still equal the plain finish's);
//   - the early returns: best < 1e-6, a positional / angular norm of 1e-6, an
//     empty near-best set.
// Stand-alone (tests/test_search_match_host.py builds and runs it, once under
// ASan + UBSan); no HIP runtime, no GPU.
#include "csm_search_match.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm.h"

namespace {

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
  double X(int idx) const { return x0 + ((idx / ns) % ns) * f; }
  double Y(int idx) const { return y0 + (idx % ns) * f; }
};

bool plain_equal(double a, double b, double tol) {  // util::DoubleEqual (util/slam_util.h:70-73)
  const double d = a - b;
  return d < 0.0 ? d >= -std::fabs(tol) : d <= std::fabs(tol);
}

struct Entry {
  double score;
  int idx;
};

struct Plain {
  int front = 0, count = 0, n_pos = 0, n_ang = 0;
  double best = 0, thx = 0, thy = 0, ssum = 0, pose[3] = {0, 0, 0}, response = 0;
  double pos_norm = 0, vxx = 0, vxy = 0, vyy = 0, ang_norm = 0, ang_acc = 0;
  double cov[9];
  std::vector<Entry> e;         // sorted
  std::vector<Entry> near;      // the near-best candidates with s >= bound, sorted
  int n_above = 0;              // candidates with s > bound
};

void plain_finish(const Window& W, const double cov_in[9], Plain& P) {
  const int n = W.n();
  P = Plain{};
  std::memcpy(P.cov, cov_in, sizeof(P.cov));
  std::vector<Entry>& e = P.e;
  e.resize((size_t)n);
  for (int i = 0; i < n; ++i) e[(size_t)i] = Entry{W.sc[(size_t)i], i};
  std::sort(e.begin(), e.end(), [](const Entry& a, const Entry& b) { return a.score > b.score; });
  const double best = e[0].score;
  double ax = 0, ay = 0;
  for (int i = 0; i < n; ++i) {  // FindBestCandidate (:670-710)
    const double s = e[(size_t)i].score;
    if (!plain_equal(s, best, 1e-2)) break;
    const int idx = e[(size_t)i].idx, a = idx / (W.ns * W.ns);
    ax += W.X(idx) * s;
    ay += W.Y(idx) * s;
    P.thx += W.rows[(size_t)a].cosine * s;
    P.thy += W.rows[(size_t)a].sine * s;
    P.ssum += s;
    P.count++;
  }
  P.front = e[0].idx;
  P.best = best;
  double bx = W.X(P.front), by = W.Y(P.front), ba = W.rows[(size_t)(P.front / (W.ns * W.ns))].angle;
  if (P.count > 1) {
    bx = ax / P.ssum;
    by = ay / P.ssum;
    ba = std::atan2(P.thy / P.ssum, P.thx / P.ssum);
  }
  P.pose[0] = bx;
  P.pose[1] = by;
  P.pose[2] = ba;
  const double bound = std::min(best - 0.1, 0.5);
  const double max_ang = 4 * (W.ares * W.ares);
  const double tol = W.sres / W.mres;
  for (const Entry& x : e) {
    if (x.score > bound) P.n_above++;
    if (x.score >= bound && plain_equal(W.X(x.idx), bx, tol) && plain_equal(W.Y(x.idx), by, tol)) P.near.push_back(x);
  }
  double* cov = P.cov;
  auto positional = [&]() {  // :887-956
    for (int i = 0; i < 9; ++i) cov[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (best < 1e-6) {
      cov[0] = 500.0;
      cov[4] = 500.0;
      cov[8] = max_ang;
      return;
    }
    int counter = 0;
    for (const Entry& x : e) {
      if (!(x.score > bound && counter < 20)) break;
      const double dx = W.X(x.idx) - bx, dy = W.Y(x.idx) - by;
      P.pos_norm += x.score;
      P.vxx += (dx * dx * x.score);
      P.vxy += (dx * dy * x.score);
      P.vyy += (dy * dy * x.score);
      counter++;
    }
    P.n_pos = counter;
    if (P.pos_norm > 1e-6) {
      double xx = P.vxx / P.pos_norm, xy = P.vxy / P.pos_norm, yy = P.vyy / P.pos_norm;
      const double r = W.sres / W.mres;
      const double minv = 0.1 * (r * r);
      xx = std::max<double>(xx, minv);
      yy = std::max<double>(yy, minv);
      const double m2 = W.mres * W.mres;
      cov[0] = (xx * m2) / best;
      cov[1] = (xy * m2) / best;
      cov[3] = (xy * m2) / best;
      cov[4] = (yy * m2) / best;
      cov[8] = max_ang;
    }
    if (plain_equal(cov[0], 0.0, 1e-6)) cov[0] = 500.0;
    if (plain_equal(cov[4], 0.0, 1e-6)) cov[4] = 500.0;
  };
  auto angular = [&]() {  // :965-1019
    if (best < 1e-6) {
      cov[8] = max_ang;
      return;
    }
    int counter = 0;
    for (const Entry& x : e) {
      if (x.score >= bound && counter < 20) {
        if (plain_equal(W.X(x.idx), bx, tol) && plain_equal(W.Y(x.idx), by, tol)) {
          const double d = W.rows[(size_t)(x.idx / (W.ns * W.ns))].angle - ba;
          P.ang_norm += x.score;
          P.ang_acc += (d * d * x.score);
          counter++;
        }
      }
    }
    P.n_ang = counter;
    double v = max_ang;
    if (P.ang_norm > 1e-6) {
      if (P.ang_acc < 1e-6) v = max_ang / 4;
      v = P.ang_acc / P.ang_norm;  // :1013 overwrites the / 4 value
    } else {
      v = 200 * max_ang;
    }
    cov[8] = v;
  };
  if (W.type == CSM_COARSE) {
    positional();
    angular();
  } else if (W.type == CSM_FINE) {
    positional();
  } else if (W.type == CSM_SUPER) {
    angular();
  }
  P.response = best > 1.0 ? 1.0 : best;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

void fail(const char* what, int trial) {
  std::printf("FAIL trial %d: %s\n", trial, what);
  std::exit(1);
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
  // a peak: scores fall off with the distance from a centre, plus noise; distinct
  const int ca = R.in(0, W.na - 1), cj = R.in(0, W.ns - 1), ck = R.in(0, W.ns - 1);
  const double width = 2.0 + 6.0 * R.uni();
  for (int tries = 0;; ++tries) {
    if (tries == 50) fail("no distinct scores drawn", trial);
    for (int i = 0; i < n; ++i) {
      const int a = i / (W.ns * W.ns), j = (i / W.ns) % W.ns, k = i % W.ns;
      const double d2 = (double)((j - cj) * (j - cj) + (k - ck) * (k - ck)) / (width * width) + 0.5 * (a - ca) * (a - ca);
      W.sc[(size_t)i] = best * (0.15 + 0.8 * std::exp(-d2)) * (0.9 + 0.1 * R.uni());
    }
    W.sc[(size_t)((ca * W.ns + cj) * W.ns + ck)] = best;
    std::vector<double> v = W.sc;
    std::sort(v.begin(), v.end());
    if (std::adjacent_find(v.begin(), v.end()) == v.end()) break;
  }
  return W;
}

struct Counts {
  long windows = 0, equal = 0, by_type[3] = {0, 0, 0};
  long tie_band = 0, tie_pos19 = 0, tie_pos20 = 0, tie_ang = 0, tie_harmless = 0, tie_unread_list = 0;
  long early_best = 0, early_norm = 0, early_near_empty = 0, rank20_exercised = 0;
};

// list_finish over the candidates of W with score >= the bound, shuffled
csm::ListFinish run_list(const Window& W, Rng& R, double cov[9], long* n_list) {
  double best = W.sc[0];
  for (double s : W.sc) best = std::max(best, s);
  const double bound = std::min(best - 0.1, 0.5);
  std::vector<csm::PyrHit> hits;
  for (int i = 0; i < W.n(); ++i)
    if (W.sc[(size_t)i] >= bound) hits.push_back(csm::PyrHit{W.sc[(size_t)i], i});
  for (size_t i = hits.size(); i > 1; --i) std::swap(hits[i - 1], hits[(size_t)R.in(0, (int)i - 1)]);
  const csm::FinishWindow FW{csm::CandGrid{W.x0, W.y0, W.f, W.ns}, W.rows.data(), W.type, W.mres, W.sres, W.ares};
  csm::ListFinish LF;
  csm::list_finish(hits.data(), (int64_t)hits.size(), FW, cov, &LF);
  if (n_list) *n_list = (long)hits.size();
  return LF;
}

void expect_equal(const Window& W, const Plain& P, const csm::ListFinish& LF, const double cov[9], int trial) {
  if (LF.tie_matters) fail("a tie is said to matter where none does", trial);
  const csm::FinishOut& o = LF.o;
  if (o.front_idx != P.front) fail("front index", trial);
  if (o.count != P.count) fail("FindBest count", trial);
  if (!same_bits(o.best_score, P.best) || !same_bits(o.thx, P.thx) || !same_bits(o.thy, P.thy) ||
      !same_bits(o.ssum, P.ssum))
    fail("FindBest sums", trial);
  for (int k = 0; k < 3; ++k)
    if (!same_bits(LF.pose_map[k], P.pose[k])) fail("averaged pose", trial);
  if (!same_bits(LF.response, P.response)) fail("response", trial);
  const bool summed = !(P.best < 1e-6);  // the early return reads no list
  if (W.type != CSM_SUPER) {
    if (summed && o.n_pos != P.n_pos) fail("positional list length", trial);
    if (!same_bits(LF.sums.pos_norm, P.pos_norm) || !same_bits(LF.sums.vxx, P.vxx) ||
        !same_bits(LF.sums.vxy, P.vxy) || !same_bits(LF.sums.vyy, P.vyy))
      fail("positional sums", trial);
  }
  if (W.type != CSM_FINE) {
    if (summed && o.n_ang != P.n_ang) fail("angular list length", trial);
    if (!same_bits(LF.sums.ang_norm, P.ang_norm) || !same_bits(LF.sums.ang_acc, P.ang_acc)) fail("angular sums", trial);
  }
  for (int k = 0; k < 9; ++k)
    if (!same_bits(cov[k], P.cov[k])) fail("covariance entry", trial);
}

void expect_tie(const csm::ListFinish& LF, const double cov[9], const double cov_in[9], const char* what, int trial) {
  if (!LF.tie_matters) fail(what, trial);
  for (int k = 0; k < 9; ++k)
    if (!same_bits(cov[k], cov_in[k])) fail("cov written although a tie matters", trial);
}

}  // namespace

int main(int argc, char** argv) {
  const int trials = argc > 1 ? std::atoi(argv[1]) : 180;
  Rng R{argc > 2 ? (uint64_t)std::atoll(argv[2]) * 2654435761ull + 99 : 20261020ull};
  Counts C;
  const double cov_in[9] = {7.0, -1.0, 2.0, 3.0, 8.0, -4.0, 5.0, 6.0, 9.0};  // in/out: untouched entries must survive
  Plain P;
  for (int trial = 0; trial < trials; ++trial) {
    Window W = draw(R, trial);
    C.windows++;
    // distinct scores
    double cov[9];
    std::memcpy(cov, cov_in, sizeof(cov));
    plain_finish(W, cov_in, P);
    long n_list = 0;
    csm::ListFinish LF = run_list(W, R, cov, &n_list);
    expect_equal(W, P, LF, cov, trial);
    C.equal++;
    C.by_type[W.type]++;
    if (P.n_above > 20) C.rank20_exercised++;
    const std::vector<Entry> e = P.e;
    const std::vector<Entry> near = P.near;
    const int n_above = P.n_above, band = P.count;
    auto with_tie = [&](int idx_to, double score, auto&& check) {
      Window V = W;
      V.sc[(size_t)idx_to] = score;
      double cv[9];
      std::memcpy(cv, cov_in, sizeof(cv));
      csm::ListFinish L2 = run_list(V, R, cv, nullptr);
      check(V, L2, cv);
    };
    // a tie inside FindBest's band (every type): the band's last member repeated by the next candidate
    if (band >= 1 && band < W.n()) {
      with_tie(e[(size_t)band].idx, e[(size_t)band - 1].score, [&](const Window&, const csm::ListFinish& L2, const double* cv) {
        expect_tie(L2, cv, cov_in, "a tie inside FindBest's band does not matter", trial);
        C.tie_band++;
      });
    }
    // ties at ranks 19 and 20 of the positional list (rank 20 is the value just past it)
    for (int r : {19, 20}) {
      if (n_above > r + 1 && r >= band) {  // below the band, so the rank alone decides
        with_tie(e[(size_t)r + 1].idx, e[(size_t)r].score, [&](const Window& V, const csm::ListFinish& L2, const double* cv) {
          if (W.type != CSM_SUPER) {
            expect_tie(L2, cv, cov_in, "a tie at rank 19/20 of the positional list does not matter", trial);
            (r == 19 ? C.tie_pos19 : C.tie_pos20)++;
          } else if (!L2.tie_matters) {  // SUPER reads no positional list: unless the pair is near-best, no tie
            Plain Q;
            plain_finish(V, cov_in, Q);
            expect_equal(V, Q, L2, cv, trial);
            C.tie_unread_list++;
          }
        });
      }
    }
    // a tie among the near-best angular candidates
    if (near.size() >= 2 && W.type != CSM_FINE) {
      // (near ranks r, r + 1 <= 20; should the pair lie in FindBest's band, it matters there already)
      const size_t r = std::min<size_t>(near.size() - 2, (size_t)R.in(0, 19));
      with_tie(near[r + 1].idx, near[r].score, [&](const Window&, const csm::ListFinish& L2, const double* cv) {
        expect_tie(L2, cv, cov_in, "a tie among the near-best angular candidates does not matter", trial);
        C.tie_ang++;
      });
    }
    // a tie far below rank 20 and outside the near-best set: no verdict, the plain outputs
    {
      int p = -1;
      auto is_near = [&](int idx) {
        for (const Entry& x : near)
          if (x.idx == idx) return true;
        return false;
      };
      for (int q = std::max(25, band + 1); q + 1 < n_above; ++q)
        if (!is_near(e[(size_t)q].idx) && !is_near(e[(size_t)q + 1].idx)) {
          p = q;
          break;
        }
      if (p >= 0) {
        with_tie(e[(size_t)p + 1].idx, e[(size_t)p].score, [&](const Window& V, const csm::ListFinish& L2, const double* cv) {
          Plain Q;
          plain_finish(V, cov_in, Q);
          expect_equal(V, Q, L2, cv, trial);
          C.tie_harmless++;
        });
      }
    }
  }
  // the early returns
  for (int type = 0; type < 3; ++type) {
    for (int kind = 0; kind < 3; ++kind) {
      Window W;
      W.na = 3;
      W.ns = 5;
      W.type = type;
      W.x0 = 10.25;
      W.y0 = 20.5;
      for (int a = 0; a < W.na; ++a) {
        const double th = 0.1 + W.ares * a;
        W.rows.push_back(csm::AngleEntry{th, std::cos(th), std::sin(th)});
      }
      W.sc.assign(75, -0.5);
      if (kind == 0) {  // best < 1e-6: kMaxVariance, kMaxVariance, max_angular_variance_
        W.sc[40] = 5e-7;
      } else if (kind == 1) {  // one candidate in the lists, norm = 1e-6: not > kDoubleTolerance
        W.sc[40] = 1e-6;
      } else {  // two band members four cells apart: the averaged pose is near neither, the near-best set is empty
        W.sc[(1 * 5 + 0) * 5 + 2] = 0.8;
        W.sc[(1 * 5 + 4) * 5 + 2] = 0.7995;
      }
      double cov[9];
      std::memcpy(cov, cov_in, sizeof(cov));
      plain_finish(W, cov_in, P);
      csm::ListFinish LF = run_list(W, R, cov, nullptr);
      expect_equal(W, P, LF, cov, 1000 + 10 * type + kind);
      const double max_ang = 4 * (W.ares * W.ares);
      if (kind == 0) {
        if (type != CSM_SUPER && !(cov[0] == 500.0 && cov[4] == 500.0)) fail("best < 1e-6: kMaxVariance", type);
        if (!same_bits(cov[8], max_ang)) fail("best < 1e-6: max_angular_variance_", type);
        C.early_best++;
      } else if (kind == 1) {
        if (type != CSM_SUPER && !(cov[0] == 1.0 && cov[4] == 1.0 && cov[1] == 0.0)) fail("norm <= 1e-6: the identity stays", type);
        if (type != CSM_FINE && !same_bits(cov[8], 200 * max_ang)) fail("angular norm <= 1e-6: 200 * max", type);
        C.early_norm++;
      } else {
        if (P.near.size() != 0) fail("the near-best set was to be empty", type);
        if (type != CSM_FINE && !same_bits(cov[8], 200 * max_ang)) fail("empty near-best set: 200 * max", type);
        C.early_near_empty++;
      }
      if (type == CSM_FINE && !same_bits(cov[8], kind == 0 ? max_ang : (P.pos_norm > 1e-6 ? max_ang : 1.0)))
        fail("FINE: cov(2,2) as the positional branch leaves it", type);
    }
  }
  std::printf("windows=%ld equal=%ld coarse=%ld fine=%ld super=%ld tie_band=%ld tie_pos19=%ld tie_pos20=%ld tie_ang=%ld "
              "tie_harmless=%ld tie_unread_list=%ld early_best=%ld early_norm=%ld early_near_empty=%ld rank20_exercised=%ld\n",
              C.windows, C.equal, C.by_type[0], C.by_type[1], C.by_type[2], C.tie_band, C.tie_pos19, C.tie_pos20, C.tie_ang,
              C.tie_harmless, C.tie_unread_list, C.early_best, C.early_norm, C.early_near_empty, C.rank20_exercised);
  std::printf("search_match_check ok\n");
  return 0;
}
