// deskew_check — csrc/csm_deskew_host.hpp (the host arithmetic behind
// csm_deskew_plan and csm_deskew_ranges) compiled alone, for
// tests/test_deskew_host.py's plain and ASan + UBSan runs. It reads the cases
// the test wrote (the ones it also gives the library and the Python
// restatement), de-skews each into a heap block of exactly n_scans * n_beams
// floats and writes the results for the test to compare bit for bit; every
// input lives in a heap block of exactly its size, so a read or write past a
// scan, the plan or the poses is reported. Then the plan's loop and the
// refusals, on blocks of exactly the capacity given.
//
// File format (native endianness): int32 n_cases, then per case csm_laser,
// int32 n_scans, int32 n_seg, float ranges[n_scans * n_beams], int64
// seg_offsets[n_scans + 1], int32 seg_close[n_seg], double poses[(n_seg +
// n_scans) * 3]. Output: the de-skewed ranges of every case, back to back.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "csm_deskew_host.hpp"

namespace {

int fails = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);  \
      ++fails;                                                    \
    }                                                             \
  } while (0)

template <class T>
bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

void check_plan(int32_t n, double start, double end, double T) {
  int32_t need = -1;
  CHECK(csm::deskew::plan(n, start, end, T, nullptr, nullptr, 0, &need) == (need == 0 ? CSM_OK : CSM_ERR_INVALID_ARG));
  CHECK(need >= 0 && need <= n - 1);
  if (!(start < end)) CHECK(need == 0);
  if (need == 0) return;
  std::vector<int32_t> close((size_t)need);  // exactly as many as needed
  std::vector<double> sec((size_t)need);
  int32_t k = -1;
  CHECK(csm::deskew::plan(n, start, end, T, close.data(), sec.data(), need, &k) == CSM_OK && k == need);
  CHECK(close.back() == n - 1 && close.front() >= 1);
  for (int32_t i = 1; i < k; ++i) CHECK(close[(size_t)i] > close[(size_t)i - 1] && sec[(size_t)i] >= sec[(size_t)i - 1]);
  if (T == 0.0 && (end - start) * 1e6 / n > 1e-3) CHECK(k == n - 1);  // every beam from 1 on closes
  if (need > 1) {  // one short: refused, nothing past the block
    std::vector<int32_t> c2((size_t)need - 1);
    std::vector<double> s2((size_t)need - 1);
    CHECK(csm::deskew::plan(n, start, end, T, c2.data(), s2.data(), need - 1, &k) == CSM_ERR_INVALID_ARG && k == need);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: deskew_check CASES OUT\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int32_t n_cases = 0;
  if (std::fread(&n_cases, sizeof(n_cases), 1, f) != 1) return 2;
  int64_t scans_done = 0;
  for (int32_t c = 0; c < n_cases; ++c) {
    csm_laser L;
    int32_t n_scans = 0, n_seg = 0;
    if (std::fread(&L, sizeof(L), 1, f) != 1 || std::fread(&n_scans, 4, 1, f) != 1 || std::fread(&n_seg, 4, 1, f) != 1)
      return 2;
    std::vector<float> ranges;
    std::vector<int64_t> off;
    std::vector<int32_t> close;
    std::vector<double> poses;
    if (!read_n(f, ranges, (size_t)n_scans * L.n_beams) || !read_n(f, off, (size_t)n_scans + 1) ||
        !read_n(f, close, (size_t)n_seg) || !read_n(f, poses, ((size_t)n_seg + n_scans) * 3))
      return 2;
    CHECK(csm::deskew::plan_valid(L, n_scans, off.data(), close.data(), poses.data()));
    std::vector<double> cs((size_t)L.n_beams * 2);
    csm::deskew::beam_trig_table(L, cs.data());
    std::vector<float> out((size_t)n_scans * L.n_beams, -7.0f);
    csm::deskew::deskew_scans(L, cs.data(), 0, n_scans, ranges.data(), off.data(), close.data(), poses.data(),
                              out.data());
    // each interior closing beam alone (the device path's host share) against the whole scan's bins:
    // the last writer of its bin is a beam at or after it
    for (int32_t s = 0; s < n_scans; ++s) {
      const int64_t k0 = off[(size_t)s], K = off[(size_t)s + 1] - k0;
      if (K == 0) continue;
      const double* P = poses.data() + (k0 + s) * 3;
      const csm::deskew::T2 base = csm::deskew::base_transform(P[0], P[1], -P[2]);
      for (int32_t k = 0; k + 1 < K; ++k) {
        int32_t bin = -5;
        float r = -1.0f;
        csm::deskew::closing_beam(L, cs.data(), ranges.data() + (size_t)s * L.n_beams, k, close.data() + k0, P, base,
                                  &bin, &r);
        CHECK(bin >= -1 && bin < L.n_beams && r >= 0.0f);
      }
    }
    // in place gives the same
    std::vector<float> inplace(ranges);
    csm::deskew::deskew_scans(L, cs.data(), 0, n_scans, inplace.data(), off.data(), close.data(), poses.data(),
                              inplace.data());
    CHECK(std::memcmp(inplace.data(), out.data(), out.size() * sizeof(float)) == 0);
    if (!out.empty() && std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size()) return 2;
    scans_done += n_scans;
  }
  std::fclose(f);
  std::fclose(o);

  const double stamps[] = {0.0, 12.5, 1.7e9 + 0.123456789, 1.7e9 + 77.000000321};
  const int beams[] = {2, 3, 64, 65, 257, 1081};
  int plans = 0;
  for (double st : stamps)
    for (int n : beams)
      for (double T : {0.0, 0.005, 0.0049999, 1.0}) {
        check_plan(n, st, st + 0.025, T);
        check_plan(n, st, st + n * 2.3e-5, T);
        check_plan(n, st, st, T);          // start == end: no segments
        check_plan(n, st + 1.0, st, T);    // start > end
        plans += 4;
      }
  // refusals
  int32_t k = 0;
  int32_t c1[4];
  double s1[4];
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  CHECK(csm::deskew::plan(1, 0.0, 1.0, 0.005, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(0, 0.0, 1.0, 0.005, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, nan, 1.0, 0.005, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, 0.0, inf, 0.005, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, 0.0, 1.0, -0.005, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, 0.0, 1.0, nan, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, 0.0, 1.0, 3000.0, c1, s1, 4, &k) == CSM_ERR_INVALID_ARG);  // T * 1e6 past int
  CHECK(csm::deskew::plan(8, 0.0, 1.0, 0.005, c1, s1, 4, nullptr) == CSM_ERR_INVALID_ARG);
  CHECK(csm::deskew::plan(8, 0.0, 1.0, 0.005, nullptr, s1, 4, &k) == CSM_ERR_INVALID_ARG);
  csm_laser L{};
  L.angle_min = -1.0f, L.angle_increment = 0.25f, L.range_min = 0.1f, L.range_max = 10.0f;
  L.range_threshold_scale = 0.95, L.n_beams = 8;
  const int64_t off1[2] = {0, 2};
  const int32_t good[2] = {3, 7}, not_inc[2] = {3, 3}, zero_first[2] = {0, 7}, short_last[2] = {3, 6};
  const double P[9] = {0, 0, 0, 0.1, 0, 0.1, 0.2, 0, 0.2};
  double Pbad[9] = {0, 0, 0, 0.1, nan, 0.1, 0.2, 0, 0.2};
  CHECK(csm::deskew::plan_valid(L, 1, off1, good, P));
  CHECK(!csm::deskew::plan_valid(L, 1, off1, not_inc, P));
  CHECK(!csm::deskew::plan_valid(L, 1, off1, zero_first, P));
  CHECK(!csm::deskew::plan_valid(L, 1, off1, short_last, P));
  CHECK(!csm::deskew::plan_valid(L, 1, off1, good, Pbad));
  CHECK(!csm::deskew::plan_valid(L, 1, off1, good, nullptr));
  csm_laser L0 = L;
  L0.angle_increment = 0.0f;
  CHECK(!csm::deskew::plan_valid(L0, 1, off1, good, P));
  L0 = L;
  L0.n_beams = 1;
  CHECK(!csm::deskew::plan_valid(L0, 1, off1, good, P));
  std::printf("cases=%d scans=%lld plans=%d fails=%d\n", n_cases, (long long)scans_done, plans, fails);
  if (fails == 0) std::printf("deskew_check ok\n");
  return fails == 0 ? 0 : 1;
}
