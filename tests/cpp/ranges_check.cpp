// ranges_check — csrc/csm_ranges_host.hpp (the host arithmetic behind
// csm_laser_range_threshold and csm_ranges_to_points) compiled alone, for
// tests/test_ranges_host.py's ASan + UBSan run: every buffer is a heap block
// of exactly the size the interface asks for, so a read or write past a scan,
// the table, the offsets or the capacity is reported.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "csm_ranges_host.hpp"

namespace {

int fails = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);  \
      ++fails;                                                    \
    }                                                             \
  } while (0)

csm_laser laser(int32_t n_beams, float amin, float ainc, float rmin, float rmax, double scale) {
  csm_laser L{};
  L.angle_min = amin;
  L.angle_increment = ainc;
  L.range_min = rmin;
  L.range_max = rmax;
  L.range_threshold_scale = scale;
  L.n_beams = n_beams;
  return L;
}

// ranges of n_scans scans: edge values and ordinary ones, scan 0, the middle
// one and the last all dropped
std::vector<float> make_ranges(const csm_laser& L, double thr, int32_t n_scans, uint32_t seed) {
  const float inf = std::numeric_limits<float>::infinity();
  const float t32 = (float)thr;
  const float edge[] = {std::nanf(""), inf, -inf, 0.0f, -1.0f, L.range_min, std::nextafter(L.range_min, inf),
                        t32, std::nextafter(t32, -inf), std::nextafter(t32, inf), L.range_max,
                        std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max()};
  const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
  std::vector<float> r((size_t)n_scans * L.n_beams);
  uint32_t x = seed * 2654435761u + 1u;
  for (int32_t s = 0; s < n_scans; ++s)
    for (int32_t i = 0; i < L.n_beams; ++i) {
      x = x * 1664525u + 1013904223u;
      const bool dead = s == 0 || s == n_scans / 2 || s == n_scans - 1;
      float v;
      if (dead)
        v = edge[(x >> 8) % 6];  // NaN, +-inf, 0, -1, range_min: all dropped
      else if ((x >> 28) < 5)
        v = edge[(x >> 8) % n_edge];
      else
        v = L.range_min + (float)((x >> 8) & 0xFFFF) / 65536.0f * (float)(thr - (double)L.range_min);
      r[(size_t)s * L.n_beams + i] = v;
    }
  return r;
}

void run(const csm_laser& L, int32_t n_scans, double factor, uint32_t seed) {
  double thr = 0.0;
  CHECK(csm::laser_threshold(L, &thr));
  CHECK(thr == (double)L.range_min + L.range_threshold_scale * ((double)L.range_max - (double)L.range_min));
  std::vector<double> cs((size_t)L.n_beams * 2);
  csm::laser_trig_table(L, cs.data());
  const std::vector<float> r = make_ranges(L, thr, n_scans, seed);
  std::vector<int64_t> off((size_t)n_scans + 1, -1), off2((size_t)n_scans + 1, -1);
  // offsets only
  CHECK(csm::ranges_to_points(L, thr, nullptr, n_scans, r.data(), factor, nullptr, 0, off.data()));
  const int64_t total = off[(size_t)n_scans];
  CHECK(off[0] == 0 && off[1] == 0 && off[(size_t)n_scans] == off[(size_t)n_scans - 1]);
  CHECK(off[(size_t)n_scans / 2 + 1] == off[(size_t)n_scans / 2]);
  // exactly enough room
  std::vector<double> pts((size_t)total * 2);
  CHECK(csm::ranges_to_points(L, thr, cs.data(), n_scans, r.data(), factor, pts.data(), total, off2.data()));
  CHECK(off == off2);
  // each point against its beam, recomputed here
  int64_t k = 0;
  for (int32_t s = 0; s < n_scans; ++s) {
    double a = (double)L.angle_min;
    for (int32_t i = 0; i < L.n_beams; ++i) {
      const double d = (double)r[(size_t)s * L.n_beams + i];
      if (d > (double)L.range_min && d < thr) {
        double sn, c;
        ::sincos(a, &sn, &c);
        const double x = c * d, y = sn * d;
        CHECK(k < total && pts[(size_t)2 * k] == x * factor && pts[(size_t)2 * k + 1] == y * factor);
        ++k;
      }
      a += (double)L.angle_increment;
    }
    CHECK(off[(size_t)s + 1] == k);
  }
  // one point short: refused, nothing past the (exactly sized) block
  if (total > 1) {  // (an empty block's null data() would ask for the offsets only)
    std::vector<double> small((size_t)(total - 1) * 2);
    CHECK(!csm::ranges_to_points(L, thr, cs.data(), n_scans, r.data(), factor, small.data(), total - 1, off2.data()));
  }
}

}  // namespace

int main() {
  const float pi = 3.14159265358979f;
  const int beams[] = {1, 63, 64, 65, 129, 1081};
  const double factors[] = {1 / 0.05, 1 / 0.025, 1 / 0.01, 1.0};
  int runs = 0;
  for (int nb : beams)
    for (double f : factors) {
      run(laser(nb, -0.75f * pi, 1.5f * pi / 1080.0f, 0.1f, 10.0f, 0.95), 7, f, (uint32_t)(nb * 4 + runs));
      run(laser(nb, -2.0f, 0.00390625f, 0.5f, 8.5f, 0.5), 5, f, (uint32_t)(nb * 8 + runs));    // threshold 4.5
      run(laser(nb, 2.0f, -0.006f, 0.06f, 5.6f, 0.9), 6, f, (uint32_t)(nb * 16 + runs));       // beams run backwards
      runs += 3;
    }
  // what csm_laser_range_threshold refuses
  double t;
  const float inf = std::numeric_limits<float>::infinity();
  CHECK(!csm::laser_threshold(laser(0, 0.f, 0.1f, 0.1f, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(-3, 0.f, 0.1f, 0.1f, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, 0.1f, 10.f, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, 0.1f, 10.f, 0.1f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, std::nanf(""), 0.1f, 0.1f, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, inf, 0.1f, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, 0.1f, -inf, 10.f, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, 0.1f, 0.1f, inf, 0.95), &t));
  CHECK(!csm::laser_threshold(laser(8, 0.f, 0.1f, 0.1f, 10.f, std::nan("")), &t));
  std::printf("runs=%d fails=%d\n", runs, fails);
  if (fails == 0) std::printf("ranges_check ok\n");
  return fails == 0 ? 0 : 1;
}
