// map_check_plan_check.cpp — the map check's host rules
// (csrc/csm_map_check_plan.hpp) as a stand-alone host program: no HIP, no
// library. Without arguments it checks fixed cases (the reference's rules,
// map/occu_grid_map.h:331-392, restated inline) and prints
// "map_check_plan_check ok". With --eval it reads one question per line from
// stdin and answers it on one line, doubles as hex floats, for
// tests/test_map_check_plan.py to compare with its Python restatement:
//
//   guard cpn tol gain                  -> 0 | 1
//   step n cpn                          -> div0 step checked   (0 0 when div0)
//   mind2 tol                           -> min_d2
//   pose scale ox oy sx sy x y th       -> inside tx ty c s x0 y0 no_rays
//   coeff count gain                    -> coefficient logistic(coefficient)
//
// Built plain and with -fsanitize=address,undefined,float-cast-overflow: no
// rule may convert a value the int cannot hold or divide by zero.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "csm_map_check_plan.hpp"

namespace {

int failed = 0;

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failed;                                                     \
    }                                                               \
  } while (0)

void fixed_cases() {
  using namespace csm;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // the guard (:337-341): both ends of (0, 1) are outside, a NaN passes every compare
  CHECK(map_check_guard(50, -1e-300, 0.015) && map_check_guard(0, 2.5, 0.015) && map_check_guard(-3, 2.5, 0.015));
  CHECK(map_check_guard(50, 2.5, 0.0) && map_check_guard(50, 2.5, 1.0) && map_check_guard(50, 2.5, -0.5));
  CHECK(!map_check_guard(50, 0.0, 0.015) && !map_check_guard(1, 2.5, 0.999) && !map_check_guard(50, nan, nan));
  // the beam rule (:362-372)
  CHECK(map_check_step(99, 50) == 1 && map_check_checked(99, 1) == 99);
  CHECK(map_check_step(100, 50) == 2 && map_check_checked(100, 2) == 50);
  CHECK(map_check_step(101, 50) == 2 && map_check_checked(101, 2) == 51);
  CHECK(map_check_step(1081, 100) == 10 && map_check_checked(1081, 10) == 109);
  CHECK(map_check_step(0, 7) == 1 && map_check_checked(0, 1) == 0);
  CHECK(map_check_step(4, 2) == 4 && map_check_checked(4, 4) == 1);
  CHECK(map_check_step(2147483647, 3) == 1073741823 && map_check_checked(2147483647, 1073741823) == 3);
  CHECK(map_check_step(2147483647, 2147483647) == 1);
  CHECK(map_check_divides_by_zero(1, 2) && !map_check_divides_by_zero(1, 1) && !map_check_divides_by_zero(2, 100));
  CHECK(map_check_step(1, 1) == 1 && map_check_step(0, 1) == 1);
  // min_d2: sqrt(d2) > tolerance
  CHECK(map_check_min_d2(0.0) == 1 && map_check_min_d2(1.0) == 2 && map_check_min_d2(2.5) == 7);
  CHECK(map_check_min_d2(3.0) == 10 && map_check_min_d2(std::sqrt(2.0)) == 3);
  CHECK(map_check_min_d2(nan) == INT64_MAX && map_check_min_d2(1e12) == INT64_MAX && map_check_min_d2(inf) == INT64_MAX);
  // the pose record: scale 20, offset (4, 6), pose (0.26, -0.49) -> (85.2, 110.2)
  MapCheckPose r;
  const double p0[3] = {0.26, -0.49, 0.0};
  CHECK(map_check_pose(20.0, 4.0, 6.0, 160, 239, p0, &r) && r.x0 == 85 && r.y0 == 110 && !r.no_rays);
  CHECK(r.c == 1.0 && r.s == 0.0);
  const double on_border[3] = {-4.0, 0.0, 1.0};  // tx == 0: PointInMap is strict
  CHECK(!map_check_pose(20.0, 4.0, 6.0, 160, 239, on_border, &r) && r.no_rays == 1);
  const double far_out[3] = {1e300, 0.0, 0.0}, bad[3] = {nan, 0.0, inf};
  CHECK(!map_check_pose(20.0, 4.0, 6.0, 160, 239, far_out, &r) && r.no_rays == 1);
  CHECK(!map_check_pose(20.0, 4.0, 6.0, 160, 239, bad, &r) && r.no_rays == 1);
  const double last[3] = {3.999, 5.949, nan};  // just inside the far corner; a NaN angle is the kernel's to skip
  CHECK(map_check_pose(20.0, 4.0, 6.0, 160, 239, last, &r) && r.x0 == 160 && r.y0 == 239 && r.c != r.c);
  // the coefficient (:388-391) and the logistic (slam_processor.cpp:590)
  CHECK(map_check_coeff(0, 0.015) == 1.0 + 2 * 0.015);
  CHECK(map_check_coeff(2, 0.015) == 1.0 + 2 * 0.015 - 2 * 0.015);
  CHECK(map_check_coeff(200, 0.05) == 0.1 && map_check_coeff(19, 0.05) == std::fmax(1.0 + 2 * 0.05 - 19 * 0.05, 0.1));
  CHECK(map_check_logistic(0.4) == 0.5 && map_check_logistic(0.0) == 1 / (1 + std::exp(4.0)));
}

int eval_stdin() {
  char kind[16];
  for (;;) {
    const int got = std::scanf("%15s", kind);
    if (got == EOF) return 0;
    if (got != 1) return 2;
    if (!std::strcmp(kind, "guard")) {
      int cpn;
      double tol, gain;
      if (std::scanf("%d %la %la", &cpn, &tol, &gain) != 3) return 2;
      std::printf("%d\n", csm::map_check_guard(cpn, tol, gain) ? 1 : 0);
    } else if (!std::strcmp(kind, "step")) {
      int n, cpn;
      if (std::scanf("%d %d", &n, &cpn) != 2) return 2;
      if (csm::map_check_divides_by_zero(cpn, n)) {
        std::printf("1 0 0\n");
      } else {
        const int32_t step = csm::map_check_step(n, cpn);
        std::printf("0 %d %d\n", step, csm::map_check_checked(n, step));
      }
    } else if (!std::strcmp(kind, "mind2")) {
      double tol;
      if (std::scanf("%la", &tol) != 1) return 2;
      std::printf("%lld\n", (long long)csm::map_check_min_d2(tol));
    } else if (!std::strcmp(kind, "pose")) {
      double scale, ox, oy, pose[3];
      int sx, sy;
      if (std::scanf("%la %la %la %d %d %la %la %la", &scale, &ox, &oy, &sx, &sy, &pose[0], &pose[1], &pose[2]) != 8)
        return 2;
      csm::MapCheckPose r;
      const bool in = csm::map_check_pose(scale, ox, oy, sx, sy, pose, &r);
      std::printf("%d %a %a %a %a %d %d %d\n", in ? 1 : 0, r.tx, r.ty, r.c, r.s, r.x0, r.y0, r.no_rays);
    } else if (!std::strcmp(kind, "coeff")) {
      long long count;
      double gain;
      if (std::scanf("%lld %la", &count, &gain) != 2) return 2;
      const double c = csm::map_check_coeff(count, gain);
      std::printf("%a %a\n", c, csm::map_check_logistic(c));
    } else {
      return 2;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--eval") == 0) return eval_stdin();
  fixed_cases();
  std::printf("failed=%d\n", failed);
  if (failed) return 1;
  std::printf("map_check_plan_check ok\n");
  return 0;
}
