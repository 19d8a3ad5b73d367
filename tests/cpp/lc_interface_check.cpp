// lc_interface_check.cpp — the host rules of csm_loop_closure_scan_match
// (csrc/csm_lc_interface.hpp) as a stand-alone host program: no HIP, no
// library. Without arguments it checks fixed cases (the reference's rules,
// scan_matchers.h:179-289,365-390, grid_map_base.h:247-273,
// slam_processor.cpp:316-317, restated inline) and prints
// "lc_interface_check ok". With --eval it reads one question per line from
// stdin and answers it on one line, doubles as hex floats, for
// tests/test_lc_interface_host.py to compare with its Python restatement:
//
//   box res ox oy px py rmax sss sx sy   -> fits min_x min_y max_x max_y size_that_fits
//   start accepted ax ay at px py pt      -> x y t
//   score levels r0 r1 r2 penalty         -> mean score
//   gate T levels                         -> gate
//
// Built plain and with -fsanitize=address,undefined,float-cast-overflow.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "csm_lc_interface.hpp"

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
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // the back end's map: (10 + 2) * 2 / 0.25 = 96 cells, centred on the pose; the box's half side
  // is (10 + 2) / 0.25 = 48 cells: min = 0 is on the bound (strict: does not fit)
  const double off96[2] = {12.0, 12.0}, origin[3] = {0.0, 0.0, 0.3};
  InterfaceBox b = interface_box(0.25, off96, origin, 10.0, 2.0);
  CHECK(b.min_x == 0.0 && b.min_y == 0.0 && b.max_x == 96.0 && b.max_y == 96.0);
  CHECK(!interface_box_fits(b, 96, 96));
  CHECK(interface_size_that_fits(b, 96, 96) == 97);
  // a window of 1.5 m: half side 46 cells, corners (2, 2) and (94, 94)
  b = interface_box(0.25, off96, origin, 10.0, 1.5);
  CHECK(b.min_x == 2.0 && b.max_x == 94.0 && interface_box_fits(b, 96, 96));
  // the far bound is size + 1 (UpdateBoundAdaptMap): max = 97 touches it, 96.75 is inside
  const double right[3] = {0.75, 0.0, 0.0}, inside[3] = {1.1875, 0.0, 0.0};
  b = interface_box(0.25, off96, right, 10.0, 1.5);
  CHECK(b.max_x == 97.0 && !interface_box_fits(b, 96, 96));
  b = interface_box(0.25, off96, inside, 10.0, 1.0);
  CHECK(b.max_x == 96.75 && b.min_x == 8.75 && interface_box_fits(b, 96, 96));
  // each side on its own, and a NaN
  const double left[3] = {-0.75, 0.0, 0.0}, down[3] = {0.0, -0.75, 0.0}, up[3] = {0.0, 0.75, 0.0}, bad[3] = {nan, 0.0, 0.0};
  CHECK(!interface_box_fits(interface_box(0.25, off96, left, 10.0, 1.5), 96, 96));
  CHECK(!interface_box_fits(interface_box(0.25, off96, down, 10.0, 1.5), 96, 96));
  CHECK(!interface_box_fits(interface_box(0.25, off96, up, 10.0, 1.5), 96, 96));
  CHECK(!interface_box_fits(interface_box(0.25, off96, bad, 10.0, 1.5), 96, 96));
  CHECK(interface_size_that_fits(interface_box(0.25, off96, bad, 10.0, 1.5), 96, 96) == -1);
  // one cell too small: 95 cells, centred the same
  const double off95[2] = {0.5 * 95 * 0.25, 0.5 * 95 * 0.25};
  b = interface_box(0.25, off95, origin, 10.0, 1.75);  // half side 47: min 0.5, max 94.5 in 95 cells
  CHECK(interface_box_fits(b, 95, 95) && !interface_box_fits(b, 93, 95) && !interface_box_fits(b, 95, 93));
  // the start pose
  const double avg[3] = {1.0, 2.0, 3.0}, in[3] = {-1.0, -2.0, -3.0};
  double out[3];
  interface_start_pose(1, avg, in, out);
  CHECK(out[0] == 1.0 && out[1] == 2.0 && out[2] == 3.0);
  interface_start_pose(0, avg, in, out);
  CHECK(out[0] == -1.0 && out[1] == -2.0 && out[2] == -3.0);
  // the score
  const double r3[3] = {0.5, 0.75, 1.0}, over[3] = {1.5, 1.5, 1.5};
  CHECK(interface_mean(r3, 3) == (0.0 + 0.5 + 0.75 + 1.0) / 3 && interface_mean(r3, 1) == 0.5);
  CHECK(interface_score(0.75, 1.0) == 0.75 && interface_score(0.75, 0.0) == 0.0 && interface_score(0.75, 0.5) == 0.375);
  CHECK(interface_score(interface_mean(over, 3), 0.5) == 0.75);  // the clamp comes after the penalty
  CHECK(interface_score(1.0, 1.03) == 1.0 && interface_score(interface_mean(over, 1), 1.0) == 1.0);
  // the wide gate
  CHECK(interface_wide_gate(0.6, 1) == 0.6);
  CHECK(interface_wide_gate(0.75, 3) < 0.25 && interface_wide_gate(0.75, 3) > 0.25 - 1e-14);
}

int eval_stdin() {
  char kind[16];
  for (;;) {
    const int got = std::scanf("%15s", kind);
    if (got == EOF) return 0;
    if (got != 1) return 2;
    if (!std::strcmp(kind, "box")) {
      double res, off[2], pose[3] = {0.0, 0.0, 0.0}, rmax, sss;
      int sx, sy;
      if (std::scanf("%la %la %la %la %la %la %la %d %d", &res, &off[0], &off[1], &pose[0], &pose[1], &rmax, &sss, &sx,
                     &sy) != 9)
        return 2;
      const csm::InterfaceBox b = csm::interface_box(res, off, pose, rmax, sss);
      std::printf("%d %a %a %a %a %lld\n", csm::interface_box_fits(b, sx, sy) ? 1 : 0, b.min_x, b.min_y, b.max_x, b.max_y,
                  (long long)csm::interface_size_that_fits(b, sx, sy));
    } else if (!std::strcmp(kind, "start")) {
      int accepted;
      double a[3], p[3], out[3];
      if (std::scanf("%d %la %la %la %la %la %la", &accepted, &a[0], &a[1], &a[2], &p[0], &p[1], &p[2]) != 7) return 2;
      csm::interface_start_pose(accepted, a, p, out);
      std::printf("%a %a %a\n", out[0], out[1], out[2]);
    } else if (!std::strcmp(kind, "score")) {
      int levels;
      double r[3], pen;
      if (std::scanf("%d %la %la %la %la", &levels, &r[0], &r[1], &r[2], &pen) != 5) return 2;
      if (levels != 1 && levels != 3) return 2;
      const double mean = csm::interface_mean(r, levels);
      std::printf("%a %a\n", mean, csm::interface_score(mean, pen));
    } else if (!std::strcmp(kind, "gate")) {
      double T;
      int levels;
      if (std::scanf("%la %d", &T, &levels) != 2) return 2;
      std::printf("%a\n", csm::interface_wide_gate(T, levels));
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
  std::printf("lc_interface_check ok\n");
  return 0;
}
