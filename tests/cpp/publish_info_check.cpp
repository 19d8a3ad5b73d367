// publish_info_check.cpp — the map publisher's host rules
// (csrc/csm_gridmap_publish.hpp) as a stand-alone host program: no HIP, no
// library. Without arguments it checks fixed cases (the reference's formulas
// restated inline) and prints "publish_info_check ok". With --eval it reads
// one case per line from stdin, "min_x min_y max_x max_y resolution offset_x
// offset_y" as hex floats, and prints "start_x start_y width height origin_x
// origin_y resolution" (the doubles as hex floats) for
// tests/test_publish_info.py to compare with its Python restatement. Built
// plain and with -fsanitize=address,undefined,float-cast-overflow: a
// floor(FLT_MAX) converted to int, as the reference's start_x does, stops it.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "csm_gridmap_publish.hpp"

namespace {

int failed = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failed;                                                            \
    }                                                                      \
  } while (0)

bool same_box(const csm::PublishBox& b, int sx, int sy, int w, int h) {
  return b.start_x == sx && b.start_y == sy && b.width == w && b.height == h;
}

void fixed_cases() {
  using csm::publish_box;
  // a bound box never set (util/boundbox.h:38-42): 0 x 0 at (0, 0)
  CHECK(same_box(publish_box((double)FLT_MAX, (double)FLT_MAX, (double)FLT_MIN, (double)FLT_MIN), 0, 0, 0, 0));
  // integer-valued bounds: ceil(max) - floor(min) + 1, both ends included
  CHECK(same_box(publish_box(3.0, 34.0, 128.0, 204.0), 3, 34, 126, 171));
  // fractional bounds round outwards
  CHECK(same_box(publish_box(3.25, 34.5, 127.5, 203.01), 3, 34, 126, 171));
  // negative bounds: floor goes down
  CHECK(same_box(publish_box(-2.5, -0.5, 1.5, 0.0), -3, -1, 6, 2));
  // max below min by less than a cell still spans cells; by a whole cell it is empty
  CHECK(same_box(publish_box(5.5, 5.5, 4.7, 4.7), 5, 5, 1, 1));
  CHECK(same_box(publish_box(5.5, 1.0, 3.2, 2.0), 0, 0, 0, 2));
  CHECK(same_box(publish_box(1.0, 5.5, 2.0, 3.2), 0, 0, 2, 0));
  // what the reference leaves undefined is an empty grid here
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(same_box(publish_box(nan, 0.0, 4.0, 4.0), 0, 0, 0, 5));
  CHECK(same_box(publish_box(0.0, 0.0, inf, 4.0), 0, 0, 0, 5));
  CHECK(same_box(publish_box(-inf, 0.0, inf, 4.0), 0, 0, 0, 5));
  CHECK(same_box(publish_box(0.0, 0.0, 3e9, 4.0), 0, 0, 0, 5));
  CHECK(same_box(publish_box(1e12, 0.0, 1e12 + 5, 4.0), 0, 0, 0, 5));
  CHECK(same_box(publish_box(-2147483648.0, 0.0, -2147483647.0, 0.0), INT32_MIN, 0, 2, 1));
  CHECK(same_box(publish_box(0.0, 0.0, 2147483645.0, 0.0), 0, 0, 2147483646, 1));
  CHECK(same_box(publish_box(0.0, 0.0, 2147483646.0, 0.0), 0, 0, 2147483647, 1));
  CHECK(same_box(publish_box(0.0, 0.0, 2147483647.0, 0.0), 0, 0, 0, 1));
  bool fits = true;
  CHECK(csm::publish_axis_size(2.0, 0.5, &fits) == 0 && !fits);
  CHECK(csm::publish_axis_size(2.0, 2.0, &fits) == 1 && fits);
  // the full-map form
  CHECK(same_box(csm::publish_full_box(160, 239), 0, 0, 160, 239));
  // origin: scale 20 (0.05 m cells), offset (1, -2): cell (3, 34) lies at
  // 3 / 20 - 1 = -0.85 and 34 / 20 + 2 = 3.7; minus half a cell
  double ox = 0, oy = 0;
  csm::publish_origin(1.0 / 0.05, 1.0, -2.0, 3, 34, &ox, &oy);
  CHECK(std::fabs(ox - (-0.875)) < 1e-12 && std::fabs(oy - 3.675) < 1e-12);
  // a power-of-two scale is exact
  csm::publish_origin(4.0, 0.5, 0.25, -3, 8, &ox, &oy);
  CHECK(ox == -3 / 4.0 - 0.5 - 0.125 && oy == 8 / 4.0 - 0.25 - 0.125);
  CHECK(csm::publish_resolution(4.0) == 0.25);
}

int eval_stdin() {
  double v[7];
  for (;;) {
    const int got = std::scanf("%la %la %la %la %la %la %la", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]);
    if (got == EOF) return 0;
    if (got != 7) return 2;
    const csm::PublishBox b = csm::publish_box(v[0], v[1], v[2], v[3]);
    const double scale = 1.0 / v[4];  // scale_factor_ (map/grid_map_base.h:50)
    double ox = 0, oy = 0;
    csm::publish_origin(scale, v[5], v[6], b.start_x, b.start_y, &ox, &oy);
    std::printf("%d %d %d %d %a %a %a\n", b.start_x, b.start_y, b.width, b.height, ox, oy,
                csm::publish_resolution(scale));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--eval") == 0) return eval_stdin();
  fixed_cases();
  std::printf("failed=%d\n", failed);
  if (failed) return 1;
  std::printf("publish_info_check ok\n");
  return 0;
}
