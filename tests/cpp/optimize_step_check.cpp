// optimize_step_check.cpp — the Gauss-Newton matcher's step rules
// (csrc/csm_optimize_step.hpp) driven on the CPU: reads cases from a binary
// file, applies csm::opt::step and csm::opt::ldlt_solve3 to each, writes the
// results to another; tests/test_optimize_step.py compares them with the
// pure-Python restatement bit for bit. Stand-alone: the header alone, no HIP.
//
//   optimize_step_check <cases.bin> <results.bin>
//
// A case is kCaseDoubles doubles: v[10] (the ten sums), valid, previous cost,
// est[3], iter, cost_decrease_threshold, cost_min_threshold, max_update_cells,
// max_update_angle. A result is kResultDoubles doubles: state, cost, est[3],
// det[3] (ldlt_solve3 of the case's H and b).
#include <cstdio>
#include <vector>

#include "csm_optimize_step.hpp"

namespace {

constexpr int kCaseDoubles = 20;
constexpr int kResultDoubles = 8;

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <cases.bin> <results.bin>\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<double> cases;
  double buf[kCaseDoubles];
  while (std::fread(buf, sizeof(double), kCaseDoubles, in) == (size_t)kCaseDoubles)
    cases.insert(cases.end(), buf, buf + kCaseDoubles);
  std::fclose(in);
  const size_t n = cases.size() / kCaseDoubles;
  std::vector<double> out(n * kResultDoubles);
  for (size_t i = 0; i < n; ++i) {
    const double* c = &cases[i * kCaseDoubles];
    double* r = &out[i * kResultDoubles];
    const csm::opt::StepParam P{c[16], c[17], c[18], c[19]};
    double est[3] = {c[12], c[13], c[14]};
    double cost = c[11];
    const int32_t state = csm::opt::step(c, (int32_t)c[10], (int)c[15], P, est, &cost);
    r[0] = (double)state;
    r[1] = cost;
    r[2] = est[0];
    r[3] = est[1];
    r[4] = est[2];
    csm::opt::ldlt_solve3(c + 1, c + 7, r + 5);
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) {
    std::perror(argv[2]);
    return 2;
  }
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
  if (std::fclose(o) != 0 || !ok) {
    std::fprintf(stderr, "short write\n");
    return 2;
  }
  std::printf("optimize_step_check ok cases=%zu\n", n);
  return 0;
}
