// search_gate_check.cpp — csrc/csm_search_gate.hpp alone on the host, driven
// by tests/test_search_gate_host.py (which holds the Python restatement).
//
//   (no argument)  a self-check of the key's round trip; prints "search_gate_check ok"
//   --keys         stdin: one double per line as its 64 bits in hex
//                  stdout: select_key(x) and the bits of gate_key_score(select_key(x)), hex
//   --results      stdin: cases "n_windows n_cand capacity", then n_windows lines
//                  "key(hex) flat(decimal)"; stdout per case: n_pass, then the
//                  written entries "window score_bits(hex) flat"
//   --after        stdin: "descents listed capacity fixed" per line
//                  stdout: "next grow_to" (next: 0 done, 1 redescend, 2 grow, 3 fallback)
//   --first        stdin: "asked list_has" per line; stdout: the first capacity
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "csm_search_gate.hpp"

namespace {

uint64_t bits(double x) { return (uint64_t)__builtin_bit_cast(int64_t, x); }
double from_bits(uint64_t u) { return __builtin_bit_cast(double, u); }

int self_check() {
  const double inf = std::numeric_limits<double>::infinity();
  const double v[] = {-inf, -1.5, -1e-300, -4.9e-324, -0.0, 0.0, 4.9e-324, 0.3, 1.0, 1.1414, 2.0, inf};
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) {
    const uint64_t k = csm::select_key(v[i]);
    const double back = csm::gate_key_score(k);
    const double want = v[i] + 0.0;  // the key of -0.0 is +0.0's
    if (bits(back) != bits(want)) {
      std::printf("round trip of %a gives %a\n", v[i], back);
      return 1;
    }
    if (i > 0 && !(csm::select_key(v[i - 1]) <= k)) {
      std::printf("keys out of order at %a\n", v[i]);
      return 1;
    }
    if (i > 0 && v[i - 1] < v[i] && !(csm::select_key(v[i - 1]) < k)) {
      std::printf("keys not strictly ordered at %a\n", v[i]);
      return 1;
    }
  }
  std::printf("search_gate_check ok\n");
  return 0;
}

int keys() {
  uint64_t u;
  while (std::scanf("%" SCNx64, &u) == 1) {
    const uint64_t k = csm::select_key(from_bits(u));
    std::printf("%016" PRIx64 " %016" PRIx64 "\n", k, bits(csm::gate_key_score(k)));
  }
  return 0;
}

int results() {
  int64_t nw, n_cand, capacity;
  while (std::scanf("%" SCNd64 " %" SCNd64 " %" SCNd64, &nw, &n_cand, &capacity) == 3) {
    // exactly sized, so the sanitizer sees a write past either end
    std::vector<uint64_t> wkey((size_t)nw);
    std::vector<int64_t> wflat((size_t)nw);
    for (int64_t w = 0; w < nw; ++w)
      if (std::scanf("%" SCNx64 " %" SCNd64, &wkey[(size_t)w], &wflat[(size_t)w]) != 2) return 2;
    std::vector<csm::GatePass> out((size_t)capacity);
    const int64_t n = csm::gate_results(wkey.data(), wflat.data(), nw, n_cand, capacity > 0 ? out.data() : nullptr, capacity);
    std::printf("%" PRId64 "\n", n);
    for (int64_t k = 0; k < (n < capacity ? n : capacity); ++k)
      std::printf("%d %016" PRIx64 " %" PRId64 "\n", out[(size_t)k].window, bits(out[(size_t)k].score), out[(size_t)k].flat);
  }
  return 0;
}

int after() {
  int descents, fixed;
  int64_t listed, capacity;
  while (std::scanf("%d %" SCNd64 " %" SCNd64 " %d", &descents, &listed, &capacity, &fixed) == 4) {
    int64_t grow_to = capacity;
    const csm::GateNext nx = csm::gate_after(descents, listed, capacity, fixed != 0, &grow_to);
    std::printf("%d %" PRId64 "\n", (int)nx, grow_to);
  }
  return 0;
}

int first() {
  int64_t asked, has;
  while (std::scanf("%" SCNd64 " %" SCNd64, &asked, &has) == 2)
    std::printf("%" PRId64 "\n", csm::gate_first_capacity(asked, has));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return self_check();
  if (!std::strcmp(argv[1], "--keys")) return keys();
  if (!std::strcmp(argv[1], "--results")) return results();
  if (!std::strcmp(argv[1], "--after")) return after();
  if (!std::strcmp(argv[1], "--first")) return first();
  return 2;
}
