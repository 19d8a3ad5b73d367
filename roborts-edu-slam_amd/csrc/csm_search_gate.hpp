// csm_search_gate.hpp — the host half of the gated search (csm_search_gated,
// include/csm.h): what a descent's per-window device state means, and what to
// do when its list overflowed.
//
// The device leaves, per window w (csm_select.hpp, pyr_gate_kernel):
//   wkey[w]   the maximum of select_key(score) over the window's candidates at
//             or above the gate (complete after any descent: the atomicMax does
//             not depend on the list's room)
//   wflat[w]  the lowest global flat index (w * n_cand + flat) among the listed
//             candidates whose key equals wkey[w]; INT64_MAX when there is none
// A window passes iff wflat[w] != INT64_MAX: no key value stands for "none".
// When the list held everything appended to it, wflat[w] is the lowest index
// among all the window's best candidates: csm_best_window's tie rule.
//
// Host only, no HIP call: tests/cpp/search_gate_check.cpp drives it alone.
#pragma once

#include <climits>
#include <cstdint>

#include "csm_search_match.hpp"  // select_key

namespace csm {

// select_key's inverse on the keys it produces. -0.0 and +0.0 share a key, so
// a zero comes back as +0.0 (a candidate's score is never -0.0: it is a
// non-negative factor times the quotient of an integer's double).
inline double gate_key_score(uint64_t key) {
  const uint64_t u = (key >> 63) ? (key & ~((uint64_t)1 << 63)) : ~key;
  return __builtin_bit_cast(double, u);
}

struct GatePass {
  int32_t window;
  double score;
  int64_t flat;  // within the window
};

// The passing windows in ascending order: out[k] for k < min(n_pass,
// capacity) (out may be null when capacity is 0); returns n_pass, the count of
// every passing window.
inline int64_t gate_results(const uint64_t* wkey, const int64_t* wflat, int64_t n_windows, int64_t n_cand, GatePass* out,
                            int64_t capacity) {
  int64_t n_pass = 0;
  for (int64_t w = 0; w < n_windows; ++w) {
    if (wflat[w] == INT64_MAX) continue;
    if (n_pass < capacity) out[n_pass] = GatePass{(int32_t)w, gate_key_score(wkey[w]), wflat[w] - w * n_cand};
    ++n_pass;
  }
  return n_pass;
}

// After descent number `descents` (1, 2, 3) appended `listed` entries to a
// list of `capacity`:
//   kDone       the list held them all: the state is the answer
//   kRedescend  descend again with the keys kept (the list then takes only
//               candidates tied at their window's maximum)
//   kGrow       automatic capacity only, after the second overflow: the count
//               is deterministic now (every tied candidate, nothing else), so
//               a list of *grow_to = listed entries holds the third descent's
//   kFallback   the exhaustive per-window argmax: a fixed capacity after the
//               second overflow, more than kGateMaxList entries, or an overflow
//               that outlived the grown list
constexpr int64_t kGateMinList = 10240;
constexpr int64_t kGateMaxList = (int64_t)1 << 26;  // entries: 1 GiB
enum class GateNext { kDone, kRedescend, kGrow, kFallback };
inline GateNext gate_after(int descents, int64_t listed, int64_t capacity, bool fixed_capacity, int64_t* grow_to) {
  if (listed <= capacity) return GateNext::kDone;
  if (descents <= 1) return GateNext::kRedescend;
  if (descents == 2 && !fixed_capacity && listed <= kGateMaxList) {
    *grow_to = listed;
    return GateNext::kGrow;
  }
  return GateNext::kFallback;
}

// The first descent's list: as many entries as asked (never grown), or
// automatically the larger of kGateMinList and what the context's list has
// grown to.
inline int64_t gate_first_capacity(int64_t asked, int64_t list_has) {
  if (asked > 0) return asked;
  return list_has > kGateMinList ? list_has : kGateMinList;
}

}  // namespace csm
