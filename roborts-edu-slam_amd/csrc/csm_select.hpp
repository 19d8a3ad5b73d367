// csm_select.hpp — the selection the reduced finish cuts out of a collected
// list, on the device (csm_search_match.hpp states the definition and why the
// selected subset is sufficient for list_finish).
//
// Over hits[0, n), n = min(*n_dev, cap) read on the device (the collect's
// counter; cap: the entries the list holds):
//
//   S = { h : pred(h) and (key(h) >= key_K or (band_on and in_response_band(h.score, best))) }
//
// pred, key and key_K as SelectSpec / select_key say. key_K comes from a radix
// select from the top digit down, kSelBits bits a pass: select_hist_kernel
// counts the current digit of the hits that pass pred and match the prefix
// fixed so far (an LDS histogram per block, one global atomic per non-empty
// bin per block), select_pick_kernel (one block) scans the bins from the top,
// fixes the digit, updates prefix and remaining rank in device memory and
// clears the bins: no host round trip between passes. select_compact_kernel
// appends S (a ballot, one returning atomic per wave: pyr_collect_kernel's
// idiom), counting every member and writing only slots below out_cap.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "csm_search_match.hpp"

namespace csm {

constexpr int kSelBits = 11;  // 6 passes over a 64-bit key: 11, 11, 11, 11, 11, 9 bits
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelPasses = 6;
constexpr int kSelMaxBlocks = 2048;  // of 256 threads, striding over longer lists

// A selection's device state, set by its init launch.
struct SelectState {
  unsigned long long prefix;     // the key's digits fixed so far (after the last pass: key_K)
  unsigned long long remaining;  // the rank still to find among the hits matching the prefix
  unsigned int all;              // fewer than K hits pass pred: every one of them is selected
  unsigned int pad;
  unsigned int bins[kSelBins];
};

// The output: the full count of S, then its first out_cap members in any order.
struct SelectHead {
  unsigned long long count;
  unsigned long long key;  // key_K (0 when SelectState::all)
};
inline size_t select_out_bytes(int64_t out_cap) { return sizeof(SelectHead) + (size_t)out_cap * sizeof(PyrHit); }
inline PyrHit* select_entries(SelectHead* h) { return reinterpret_cast<PyrHit*>(h + 1); }

// Enqueues the whole selection on `stream`: init, kSelPasses x (hist, pick),
// compact. `upper` (>= n when known, else cap) sizes the grids. *launches
// (nullable): the kernels launched. Nothing is waited for.
hipError_t launch_list_select(const PyrHit* hits, const unsigned long long* n_dev, int64_t cap, int64_t upper,
                              const SelectSpec& spec, SelectState* state, SelectHead* out, int64_t out_cap,
                              hipStream_t stream, int* launches);

// --- the gated search's per-window reduction (PyramidSearch::gate) ----------
// Device state of a gated search: the head, then wkey[n_windows] (u64: the
// running maximum of select_key(score) over the window's leaves at or above
// the gate, raised by pyr_gate_kernel), then wflat[n_windows] (i64: the lowest
// global flat index among the list's entries whose key equals wkey[w];
// INT64_MAX: no entry, the window does not pass).
constexpr int kGateLevels = 11;  // kPyrMaxDepth + 1
#ifndef CSM_GATE_MUTATION  // the mutation builds of DESIGN 11 (1: plain store for the atomicMin, 2: a strict
#define CSM_GATE_MUTATION 0  // append test, 3: the keys not kept for the second descent); each must fail tests
#endif
struct GateHead {
  unsigned long long scored[kGateLevels];  // nodes bounded per depth by the last descent
  unsigned long long listed;               // entries the last descent appended (beyond the list's room too)
};
inline size_t gate_state_bytes(int64_t n_windows) { return sizeof(GateHead) + (size_t)n_windows * 16; }

// wflat = INT64_MAX; wkey = 0 unless keep_keys (a second descent keeps them).
hipError_t launch_gate_init(unsigned long long* wkey, long long* wflat, int64_t n_windows, bool keep_keys,
                            hipStream_t stream);
// gate_window_best_kernel over the list's first min(*n_dev, cap) entries
// (16-byte loads): an entry whose key equals wkey[flat / n_cand] lowers
// wflat[that window] to its flat (a 64-bit atomicMin). Copies scored[0,
// kGateLevels) and *n_dev into *head.
hipError_t launch_gate_window_best(const PyrHit* hits, const unsigned long long* n_dev, int64_t cap, int64_t n_cand,
                                   const unsigned long long* wkey, long long* wflat, const unsigned long long* scored,
                                   GateHead* head, hipStream_t stream);

}  // namespace csm
