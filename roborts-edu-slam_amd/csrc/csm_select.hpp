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

}  // namespace csm
