// csm_grid_copies.hpp — the copies the scoring kernels read in place of the
// fixed-point grid (the palette index grid and its values, the pair kernel's
// strip copies of it, the maps of uniform boxes, the phase kernel's strip
// copies of gridi): the record that holds them, the key that says whether they
// are of the current grid, and the rules that say which are built and used,
// as pure host arithmetic (no HIP, no context). csm_grid.cpp builds the copies
// and turns them into LevelWork fields; tests/test_grid_copies.py compiles
// this header into a stand-alone program.
#pragma once
#include <cstdint>

namespace csmh {

// The pair kernel's palettes (csm::kPairMaxPal; csm_grid.cpp asserts they agree).
constexpr int32_t kStripsMaxPal = 16;

// The share of set bits in the map of uniform boxes below which the pair
// kernel does not read it. The read costs the same whatever it finds: with an
// empty map forced on, the headline step is 0.060 ms longer; with config 2's
// map (38 % of corners set) it is 0.149 ms shorter than that. Taking the gain
// as proportional to the share, the two meet at 0.38 * 0.060 / 0.149 = 0.15
// (profiles/background_runs/speed.md).
constexpr double kBgMinShare = 0.16;

// The pair kernel's strip copies of the palette grid are built: its palettes
// are small, and its strip offsets are 24-bit products (strips under 2^24 bytes).
inline bool pal_strips_built(bool pair_kernel, int32_t pal_n, int64_t grid_bytes, int64_t strip_bytes) {
  return pair_kernel && pal_n >= 1 && pal_n <= kStripsMaxPal && grid_bytes <= INT32_MAX && strip_bytes < (1 << 24);
}
// ... and with them the maps of uniform boxes (CSM_BG_RUNS=0: none): byte
// offsets and the corner's bit in one 32-bit key (maps under 2^28 bytes), the
// grid of a stack in 16 bits.
inline bool bg_maps_built(int bg_runs, int64_t map_bytes, int32_t n_grids) {
  return bg_runs != 0 && map_bytes < (1 << 28) && n_grids <= 65535;
}
// A built map is read: by its share of set bits, or forced (CSM_BG_RUNS >= 2).
inline bool bg_map_used(int bg_runs, double share) { return bg_runs >= 2 || share >= kBgMinShare; }
// The phase kernel's strip copies of gridi are built.
inline bool istrips_built(int64_t grid_bytes) { return grid_bytes <= INT32_MAX; }
// The phase kernel's strip form reads the map of 5 x 5 boxes, which is made
// from the palette's index grid: a phase level wants the palette built too.
inline bool phase_wants_palette(bool phase_strips, bool pair_kernel, int bg_runs) {
  return phase_strips && pair_kernel && bg_runs != 0;
}

// What a family of copies was built from: the grid generation (csm_ctx::grid_gen)
// and the fixed-point grid itself.
struct CopyKey {
  uint64_t gen = 0;
  const int32_t* src = nullptr;
  bool current(uint64_t g, const int32_t* s) const { return gen == g && src == s; }
};

// Everything the palette and strip builders produce (csm_grid.cpp
// ensure_palette, ensure_istrips), over the context's buffer type. The
// context's, not a grid's: swap_grid moves grid_gen on, so a grid switched
// back in rebuilds them.
template <class Buf>
struct GridCopiesOf {
  // the grid's palette: the byte copy of gridi (palette indices) and the
  // palette, rebuilt when grid_gen moves on (the pair box kernel's source)
  Buf pal_grid, pal_vals, pal_scratch;
  int32_t pal_n = 0;  // palette size (0: none, e.g. more than kPalMax values)
  Buf pal_strips;     // strip copies of pal_grid (v11 pair kernel; palettes of <= kPairMaxPal values)
  bool pal_strips_ok = false;
  // The pair kernel's map of uniform boxes (csm_palette.hip bg_geom), built
  // with the strips and keyed like them. bg_ok: the pair kernel uses it
  // (bg_map_used).
  Buf bg_map, bg_info;
  bool bg_ok = false;
  double bg_share = 0.0;  // set bits / corners of the current grid(s)
  // ... and the phase kernel's map of 5 x 5 boxes, built with it
  Buf bg_map5;
  bool bg5_ok = false;
  double bg5_share = 0.0;
  CopyKey pal_key;  // what all of the above were built from
  Buf istrips;      // strip copies of gridi (the phase kernel's strip form)
  bool istrips_ok = false;
  CopyKey istrips_key;

  // the pair kernel can run: a palette and its strips (after ensure_palette)
  bool pair_ok() const { return pal_n > 0 && pal_strips_ok; }
};

}  // namespace csmh
