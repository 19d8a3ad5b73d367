// csm_grid_copies.hpp — the copies the scoring kernels read in place of the
// fixed-point grid (the palette index grid and its values, the pair kernel's
// strip copies of it, the maps of uniform boxes, the phase kernel's strip
// copies of gridi): the record that holds them, the key that says whether they
// are of the current grid, the rules that say which are built and used, and
// the layouts' geometry (how large gridi and each copy are for a grid size),
// as pure host arithmetic (no HIP, no context). csm_grid.cpp builds the copies
// and turns them into LevelWork fields; tests/test_grid_copies.py and
// tests/test_grid_geom.py compile this header into stand-alone programs.
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

// ---- The layouts' geometry -------------------------------------------------
// How large gridi and each copy are, from the grid's size alone. The kernels
// that read them (csm_box.hip, csm_phase.hip, csm_tiny.hip) and the builders
// (csm_gridprep.hip, csm_palette.hip) all take their sizes from here;
// tests/cpp/grid_geom_check.cpp walks every read pattern the kernels document
// over a range of grid sizes and checks that none leaves these sizes.

// gridi layout: row pitch = round4(size_x + kGridiPadCols) cells, size_y +
// kGridiPadRows rows; every cell outside [0,size_x) x [0,size_y) is zero, so a
// 16 x 16 box whose corner lies on the grid never leaves the buffer.
constexpr int kGridiPadCols = 15;
constexpr int kGridiPadRows = 16;
constexpr int32_t gridi_pitch(int32_t sx) { return (sx + kGridiPadCols + 3) & ~3; }

// The pair kernel's strip copies of the palette index grid: kStripCopies
// copies, each kStripShift cells further along, in strips kStripW bytes wide
// (csm_internal.hpp says why).
constexpr int kStripW = 16;
#ifndef CSM_STRIP_COPIES
#define CSM_STRIP_COPIES 16
#endif
constexpr int kStripCopies = CSM_STRIP_COPIES;
constexpr int kStripShift = kStripW / kStripCopies;
static_assert(kStripCopies == 4 || kStripCopies == 16, "strip copies: 4 or 16");
constexpr int kStripPadRows = 16;  // zero rows below the grid (box rows and the zero run's rows)
constexpr int kStripPadLo = 16;    // columns and rows before the grid's first
struct StripGeom {
  int32_t rows, n_strips;
  int64_t strip_bytes, copy_bytes, grid_bytes;
};
inline StripGeom strip_geom(int size_x, int size_y) {
  StripGeom G{};
  G.rows = kStripPadLo + size_y + kStripPadRows;
  // a box row piece starts at (ix & ~(S - 1)) + S c <= kStripPadLo + size_x - 1 + 16 - S
  // in copy c (S = kStripShift, ix the padded column)
  G.n_strips = (kStripPadLo + size_x + 15 - kStripShift) / kStripW + 1;
  G.strip_bytes = (int64_t)G.rows * kStripW;
  G.copy_bytes = G.strip_bytes * G.n_strips;
  G.grid_bytes = G.copy_bytes * kStripCopies;
  return G;
}

// The maps of uniform boxes: one bit per padded box corner, 8 x 8 corners to a
// 64-bit word.
struct BgGeom {
  int32_t tiles_x, tiles_y;
  int64_t grid_bytes;
};
inline BgGeom bg_geom(int size_x, int size_y) {
  BgGeom G{};
  // corners 0 .. kStripPadLo + size - 1 per axis (the box test's in-grid range)
  G.tiles_x = (kStripPadLo + size_x + 7) / 8;
  G.tiles_y = (kStripPadLo + size_y + 7) / 8;
  G.grid_bytes = (int64_t)G.tiles_x * G.tiles_y * 8;
  return G;
}

// The phase kernel's strip copies of gridi: kIStripCopies copies, each 4 cells
// further along, in strips of kIStripCells cells.
constexpr int kIStripCells = 8;
constexpr int kIStripCopies = 2;
constexpr int kIStripPadRows = 16;
constexpr int kIStripPadLo = 16;
inline StripGeom istrip_geom(int size_x, int size_y) {
  StripGeom G{};
  G.rows = kIStripPadLo + size_y + kIStripPadRows;
  // a box row starts at cell (ix & ~3) + 4c <= kIStripPadLo + size_x - 1 + 4 in
  // copy c (ix the padded column), phase <= 3
  G.n_strips = (kIStripPadLo + size_x + 3) / kIStripCells + 1;
  G.strip_bytes = (int64_t)G.rows * kIStripCells * 4;
  G.copy_bytes = G.strip_bytes * G.n_strips;
  G.grid_bytes = G.copy_bytes * kIStripCopies;
  return G;
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
  // The pair kernel's map of uniform boxes (bg_geom above), built
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
