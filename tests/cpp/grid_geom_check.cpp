// grid_geom_check.cpp — the layouts' geometry (csrc/csm_grid_copies.hpp:
// gridi_pitch, strip_geom, istrip_geom, bg_geom) against the read patterns the
// scoring kernels document, as pure host arithmetic: for every grid size of a
// range, every cell a pattern can touch lies inside the buffer the geometry
// sizes, coordinate by coordinate (column within the row, row within the
// rows, strip within the copy) and as a linear offset. No HIP, no GPU.
//
//   grid_geom_check [size_y size_x]...
//
// runs over every size_x, size_y in 1..80, 399..403, 1999..2003 and
// 2047..2049, then over the sizes given as arguments (the GPU tests' shapes),
// printing one line of geometry for each of those.
//
// The patterns restate the kernels' own guards; each says which. Column and
// row extents are independent in every layout (an offset is a function of the
// column plus a function of the row), so each size walks every column and
// every row once, not every pair.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "csm_grid_copies.hpp"

using namespace csmh;

static long long g_checks = 0, g_failed = 0;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      if (++g_failed <= 20) {                              \
        std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

// The box kernels over gridi or the palette's byte copy of it (same pitch):
// csm_box.hip BoxWave::offsets takes a corner with 0 <= ix0 < sx + pad and
// 0 <= iy0 < sy + pad (`in = live && clean && ix0 < sx + pad && iy0 < sy + pad`,
// pad = 0 here, ix0 = (int)tx with tx >= 0) at cell offset iy0 * pitch + ix0,
// and the layout's comment (csm_grid_copies.hpp, "a 16 x 16 box whose corner
// lies on the grid never leaves the buffer") gives the box: cells
// (ix0 + 0..15, iy0 + 0..15). The phase kernel's row-major form (csm_phase.hip
// classify, `use = live && ok && ix0 < sx + kPad && iy0 < sy + kPad`, 5 rows of
// two 16-byte pieces) reads a part of that box.
static void gridi_box(int sx, int sy) {
  const int32_t pitch = gridi_pitch(sx);
  const int64_t cells = (int64_t)pitch * (sy + kGridiPadRows);  // csm_host.hpp gridi_cells()
  int far_col = -1, far_row = -1;
  for (int ix0 = 0; ix0 < sx; ++ix0) far_col = std::max(far_col, ix0 + 15);
  for (int iy0 = 0; iy0 < sy; ++iy0) far_row = std::max(far_row, iy0 + 15);
  // within the row: a cell past size_x is the row's own zero pad, not the next row's column 0
  CHECK(far_col < pitch, "sx %d pitch %d column %d", sx, pitch, far_col);
  CHECK(far_row < sy + kGridiPadRows, "sy %d row %d", sy, far_row);
  CHECK((int64_t)far_row * pitch + far_col < cells, "sx %d sy %d", sx, sy);
  // the zero block of lanes that read nothing: csm_phase.hip `zero_off = sy * pitch4`
  // (row-major form), 5 rows of 8 cells from there
  CHECK((int64_t)(sy + 4) * pitch + 7 < cells, "sx %d sy %d", sx, sy);
}

// The tiny kernel (csm_tiny.hip: `gx_hi = pitch - 2, gy_hi = sy + kGridiPadRows - 2`,
// fast when 0 <= gx[0] <= gx_hi and 0 <= gy[0] <= gy_hi): two 8-byte loads, cells
// (gx0, gx0 + 1) of rows gy0 and gy0 + 1.
static void gridi_tiny(int sx, int sy) {
  const int32_t pitch = gridi_pitch(sx);
  const int64_t cells = (int64_t)pitch * (sy + kGridiPadRows);
  const int gx_hi = pitch - 2, gy_hi = sy + kGridiPadRows - 2;
  CHECK(gx_hi >= sx - 1 && gy_hi >= sy - 1, "sx %d sy %d: an on-grid beam leaves the fast path", sx, sy);
  CHECK(gx_hi + 1 < pitch && gy_hi + 1 < sy + kGridiPadRows, "sx %d sy %d", sx, sy);
  CHECK((int64_t)(gy_hi + 1) * pitch + gx_hi + 1 < cells, "sx %d sy %d", sx, sy);
}

// The pair kernel's strip copies (csm_box.hip BoxWave::offsets<STRIP>): padded
// corner 0 <= ix0 < sx + kStripPadLo, 0 <= iy0 < sy + kStripPadLo; copy
// `c = (-(ix0 >> LS)) & (kStripCopies - 1)`, piece start
// `xs = (ix0 & ~(S - 1)) + S * c` (strip_geom's comment: "a box row piece starts
// at (ix & ~(S - 1)) + S c"), byte offset
// c * copy_bytes + (xs >> 4) * strip_bytes + iy0 * 16 + (ix0 & (S - 1)); one
// aligned 16-byte piece per box row, and kStripPadRows = 16 rows from the
// corner ("box rows and the zero run's rows").
static void pair_strips(int sx, int sy) {
  constexpr int S = kStripShift, LS = S == 4 ? 2 : 0;
  const StripGeom G = strip_geom(sx, sy);
  int far_row = -1;
  for (int iy0 = 0; iy0 < sy + kStripPadLo; ++iy0) far_row = std::max(far_row, iy0 + 15);
  CHECK(far_row < G.rows, "sy %d row %d of %d", sy, far_row, G.rows);
  int far_strip = -1;
  for (int ix0 = 0; ix0 < sx + kStripPadLo; ++ix0) {
    const int c = (-(ix0 >> LS)) & (kStripCopies - 1);
    const int xs = (ix0 & ~(S - 1)) + S * c;
    const int t = xs >> 4, phase = ix0 & (S - 1);
    far_strip = std::max(far_strip, t);
    // the piece is one whole strip row, and the box's 13 cells from the phase lie in it
    CHECK((xs & 15) == 0 && phase + 13 <= kStripW, "sx %d ix0 %d xs %d", sx, ix0, xs);
    CHECK(t < G.n_strips, "sx %d ix0 %d copy %d strip %d of %d", sx, ix0, c, t, G.n_strips);
    const int64_t last = (int64_t)c * G.copy_bytes + (int64_t)t * G.strip_bytes + (int64_t)far_row * 16 + 15;
    CHECK(last < G.grid_bytes, "sx %d sy %d ix0 %d", sx, sy, ix0);
    // what the copy holds there is cell ix0 of the padded image: the builder
    // (csm_palette.hip pal_strips_kernel) writes x = 16 t + b - S c - kStripPadLo at byte b
    CHECK(16 * t + phase - S * c == ix0, "sx %d ix0 %d", sx, ix0);
  }
  // the geometry is not larger than the pattern needs
  CHECK(far_strip == G.n_strips - 1, "sx %d strips %d, the furthest read %d", sx, G.n_strips, far_strip);
  // the zero block (csm_box.hip: `zero_off = (kStripPadLo + L.size_y) * 16`, copy 0, strip 0), 16 rows
  CHECK((int64_t)(kStripPadLo + sy + 15) * 16 + 15 < G.strip_bytes, "sy %d", sy);
}

// The phase kernel's strip form (csm_phase.hip classify): padded corner
// 0 <= ix0 < sx + kIStripPadLo, 0 <= iy0 < sy + kIStripPadLo; copy
// `c = (ix0 >> 2) & 1`, `xs = (ix0 & ~3) + 4 * c` (istrip_geom's comment: "a
// box row starts at cell (ix & ~3) + 4c ... phase <= 3"), byte offset
// c * copy_bytes + (xs >> 3) * strip_bytes + iy0 * 32 + (ix0 & 3) * 4, plus the
// lane's `voff = cv * kRowB + ch * 16` for box row cv < 5 and piece ch < 2 of
// 16 bytes ("a box row's pieces stay within its strip row and the next").
static void phase_strips(int sx, int sy) {
  constexpr int kRowB = kIStripCells * 4, C = 5, NPC = (C + 3) / 4;
  const StripGeom G = istrip_geom(sx, sy);
  static_assert(3 + C <= kIStripCells, "the box's cells from any phase stay in the strip row");
  int far_row = -1;
  for (int iy0 = 0; iy0 < sy + kIStripPadLo; ++iy0) far_row = std::max(far_row, iy0 + C - 1);
  CHECK(far_row + 1 < G.rows, "sy %d row %d (and the next) of %d", sy, far_row, G.rows);
  int far_strip = -1;
  for (int ix0 = 0; ix0 < sx + kIStripPadLo; ++ix0) {
    const int c = (ix0 >> 2) & 1;
    const int xs = (ix0 & ~3) + 4 * c;
    const int t = xs >> 3, phase = ix0 & 3;
    far_strip = std::max(far_strip, t);
    CHECK((xs & 7) == 0, "sx %d ix0 %d xs %d", sx, ix0, xs);
    CHECK(t < G.n_strips, "sx %d ix0 %d copy %d strip %d of %d", sx, ix0, c, t, G.n_strips);
    // the furthest byte a lane loads: the last piece of the last box row, within the strip
    const int64_t in_strip = (int64_t)far_row * kRowB + phase * 4 + (NPC - 1) * 16 + 15;
    CHECK(in_strip < G.strip_bytes, "sx %d sy %d ix0 %d", sx, sy, ix0);
    CHECK((int64_t)c * G.copy_bytes + (int64_t)t * G.strip_bytes + in_strip < G.grid_bytes, "sx %d sy %d ix0 %d", sx,
          sy, ix0);
    // the builder (csm_palette.hip istrips_kernel) writes x = 8 t + b - 4 c - kIStripPadLo at cell b
    CHECK(8 * t + phase - 4 * c == ix0, "sx %d ix0 %d", sx, ix0);
  }
  CHECK(far_strip == G.n_strips - 1, "sx %d strips %d, the furthest read %d", sx, G.n_strips, far_strip);
  // the zero block (csm_phase.hip: `zero_off = (kPad + sy) * kRowB`, copy 0, strip 0)
  CHECK((int64_t)(kIStripPadLo + sy + C - 1) * kRowB + 12 + 16 + 15 < G.strip_bytes, "sy %d", sy);
}

// The maps of uniform boxes (bg_geom's comment: "corners 0 .. kStripPadLo +
// size - 1 per axis"; csm_box.hip offsets<.., BG> and csm_phase.hip classify:
// byte `(iy0 >> 3) * bg_tiles8 + (ix0 & ~7) + (iy0 & 7)`, bg_tiles8 = tiles_x * 8,
// bit ix0 & 7).
static void bg_maps(int sx, int sy) {
  const BgGeom G = bg_geom(sx, sy);
  const int tiles8 = G.tiles_x * 8;
  int64_t far_x = -1, far_y = -1;
  for (int ix0 = 0; ix0 < sx + kStripPadLo; ++ix0) {
    CHECK((ix0 >> 3) < G.tiles_x, "sx %d ix0 %d", sx, ix0);
    far_x = std::max<int64_t>(far_x, ix0 & ~7);
  }
  for (int iy0 = 0; iy0 < sy + kStripPadLo; ++iy0) {
    CHECK((iy0 >> 3) < G.tiles_y, "sy %d iy0 %d", sy, iy0);
    far_y = std::max<int64_t>(far_y, (int64_t)(iy0 >> 3) * tiles8 + (iy0 & 7));
  }
  CHECK(far_x + far_y < G.grid_bytes, "sx %d sy %d", sx, sy);
  CHECK(far_x + 8 == tiles8 && far_y / tiles8 == G.tiles_y - 1, "sx %d sy %d: tiles nobody reads", sx, sy);
}

static long long g_tight = 0;

// gridi_pitch(sx) >= sx + kGridiPadCols, with no spare column exactly when
// sx = 1 (mod 4): the tight pitch, where one column too far is the next row.
static void tight_pitch(int sx) {
  const int32_t pitch = gridi_pitch(sx);
  CHECK(pitch % 4 == 0, "sx %d pitch %d", sx, pitch);
  CHECK(pitch >= sx + kGridiPadCols, "sx %d pitch %d", sx, pitch);
  CHECK((pitch == sx + kGridiPadCols) == (sx % 4 == 1), "sx %d pitch %d", sx, pitch);
  CHECK(pitch - (sx + kGridiPadCols) <= 3, "sx %d pitch %d", sx, pitch);
  g_tight += pitch == sx + kGridiPadCols;
}

static void one_size(int sx, int sy) {
  gridi_box(sx, sy);
  gridi_tiny(sx, sy);
  pair_strips(sx, sy);
  phase_strips(sx, sy);
  bg_maps(sx, sy);
}

int main(int argc, char** argv) {
  std::vector<int> axis;
  for (int v = 1; v <= 80; ++v) axis.push_back(v);
  for (int v = 399; v <= 403; ++v) axis.push_back(v);
  for (int v = 1999; v <= 2003; ++v) axis.push_back(v);
  for (int v = 2047; v <= 2049; ++v) axis.push_back(v);
  for (int sx : axis) tight_pitch(sx);
  long long sizes = 0;
  for (int sy : axis)
    for (int sx : axis) {
      one_size(sx, sy);
      ++sizes;
    }
  if ((argc - 1) % 2 != 0) {
    std::printf("usage: grid_geom_check [size_y size_x]...\n");
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    const int sy = std::atoi(argv[i]), sx = std::atoi(argv[i + 1]);
    if (sx < 1 || sy < 1) {
      std::printf("bad size %s %s\n", argv[i], argv[i + 1]);
      return 2;
    }
    tight_pitch(sx);
    one_size(sx, sy);
    const StripGeom P = strip_geom(sx, sy), I = istrip_geom(sx, sy);
    const BgGeom B = bg_geom(sx, sy);
    std::printf("shape size_y=%d size_x=%d pitch=%d slack=%d strips=%d istrips=%d tiles_x=%d tiles_y=%d\n", sy, sx,
                gridi_pitch(sx), gridi_pitch(sx) - (sx + kGridiPadCols), P.n_strips, I.n_strips, B.tiles_x, B.tiles_y);
  }
  std::printf("sizes=%lld per_axis=%d tight_pitch=%lld checks=%lld failed=%lld\n", sizes, (int)axis.size(), g_tight,
              g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("grid_geom_check ok\n");
  return 0;
}
