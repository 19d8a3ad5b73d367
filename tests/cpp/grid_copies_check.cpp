// grid_copies_check.cpp — the grid's derived copies (csrc/csm_grid_copies.hpp)
// without HIP: every rule on both sides of each threshold, the key that says
// whether a family of copies is of the current grid, and the record over the
// counting malloc / free policy of resources_check.cpp: moved and swapped
// whole, every buffer freed once, keys and outcomes travelling with the
// buffers. Stand-alone (tests/test_grid_copies.py builds and runs it, once
// more under ASan + UBSan).
#define CSM_RESOURCES_NO_HIP
#include "csm_grid_copies.hpp"
#include "csm_resources.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

namespace {

int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    ++g_checks;                                             \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_failed;                                           \
    }                                                       \
  } while (0)

using namespace csmh;

void rules() {
  const int64_t fits = INT32_MAX, k24 = (int64_t)1 << 24, k28 = (int64_t)1 << 28;
  // the pair kernel's strips: palettes of 1 .. 16 values
  for (int32_t n : {0, 1, 16, 17, 257}) CHECK(pal_strips_built(true, n, 1000, 100) == (n == 1 || n == 16));
  for (int32_t n : {0, 1, 16, 17, 257}) CHECK(!pal_strips_built(false, n, 1000, 100));
  CHECK(kStripsMaxPal == 16);
  // ... a strip under 2^24 bytes, the strip grid within INT32_MAX
  CHECK(pal_strips_built(true, 16, fits, k24 - 1) && !pal_strips_built(true, 16, fits, k24));
  CHECK(!pal_strips_built(true, 16, fits + 1, k24 - 1));
  // the maps: CSM_BG_RUNS != 0, under 2^28 bytes, at most 65535 grids
  for (int runs = 0; runs <= 3; ++runs) {
    CHECK(bg_maps_built(runs, k28 - 1, 65535) == (runs != 0));
    CHECK(!bg_maps_built(runs, k28, 1) && !bg_maps_built(runs, 1, 65536));
  }
  CHECK(bg_maps_built(1, 1, 1) && bg_maps_built(1, k28 - 1, 1) && bg_maps_built(1, 1, 65535));
  // a map is read by its share, or forced
  const double under = kBgMinShare - 1e-12;
  CHECK(kBgMinShare == 0.16 && under < kBgMinShare);
  for (int runs = 0; runs <= 3; ++runs) {
    CHECK(bg_map_used(runs, kBgMinShare));
    CHECK(bg_map_used(runs, under) == (runs >= 2));
    CHECK(bg_map_used(runs, 0.0) == (runs >= 2) && bg_map_used(runs, 1.0));
  }
  // the strips of gridi
  CHECK(istrips_built(0) && istrips_built(fits) && !istrips_built(fits + 1));
  // the phase kernel wants the palette: all eight combinations
  int wants = 0;
  for (int m = 0; m < 8; ++m) {
    const bool strips = m & 1, pair = m & 2, runs_on = m & 4;
    for (int runs : {0, 1, 2, 3}) {
      if ((runs != 0) != runs_on) continue;
      const bool w = phase_wants_palette(strips, pair, runs);
      CHECK(w == (strips && pair && runs_on));
      wants += w;
    }
  }
  CHECK(wants == 3);  // (true, true, 1 | 2 | 3)
}

void keys() {
  const int32_t a[2] = {0, 0};
  CopyKey k;
  CHECK(k.gen == 0 && k.src == nullptr);
  CHECK(k.current(0, nullptr));  // (the builders never ask without a grid)
  CHECK(!k.current(1, &a[0]));
  k = {7, &a[0]};
  CHECK(k.current(7, &a[0]));
  CHECK(!k.current(8, &a[0]));  // a generation step, the same grid
  CHECK(!k.current(6, &a[0]));
  CHECK(!k.current(7, &a[1]));  // another grid at the same generation
  CHECK(!k.current(7, nullptr));
  CHECK(!k.current(8, &a[1]));
  k = {8, &a[1]};
  CHECK(k.current(8, &a[1]) && !k.current(7, &a[0]));
}

// Every live allocation with its size; frees of anything else are counted
// (resources_check.cpp's policy).
struct CountingMem {
  using Status = int;
  static constexpr Status kOk = 0;
  static std::map<void*, size_t> live;
  static int allocs, frees, bad_frees;
  static Status alloc(void** p, size_t bytes) {
    *p = std::malloc(64);  // sizes are checked, not touched
    if (!*p) return 2;
    live[*p] = bytes;
    ++allocs;
    return kOk;
  }
  static void free(void* p) {
    auto it = live.find(p);
    if (it == live.end()) {
      ++bad_frees;  // a double free, or a pointer never handed out
      return;
    }
    live.erase(it);
    std::free(p);
    ++frees;
  }
  static bool balanced() { return live.empty() && allocs == frees && bad_frees == 0; }
};
std::map<void*, size_t> CountingMem::live;
int CountingMem::allocs = 0, CountingMem::frees = 0, CountingMem::bad_frees = 0;

using Buf = Buffer<CountingMem>;
using Copies = GridCopiesOf<Buf>;
static_assert(kMoveOnly<Copies>, "the grid's copies are exchanged, never copied");
constexpr int kBufs = 8;

Buf* bufs(Copies& c, int i) {
  Buf* all[kBufs] = {&c.pal_grid, &c.pal_vals, &c.pal_scratch, &c.pal_strips,
                     &c.bg_map,   &c.bg_map5,  &c.bg_info,     &c.istrips};
  return all[i];
}

// What ensure_palette and ensure_istrips leave for a grid of `cells` cells.
Copies build(size_t cells, int32_t pal_n, uint64_t gen, const int32_t* src) {
  Copies c;
  for (int i = 0; i < kBufs; ++i) CHECK(bufs(c, i)->ensure(cells * (size_t)(i + 1)) == 0);
  c.pal_n = pal_n;
  c.pal_strips_ok = pal_strips_built(true, pal_n, 1000, 100);
  c.bg_share = 0.25 * pal_n;
  c.bg5_share = pal_n / 64.0;
  c.bg_ok = bg_map_used(1, c.bg_share);
  c.bg5_ok = bg_map_used(1, c.bg5_share);
  c.istrips_ok = true;
  c.pal_key = {gen, src};
  c.istrips_key = {gen + 1, src};
  return c;
}

bool is_a(const Copies& c, void* const p[kBufs], const int32_t* src) {
  bool ok = c.pal_n == 3 && c.pal_strips_ok && c.pair_ok() && c.bg_ok && !c.bg5_ok && c.bg_share == 0.75 &&
            c.bg5_share == 3 / 64.0 && c.istrips_ok && c.pal_key.current(5, src) && c.istrips_key.current(6, src);
  for (int i = 0; i < kBufs; ++i) ok = ok && bufs(const_cast<Copies&>(c), i)->p == p[i];
  return ok;
}

bool is_empty(const Copies& c) {
  bool ok = c.pal_n == 0 && !c.pal_strips_ok && !c.pair_ok() && !c.bg_ok && !c.bg5_ok && c.bg_share == 0.0 &&
            c.bg5_share == 0.0 && !c.istrips_ok && c.pal_key.current(0, nullptr) && c.istrips_key.current(0, nullptr);
  for (int i = 0; i < kBufs; ++i) ok = ok && bufs(const_cast<Copies&>(c), i)->p == nullptr;
  return ok;
}

void record() {
  const int32_t ga[1] = {0}, gb[1] = {0};
  {
    Copies a = build(200000, 3, 5, ga);
    CHECK(CountingMem::live.size() == kBufs);
    void* pa[kBufs];
    for (int i = 0; i < kBufs; ++i) {
      pa[i] = bufs(a, i)->p;
      CHECK(CountingMem::live.count(pa[i]) == 1 && bufs(a, i)->cap == 200000 * (size_t)(i + 1));
    }
    CHECK(is_a(a, pa, ga));
    Copies b(std::move(a));  // move construction: everything travels, the source is empty
    CHECK(is_a(b, pa, ga) && CountingMem::frees == 0);
    for (int i = 0; i < kBufs; ++i) CHECK(bufs(a, i)->p == nullptr && bufs(a, i)->cap == 0);
    Copies c = build(70000, 40, 9, gb);  // no strips, no maps in use
    CHECK(!c.pal_strips_ok && !c.pair_ok() && c.pal_n == 40 && CountingMem::live.size() == 2 * kBufs);
    void* pc[kBufs];
    for (int i = 0; i < kBufs; ++i) pc[i] = bufs(c, i)->p;
    std::swap(b, c);  // nothing freed, both exchanged whole
    CHECK(CountingMem::frees == 0 && is_a(c, pa, ga));
    CHECK(b.pal_n == 40 && b.pal_key.current(9, gb) && b.istrips_key.current(10, gb) && !b.pal_key.current(5, ga));
    for (int i = 0; i < kBufs; ++i) CHECK(bufs(b, i)->p == pc[i]);
    b = std::move(c);  // move assignment frees what the target held, once each
    CHECK(CountingMem::frees == kBufs && CountingMem::live.size() == kBufs && is_a(b, pa, ga));
    for (int i = 0; i < kBufs; ++i) CHECK(CountingMem::live.count(pc[i]) == 0);
    Copies& self = b;
    b = std::move(self);  // onto itself: kept
    CHECK(is_a(b, pa, ga) && CountingMem::frees == kBufs);
    b = Copies();  // an empty value assigned over it: all eight freed, outcomes and keys reset
    CHECK(CountingMem::frees == 2 * kBufs && CountingMem::live.empty() && is_empty(b));
    Copies d = build(100, 16, 1, ga);  // freed by its destructor
    CHECK(d.pair_ok() && CountingMem::live.size() == kBufs);
  }
  CHECK(CountingMem::balanced() && CountingMem::allocs == 3 * kBufs);
}

}  // namespace

int main() {
  rules();
  keys();
  record();
  std::printf("checks=%d allocs=%d frees=%d bad_frees=%d live=%zu failed=%d\n", g_checks, CountingMem::allocs,
              CountingMem::frees, CountingMem::bad_frees, CountingMem::live.size(), g_failed);
  if (g_failed || !CountingMem::balanced()) return 1;
  std::printf("grid_copies_check ok\n");
  return 0;
}
