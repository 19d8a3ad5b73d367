// resources_check.cpp — ownership of csmh::Buffer (csrc/csm_resources.hpp)
// over a counting malloc / free policy, without HIP: what ensure and
// ensure_exact ask for, what a failed allocation leaves, and that moves, swaps
// and the eviction pattern free every allocation exactly once; and that the
// resident batch, exchanged whole through the submit sequence, keeps a pending
// job's offsets where its pointer reads them. Stand-alone
// (tests/test_resources.py builds and runs it, once more under ASan + UBSan).
#define CSM_RESOURCES_NO_HIP
#include "csm_resources.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

namespace {

int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

// Every live allocation with its size; frees of anything else are counted.
struct CountingMem {
  using Status = int;
  static constexpr Status kOk = 0;
  static std::map<void*, size_t> live;
  static std::vector<size_t> asked;  // every alloc call's size, failed ones included
  static int allocs, frees, bad_frees, fail_next, last_flags;
  static Status alloc(void** p, size_t bytes, int flags = 0) {
    asked.push_back(bytes);
    last_flags = flags;
    if (fail_next > 0) {
      --fail_next;
      *p = reinterpret_cast<void*>(0x1);  // a failed call may leave anything in *p
      return 2;
    }
    // sizes are checked, not touched: a small block stands for a large request
    *p = std::malloc(bytes < 64 ? bytes + 1 : 64);
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
std::vector<size_t> CountingMem::asked;
int CountingMem::allocs = 0, CountingMem::frees = 0, CountingMem::bad_frees = 0, CountingMem::fail_next = 0,
    CountingMem::last_flags = 0;

using Buf = csmh::Buffer<CountingMem>;
static_assert(csmh::kMoveOnly<Buf>, "Buffer has one owner");

// Stands in for GridState: several buffers plus scalars, defaulted moves.
struct Grid {
  Buf a, b;
  int sx = 0;
  const void* key = nullptr;
  bool has = false;
  uint64_t last_use = 0;
};
static_assert(csmh::kMoveOnly<Grid>, "a struct of buffers is exchanged, never copied");

Grid make_grid(int sx, size_t bytes, const void* key) {
  Grid g;
  CHECK(g.a.ensure(bytes) == 0 && g.b.ensure_exact(bytes / 2) == 0);
  g.sx = sx;
  g.key = key;
  g.has = true;
  g.last_use = (uint64_t)sx * 10;
  return g;
}

void sizes() {
  const size_t k64 = (size_t)64 << 10;
  CHECK(csm::grow_bytes(1, 0) == k64 && csm::grow_bytes(k64 + 1, 0) == k64 + 1);
  CHECK(csm::grow_bytes(100000, k64) == 100000 && csm::grow_bytes(70000, k64) == k64 + k64 / 2);
  CHECK(csm::grow_bytes(((size_t)1 << 30) + 1, (size_t)1 << 30) == ((size_t)1 << 30) + 1 + ((size_t)256 << 20));
  {
    Buf b;
    CHECK(b.p == nullptr && b.cap == 0);
    // above capacity: exactly grow_bytes(bytes, cap) each time
    size_t cap = 0;
    for (size_t bytes : {(size_t)1, (size_t)70000, (size_t)70001, (size_t)98304, (size_t)98305, (size_t)5 << 20}) {
      const size_t n0 = CountingMem::asked.size();
      const size_t want = bytes <= cap ? cap : csm::grow_bytes(bytes, cap);
      void* before = b.p;
      CHECK(b.ensure(bytes) == 0);
      if (bytes <= cap) {  // below capacity: no call, the same block
        CHECK(CountingMem::asked.size() == n0 && b.p == before && b.cap == cap);
      } else {
        CHECK(CountingMem::asked.size() == n0 + 1 && CountingMem::asked.back() == want && b.cap == want);
        CHECK(CountingMem::live.size() == 1 && CountingMem::live.count(b.p) == 1);  // the old block is gone
      }
      cap = b.cap;
    }
    CHECK(b.as<char>() == static_cast<char*>(b.p));
    // ensure_exact: exactly `bytes`, however large the buffer was
    const size_t n0 = CountingMem::asked.size();
    CHECK(b.ensure_exact(cap) == 0 && CountingMem::asked.size() == n0);
    CHECK(b.ensure_exact(cap + 8) == 0 && CountingMem::asked.back() == cap + 8 && b.cap == cap + 8);
    Buf e;
    CHECK(e.ensure_exact(8) == 0 && CountingMem::asked.back() == 8 && e.cap == 8);
    CHECK(e.ensure(9, 7) == 0 && CountingMem::asked.back() == k64 && CountingMem::last_flags == 7);  // flags pass through
    e.release();
    CHECK(e.p == nullptr && e.cap == 0);
    e.release();  // twice is nothing
  }
  CHECK(CountingMem::balanced());
}

void failures() {
  {
    Buf b;
    CountingMem::fail_next = 1;
    CHECK(b.ensure(100) != 0 && b.p == nullptr && b.cap == 0);
    CHECK(b.ensure(100) == 0 && b.cap == ((size_t)64 << 10));
    // a failed growth: the old block was freed, nothing is held
    CountingMem::fail_next = 1;
    CHECK(b.ensure_exact((size_t)1 << 20) != 0 && b.p == nullptr && b.cap == 0);
    CHECK(CountingMem::live.empty());
  }
  CHECK(CountingMem::balanced());
}

void moves() {
  {
    Buf a;
    CHECK(a.ensure(1000) == 0);
    void* pa = a.p;
    const size_t ca = a.cap;
    Buf b(std::move(a));  // move construction empties the source
    CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == ca);
    Buf c;
    CHECK(c.ensure_exact(24) == 0);
    void* pc = c.p;
    const int frees0 = CountingMem::frees;
    c = std::move(b);  // move assignment frees what the target held
    CHECK(CountingMem::frees == frees0 + 1 && CountingMem::live.count(pc) == 0);
    CHECK(c.p == pa && c.cap == ca && b.p == nullptr && b.cap == 0);
    Buf& self = c;
    c = std::move(self);  // onto itself: kept
    CHECK(c.p == pa && c.cap == ca && CountingMem::live.count(pa) == 1);
    Buf d;
    CHECK(d.ensure_exact(48) == 0);
    void* pd = d.p;
    const int frees1 = CountingMem::frees;
    std::swap(c, d);  // nothing freed, both exchanged
    CHECK(CountingMem::frees == frees1 && c.p == pd && c.cap == 48 && d.p == pa && d.cap == ca);
    Buf empty;
    std::swap(c, empty);
    CHECK(c.p == nullptr && empty.p == pd && CountingMem::live.size() == 2);
  }
  CHECK(CountingMem::balanced());
}

// swap_grid and select_grid's eviction: the current grid and three parked ones.
void eviction() {
  const int k1 = 0, k2 = 0, k3 = 0;  // their addresses are the keys
  {
    Grid cur = make_grid(1, 200000, &k1);
    Grid parked[3];
    parked[0] = make_grid(2, 300000, &k2);
    void* cur_a = cur.a.p;
    void* p0_b = parked[0].b.p;
    std::swap(cur, parked[0]);  // whole: buffers and scalars
    CHECK(cur.sx == 2 && cur.key == &k2 && cur.has && cur.last_use == 20 && cur.b.p == p0_b && cur.a.cap == 300000);
    CHECK(parked[0].sx == 1 && parked[0].key == &k1 && parked[0].last_use == 10 && parked[0].a.p == cur_a);
    CHECK(CountingMem::live.size() == 4);
    parked[1] = make_grid(3, 100, &k3);
    CHECK(CountingMem::live.size() == 6);
    // evict the least recently used slot: an empty value assigned over it
    const int frees0 = CountingMem::frees;
    parked[0] = Grid();
    CHECK(CountingMem::frees == frees0 + 2 && CountingMem::live.count(cur_a) == 0);
    CHECK(parked[0].a.p == nullptr && parked[0].b.p == nullptr && parked[0].sx == 0 && !parked[0].has &&
          parked[0].key == nullptr && parked[0].last_use == 0);
    std::swap(cur, parked[0]);  // the current grid parked, the empty slot current
    CHECK(!cur.has && cur.a.p == nullptr && parked[0].sx == 2 && parked[0].b.p == p0_b);
    parked[2] = Grid();  // over an empty slot: nothing to free
    CHECK(CountingMem::frees == frees0 + 2 && CountingMem::live.size() == 4);
    std::vector<Grid> v;  // reallocation moves (nothrow), never copies
    for (int i = 0; i < 5; ++i) v.push_back(make_grid(10 + i, 64, nullptr));
    CHECK(CountingMem::live.size() == 14 && v[0].sx == 10 && v[4].a.cap == ((size_t)64 << 10));
  }
  CHECK(CountingMem::balanced());
}

// Stands in for ScanBatch (csm_host.hpp): the points' buffer, the offsets, the
// per-scan grids, the scan count, the points' bound and the cache flag; and for
// the context, which is one and exchanges it whole (csm_ctx::swap_batch).
struct Batch {
  Buf pts;
  std::vector<int64_t> off;
  std::vector<int32_t> grid;
  int32_t n = -1;
  double maxabs = 0.0;
  bool cached = false;
};
static_assert(csmh::kMoveOnly<Batch>, "a batch is exchanged, never copied");

struct Ctx : Batch {
  void swap_batch(Batch& b) {
    std::swap(static_cast<Batch&>(*this), b);
    cached = b.cached = false;
  }
};

void fill_batch(Batch& b, std::vector<int64_t> off, double maxabs) {  // a load, or a queueing call into a slot
  CHECK(b.pts.ensure((size_t)off.back() * 16) == 0);
  b.off.assign(off.begin(), off.end());
  b.grid.clear();
  b.n = (int32_t)off.size() - 1;
  b.maxabs = maxabs;
}

// csm_scan_matchers_submit over queued batches: batch A loaded and submitted
// (its job reads A's offsets through a pointer), B queued and taken (A parks in
// B's slot), A borrowed back for its last hand-off and returned, C queued into
// the slot that holds A, C taken.
void submit_sequence() {
  const std::vector<int64_t> off_a = {0, 5000, 9000}, off_b = {0, 100, 300, 600, 7000}, off_c = {0, 40000};
  {
    Ctx cur;
    Batch slot[2];
    fill_batch(cur, off_a, 11.0);
    cur.grid = {1, 0};
    cur.cached = true;  // a synchronous load leaves the device buffer mirrored on the host
    const int64_t* job = cur.off.data();  // PipeJob::offsets of A's job
    void* pts_a = cur.pts.p;
    auto job_reads_a = [&] { return job[0] == off_a[0] && job[1] == off_a[1] && job[2] == off_a[2]; };

    fill_batch(slot[0], off_b, 22.0);
    void* pts_b = slot[0].pts.p;
    const int frees0 = CountingMem::frees;
    cur.swap_batch(slot[0]);  // take_staged: B current, A parked, whole
    CHECK(cur.n == 4 && cur.maxabs == 22.0 && cur.pts.p == pts_b && cur.off == off_b && cur.grid.empty());
    CHECK(slot[0].n == 2 && slot[0].maxabs == 11.0 && slot[0].pts.p == pts_a && slot[0].grid.size() == 2);
    CHECK(!cur.cached && !slot[0].cached);
    CHECK(slot[0].off.data() == job && job_reads_a());
    const int64_t* job_b = cur.off.data();

    cur.swap_batch(slot[0]);  // A's last hand-off: A borrowed back, every field its own
    CHECK(cur.n == 2 && cur.maxabs == 11.0 && cur.pts.p == pts_a && cur.off.data() == job && cur.grid.size() == 2);
    CHECK(slot[0].n == 4 && slot[0].pts.p == pts_b && slot[0].off.data() == job_b);
    CHECK(!cur.cached && !slot[0].cached && job_reads_a());
    cur.swap_batch(slot[0]);  // ... and returned
    CHECK(cur.n == 4 && cur.maxabs == 22.0 && cur.pts.p == pts_b && cur.off.data() == job_b);
    CHECK(slot[0].pts.p == pts_a && slot[0].off.data() == job && job_reads_a());
    CHECK(!cur.cached && !slot[0].cached);
    CHECK(CountingMem::frees == frees0 && CountingMem::live.size() == 2);  // swaps free nothing

    // A's job is complete: the next batch is queued into the slot that holds A (its points outgrow A's buffer)
    fill_batch(slot[0], off_c, 33.0);
    CHECK(CountingMem::frees == frees0 + 1 && CountingMem::live.size() == 2 && slot[0].pts.cap == 640000);
    void* pts_c = slot[0].pts.p;
    cur.swap_batch(slot[0]);  // C taken: B parks where A did
    CHECK(cur.n == 1 && cur.maxabs == 33.0 && cur.pts.p == pts_c && cur.off == off_c && cur.grid.empty());
    CHECK(slot[0].n == 4 && slot[0].pts.p == pts_b && slot[0].off.data() == job_b && slot[0].off == off_b);
    CHECK(!cur.cached && !slot[0].cached);
    CHECK(slot[1].pts.p == nullptr && slot[1].n == -1);
  }
  CHECK(CountingMem::balanced());
}

}  // namespace

int main() {
  sizes();
  failures();
  moves();
  eviction();
  submit_sequence();
  std::printf("allocs=%d frees=%d bad_frees=%d live=%zu failed=%d\n", CountingMem::allocs, CountingMem::frees,
              CountingMem::bad_frees, CountingMem::live.size(), g_failed);
  if (g_failed || !CountingMem::balanced()) return 1;
  std::printf("resources_check ok\n");
  return 0;
}
