// chain_plan_check.cpp — csrc/csm_chain_maps.hpp alone on the host, driven by
// tests/test_chain_plan_host.py (which holds the restatement).
//
//   (no argument)  a self-check of the rejected arguments; prints "chain_plan_check ok"
//   --plan         stdin, per case (every double as its 64 bits in hex):
//                    "resolution deviation offset size_x size_y use_blur default(float bits, hex)"
//                    "map_offset_x map_offset_y n_scans n_grids"
//                    n_scans lines "pt_begin n_points pose_x pose_y pose_theta"
//                    n_grids + 1 chain offsets, then the chain ids
//                  stdout per case: the status; when 0, "update_index max_points
//                  half_kernel n_ktab n_place", the table (float bits, hex), and
//                  per placement "pt_begin n_points grid c s tx ty" (hex)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "csm_chain_maps.hpp"

namespace {

uint64_t bits(double x) { return (uint64_t)__builtin_bit_cast(int64_t, x); }
double from_bits(uint64_t u) { return __builtin_bit_cast(double, u); }
uint32_t fbits(float x) { return (uint32_t)__builtin_bit_cast(int32_t, x); }

bool read_double(double* v) {
  uint64_t u;
  if (std::scanf("%" SCNx64, &u) != 1) return false;
  *v = from_bits(u);
  return true;
}

csm_chain_map_param good_param() {
  csm_chain_map_param mp{};
  mp.resolution = 0.08;
  mp.deviation = 0.24;
  mp.gaussian_blur_offset = 0.72;
  mp.size_x = 64;
  mp.size_y = 48;
  mp.use_blur = 1;
  mp.default_cell_prob = 0.3f;
  return mp;
}

int expect(const char* what, int got, int want, const std::string& err) {
  if (got == want && (want == CSM_OK || !err.empty())) return 0;
  std::printf("%s: status %d (wanted %d), text \"%s\"\n", what, got, want, err.c_str());
  return 1;
}

int self_check() {
  std::vector<csm::ChainScan> scans(3);
  for (int i = 0; i < 3; ++i) {
    scans[(size_t)i].pt_begin = 10 * i;
    scans[(size_t)i].n_points = 10;
  }
  const double mo[2] = {1.0, 2.0};
  const int32_t off[3] = {0, 2, 3}, ids[3] = {0, 2, 1};
  int bad = 0;
  const auto run = [&](const csm_chain_map_param& mp, int32_t n_grids, const int32_t* o, const int32_t* d,
                       std::string* err) {
    csm::ChainPlan plan;
    return csm::plan_chains(&mp, n_grids, o, d, mo, scans.data(), 3, &plan, err);
  };
  std::string err;
  csm_chain_map_param mp = good_param();
  bad += expect("good", run(mp, 2, off, ids, &err), CSM_OK, err);
  bad += expect("n_grids 0", run(mp, 0, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  bad += expect("n_grids -1", run(mp, -1, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  const int32_t down[3] = {0, 2, 1}, late[3] = {1, 2, 3};
  bad += expect("offsets decrease", run(mp, 2, down, ids, &err), CSM_ERR_INVALID_ARG, err);
  bad += expect("offsets start late", run(mp, 2, late, ids, &err), CSM_ERR_INVALID_ARG, err);
  const int32_t past[3] = {0, 3, 1}, neg[3] = {0, -1, 1};
  bad += expect("id past the store", run(mp, 2, off, past, &err), CSM_ERR_INVALID_ARG, err);
  bad += expect("negative id", run(mp, 2, off, neg, &err), CSM_ERR_INVALID_ARG, err);
  bad += expect("null ids", run(mp, 2, off, nullptr, &err), CSM_ERR_INVALID_ARG, err);
  mp = good_param();
  mp.size_x = 0;
  bad += expect("size_x 0", run(mp, 2, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  mp = good_param();
  mp.size_y = -4;
  bad += expect("size_y < 0", run(mp, 2, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  mp = good_param();
  mp.resolution = 0.0;
  bad += expect("resolution 0", run(mp, 2, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  mp.resolution = from_bits(0x7ff8000000000000ull);
  bad += expect("resolution NaN", run(mp, 2, off, ids, &err), CSM_ERR_INVALID_ARG, err);
  mp = good_param();
  mp.use_blur = 0;
  bad += expect("use_blur 0", run(mp, 2, off, ids, &err), CSM_ERR_UNSUPPORTED, err);
  if (err.find("use_blur") == std::string::npos) bad += expect("use_blur text", 0, 1, err);
  mp = good_param();
  mp.deviation = 0.04;  // = 0.5 resolution: not accepted (strict)
  bad += expect("deviation low", run(mp, 2, off, ids, &err), CSM_ERR_UNSUPPORTED, err);
  if (err.find("deviation") == std::string::npos) bad += expect("deviation text", 0, 1, err);
  mp.deviation = 0.8;  // = 10 resolution
  bad += expect("deviation high", run(mp, 2, off, ids, &err), CSM_ERR_UNSUPPORTED, err);
  // an invalid argument is reported before an unsupported mode
  mp.use_blur = 0;
  bad += expect("invalid before unsupported", run(mp, 2, off, past, &err), CSM_ERR_INVALID_ARG, err);
  // every chain empty: no ids needed
  mp = good_param();
  const int32_t none[3] = {0, 0, 0};
  bad += expect("empty chains", run(mp, 2, none, nullptr, &err), CSM_OK, err);
  if (bad) return 1;
  std::printf("chain_plan_check ok\n");
  return 0;
}

int plans() {
  for (;;) {
    csm_chain_map_param mp{};
    uint32_t dflt;
    if (!read_double(&mp.resolution)) return 0;
    if (!read_double(&mp.deviation) || !read_double(&mp.gaussian_blur_offset) ||
        std::scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNx32, &mp.size_x, &mp.size_y, &mp.use_blur, &dflt) != 4)
      return 2;
    mp.default_cell_prob = __builtin_bit_cast(float, dflt);
    double mo[2];
    int32_t n_scans, n_grids;
    if (!read_double(&mo[0]) || !read_double(&mo[1]) || std::scanf("%" SCNd32 " %" SCNd32, &n_scans, &n_grids) != 2 ||
        n_scans < 0 || n_grids < 0)
      return 2;
    std::vector<csm::ChainScan> scans((size_t)n_scans);
    for (auto& s : scans)
      if (std::scanf("%" SCNd64 " %" SCNd32, &s.pt_begin, &s.n_points) != 2 || !read_double(&s.pose[0]) ||
          !read_double(&s.pose[1]) || !read_double(&s.pose[2]))
        return 2;
    std::vector<int32_t> off((size_t)n_grids + 1);
    for (auto& o : off)
      if (std::scanf("%" SCNd32, &o) != 1) return 2;
    // the ids' count is the input's own: the offsets may be the invalid part
    int32_t n_ids;
    if (std::scanf("%" SCNd32, &n_ids) != 1 || n_ids < 0) return 2;
    std::vector<int32_t> ids((size_t)n_ids);
    for (auto& i : ids)
      if (std::scanf("%" SCNd32, &i) != 1) return 2;
    csm::ChainPlan plan;
    std::string err;
    const int st = csm::plan_chains(&mp, n_grids, off.data(), ids.empty() ? nullptr : ids.data(), mo, scans.data(),
                                    n_scans, &plan, &err);
    std::printf("%d\n", st);
    if (st != CSM_OK) continue;
    std::printf("%d %d %d %zu %zu\n", plan.update_index, plan.max_points, plan.half_kernel, plan.ktab.size(),
                plan.place.size());
    for (float v : plan.ktab) std::printf("%08" PRIx32 " ", fbits(v));
    std::printf("\n");
    for (const auto& p : plan.place)
      std::printf("%" PRId64 " %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", p.pt_begin,
                  p.n_points, p.grid, bits(p.c), bits(p.s), bits(p.tx), bits(p.ty));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return self_check();
  if (!std::strcmp(argv[1], "--plan")) return plans();
  std::printf("unknown mode %s\n", argv[1]);
  return 2;
}
