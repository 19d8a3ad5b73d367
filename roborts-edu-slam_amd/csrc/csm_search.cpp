// csm_search.cpp — host driver of the admissible multi-resolution search
// (csm_pyramid.hpp). The host walks the resolution levels; the device bounds
// every node of a level in one launch and compacts the survivors' children.
//
//   top depth D: every (window, angle, J, K) node, bounded on level D
//   probe: the best node's 4^d leaves are scored exactly, raising the
//          incumbent before the level is pruned (the first probe at the top
//          usually finds the answer; later ones tighten it)
//   expand: children of the nodes whose bound is not below the incumbent
//   depth 0: exact candidate scores, folded into the incumbent
//
// A level's child list is bounded by the node capacity: a parent list larger
// than capacity / 4 is expanded in slices, each descended before the next
// (depth-first over slices, level-synchronous inside one), so memory stays
// fixed whatever the pruning rate.
#include "csm_pyramid.hpp"
#include "csm_resources.hpp"
#include "csm_select.hpp"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace csm {

namespace {

// every buffer here is sized exactly (ensure_exact): the levels are gigabytes
using csmh::DevBuf;

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct PyramidSearch::Impl {
  // pooled levels 1..kPyrMaxDepth of the current fixed-point grid
  DevBuf level[kPyrMaxDepth + 1];
  PyrGrid lev[kPyrMaxDepth + 1]{};
  const void* key_g = nullptr;
  uint64_t key_gen = 0;
  int32_t key_sx = -1, key_sy = -1, key_grids = -1, built = 0;
  // the top level's box copy (pyr_topbox_kernel): depth and pieces it was built for
  DevBuf box;
  PyrGrid boxg{};
  int32_t box_depth = -1, box_npc = 0;
  // per-depth node lists, their values and counts (counts[d]: nodes[d]'s
  // length as the expand that filled it left it)
  DevBuf nodes[kPyrMaxDepth + 1], vals[kPyrMaxDepth + 1];
  DevBuf partials, probe_slot, probe_nodes, probe_vals;
  // device state of a search, set by one init launch: the incumbent, the
  // nodes scored per depth, and a pool of list counters (each expand appends
  // to a fresh, already zero counter: no memset per level). Once the fresh
  // slots are used up (many slices), list d counts in a slot of its own,
  // kCountPool + d, cleared before each expand into it: never the slot of the
  // parent list (depth d + 1) whose count that expand reads.
  static constexpr int kCountPool = 64;
  static constexpr int kCountSlots = kCountPool + kPyrMaxDepth + 1;
  DevBuf state;  // BestPartial inc | scored[kPyrMaxDepth + 1] | pool[kCountSlots] | the collect's hit count
  int cslot[kPyrMaxDepth + 1] = {};  // pool slot of list d's count (slot 0: never written, zero)
  int next_slot = 1;
  BestPartial* inc_dev() const { return (BestPartial*)state.p; }
  unsigned long long* scored_dev() const { return (unsigned long long*)((char*)state.p + sizeof(BestPartial)); }
  unsigned long long* pool_dev() const { return scored_dev() + kPyrMaxDepth + 1; }
  unsigned long long* hits_dev() const { return pool_dev() + kCountSlots; }
  static constexpr int kStateWords = kPyrMaxDepth + 1 + kCountSlots + 1;  // what a search's init launch zeroes
  // collect mode (PyramidSearch::collect): the incumbent is the threshold and
  // is never merged, no probe runs, depth 0 appends its leaves to `hits`
  bool collecting = false;
  double collect_T = 0.0;
  int64_t hit_cap = 0;
  DevBuf hits;
  csmh::HostBuf h_hits;
  // the gated search (PyramidSearch::gate): collect mode over every window,
  // depth 0 raising per-window keys (launch_pyr_gate); its device state
  // (GateHead | wkey | wflat, csm_select.hpp) and the pinned copy of it
  bool gating = false;
  DevBuf gate_state;
  csmh::HostBuf h_gate;
  csm::GateHead* gate_head() const { return (csm::GateHead*)gate_state.p; }
  unsigned long long* wkey_dev() const { return (unsigned long long*)(gate_head() + 1); }
  long long* wflat_dev(int64_t n_windows) const { return (long long*)(wkey_dev() + n_windows); }
  // the selection over the list (csm_select.hpp): its state, its output
  // (count, then entries) and the pinned copy of that output
  DevBuf sel_state, sel_out;
  csmh::HostBuf h_sel;
  // the beam-box top level: integer sums of the implicit node list
  DevBuf top_sums, top_thr, top_slab;
  int top_implicit = -1;  // its depth while a search runs (-1: the top is a node list)
  int32_t top_nj = 0;
  // pinned: two counts read back, then the state's incumbent and scored
  // counts (pageable copies wait for the device: ~20-70 us each)
  csmh::HostBuf h_words;
  unsigned long long* h_counts() const { return h_words.as<unsigned long long>(); }
  BestPartial* h_inc() const { return (BestPartial*)(h_counts() + 2); }
  unsigned long long* h_scored() const { return (unsigned long long*)(h_inc() + 1); }
  csmh::Event ev_top[2];  // PyrInputs::timed
  // PyrInputs::timed: an event pair around each bound launch (depth, pair)
  static constexpr int kBoundEvents = 256;
  std::vector<csmh::Event> ev_bound;
  std::vector<int> ev_bound_depth;
  int n_ev_bound = 0;
  int64_t cap = (int64_t)1 << 25;
  // per level: the capacity of its node list, min(cap, the nodes the level
  // has at all), and that count; a level whose children always fit its list
  // is descended without reading a count back (no host round trip)
  int64_t capd[kPyrMaxDepth + 1] = {};
  int64_t possible[kPyrMaxDepth + 1] = {};
  void set_caps(const LevelWork& L, int D) {
    for (int d = 0; d <= D; ++d) {
      const double nj = (double)(((int64_t)L.n_space + (1 << d) - 1) >> d);
      const double all = (double)L.n_scans * (double)L.n_angles * nj * nj;
      possible[d] = all >= 9.0e18 ? INT64_MAX / 8 : (int64_t)all;
      capd[d] = std::max<int64_t>(4, std::min(cap, possible[d]));
    }
  }
  int probe_min = 4096;
  bool probes = true;  // false: no probe at any level, the top included (a test hook)
  static constexpr int kRoots = 8;  // probe roots per probe (best partials of distinct blocks)
  PyrInputs in{};
  PyrStats* st = nullptr;

  hipError_t mark_top(int i, hipStream_t stream) {
    hipError_t e;
    if ((e = ev_top[i].create(hipEventDefault)) != hipSuccess) return e;
    return hipEventRecord(ev_top[i], stream);
  }

  hipError_t build(const PyrInputs& x) {
    const int32_t sx = x.level0.width, sy = x.level0.height;
    if (key_g != x.level0.g || key_gen != x.grid_gen || key_sx != sx || key_sy != sy || key_grids != x.n_grids) {
      built = 0;
      box_depth = -1;
      key_g = x.level0.g;
      key_gen = x.grid_gen;
      key_sx = sx;
      key_sy = sy;
      key_grids = x.n_grids;
    }
    lev[0] = x.level0;
    if (built >= x.depth) return hipSuccess;
    const double t0 = now_ms();
    hipError_t e;
    for (int d = built + 1; d <= x.depth; ++d) {
      PyrGrid& L = lev[d];
      L.shift = 1 << d;
      L.width = sx + L.shift;
      L.height = sy + L.shift;
      L.lg = d;
      L.q = (L.width + L.shift - 1) >> d;
      L.pitch = ((L.q << d) + 3) & ~3;
      L.stride = (int64_t)L.pitch * L.height;
      L.qs = kPyrQuant;
      if ((e = level[d].ensure_exact((size_t)L.stride * (size_t)x.n_grids * sizeof(int16_t))) != hipSuccess) return e;
      L.g = level[d].p;
      if ((e = launch_pyr_pool(lev[d - 1], L, d, x.n_grids, x.stream)) != hipSuccess) return e;
    }
    if ((e = hipStreamSynchronize(x.stream)) != hipSuccess) return e;
    built = x.depth;
    if (st) st->build_ms = now_ms() - t0;
    return hipSuccess;
  }

  // Level D copied into the box layout (after build(x)): columns of each
  // phase padded by 8 * npc zeros, 2^D * nj zero rows below.
  hipError_t build_box(const PyrInputs& x, int D, int32_t nj, int npc) {
    if (box_depth == D && box_npc == npc &&
        boxg.height + (nj << D) <= (int32_t)(boxg.stride / boxg.pitch))
      return hipSuccess;
    const PyrGrid& src = lev[D];
    PyrGrid b = src;
    b.q = src.q + 8 * npc;
    b.pitch = b.q << D;
    const int64_t rows = (int64_t)src.height + ((int64_t)nj << D);
    b.stride = (int64_t)b.pitch * rows;
    if (b.stride * 2 >= INT32_MAX) return hipErrorInvalidValue;
    hipError_t e;
    const double t0 = now_ms();
    if ((e = box.ensure_exact((size_t)b.stride * (size_t)x.n_grids * sizeof(int16_t))) != hipSuccess) return e;
    b.g = box.p;
    if ((e = launch_pyr_widen(src, b, x.n_grids, x.stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(x.stream)) != hipSuccess) return e;
    boxg = b;
    box_depth = D;
    box_npc = npc;
    if (st) st->build_ms += now_ms() - t0;
    return hipSuccess;
  }

  // The top level may run as beam boxes (whatever top_mode asks): one-cell
  // steps are given; the box test needs |t| < 2^24 (box_ok), nj <= 32, a
  // launch of n_scans * n_angles waves.
  static bool box_eligible(const PyrInputs& x, int64_t nj, int64_t n_top) {
    const int64_t box_blocks = (int64_t)x.L.n_scans * x.L.n_angles;
    return x.depth > 0 && x.box_ok && x.one_scan && pyr_topbox_pieces((int32_t)nj) > 0 && box_blocks <= INT32_MAX &&
           n_top <= ((int64_t)1 << 28) && x.n_used >= 1 && x.n_used <= 4096;
  }
  // ints of the split waves' partial sums (launch_pyr_topbox's rule: only
  // launches of few (window, angle)s split)
  static size_t box_slab_ints(const PyrInputs& x, int64_t n_top) {
    return (int64_t)x.L.n_scans * x.L.n_angles < 4096 ? (size_t)n_top * kPyrTopMaxSplit : 0;
  }

  // csm_search_bounds' own buffers (a search's lists stay as it left them)
  DevBuf hook_nodes, hook_vals, hook_sums, hook_slab, hook_partials;

  hipError_t ensure_lists(int D) {
    hipError_t e;
    for (int d = 0; d <= D; ++d) {
      if ((e = nodes[d].ensure_exact((size_t)capd[d] * sizeof(uint64_t))) != hipSuccess) return e;
      if ((e = vals[d].ensure_exact((size_t)capd[d] * sizeof(double))) != hipSuccess) return e;
    }
    const int64_t np = ((int64_t)1 << (2 * D)) * kRoots;
    if ((e = partials.ensure_exact((size_t)pyr_blocks(INT64_MAX / 2) * sizeof(PyrPartial))) != hipSuccess) return e;
    if ((e = state.ensure_exact(sizeof(BestPartial) + kStateWords * sizeof(unsigned long long))) != hipSuccess) return e;
    if ((e = probe_slot.ensure_exact(kRoots * sizeof(uint64_t))) != hipSuccess) return e;
    if ((e = probe_nodes.ensure_exact((size_t)np * sizeof(uint64_t))) != hipSuccess) return e;
    if ((e = probe_vals.ensure_exact((size_t)np * sizeof(double))) != hipSuccess) return e;
    if ((e = h_words.ensure_exact((2 + kPyrMaxDepth + 1) * sizeof(unsigned long long) + sizeof(BestPartial))) !=
        hipSuccess)
      return e;
    return hipSuccess;
  }

  unsigned long long* count_dev(int d) { return pool_dev() + cslot[d]; }

  // nodes (n on the host, or *n_dev), at most `upper` of them
  hipError_t bound(int d, const uint64_t* list, double* out, int64_t n, const unsigned long long* n_dev,
                   int64_t upper) {
    const bool timed = in.timed && n_ev_bound < kBoundEvents;
    hipError_t e;
    if (timed) {
      if (ev_bound.size() < (size_t)2 * kBoundEvents) ev_bound.resize((size_t)2 * kBoundEvents);
      ev_bound_depth.resize(kBoundEvents);
      for (int k = 0; k < 2; ++k)
        if ((e = ev_bound[2 * n_ev_bound + k].create(hipEventDefault)) != hipSuccess) return e;
      if ((e = hipEventRecord(ev_bound[2 * n_ev_bound], in.stream)) != hipSuccess) return e;
    }
    if ((e = launch_pyr_bound(in.L, lev[d], d, in.scans, in.angles, in.pts, in.n_used, in.step, list, n, n_dev, upper,
                              out, (PyrPartial*)partials.p, scored_dev() + d, in.stream)) != hipSuccess)
      return e;
    if (timed) {
      if ((e = hipEventRecord(ev_bound[2 * n_ev_bound + 1], in.stream)) != hipSuccess) return e;
      ev_bound_depth[(size_t)n_ev_bound++] = d;
    }
    return hipSuccess;
  }

  // Score the leaves of the best nodes of n_partials block partials exactly
  // (the incumbent only ever rises).
  hipError_t probe(int d, int64_t n_partials) {
    hipError_t e;
    if ((e = launch_pyr_final((const PyrPartial*)partials.p, n_partials, false, kRoots, inc_dev(),
                              (uint64_t*)probe_slot.p, in.stream)) != hipSuccess)
      return e;
    if ((e = launch_pyr_probe(d, kRoots, (const uint64_t*)probe_slot.p, (uint64_t*)probe_nodes.p, in.stream)) !=
        hipSuccess)
      return e;
    const int64_t np = ((int64_t)1 << (2 * d)) * kRoots;
    if ((e = launch_pyr_bound(in.L, lev[0], 0, in.scans, in.angles, in.pts, in.n_used, in.step,
                              (const uint64_t*)probe_nodes.p, np, nullptr, np, (double*)probe_vals.p,
                              (PyrPartial*)partials.p, nullptr, in.stream)) != hipSuccess)
      return e;
    if ((e = launch_pyr_final((const PyrPartial*)partials.p, pyr_bound_blocks(np, in.n_used), true, 0, inc_dev(), nullptr,
                              in.stream)) != hipSuccess)
      return e;
    st->probe_leaves += np;
    return hipSuccess;
  }

  // Children of nodes[d][s, s + k) (k on the host, or *n_dev) into nodes[d-1].
  hipError_t expand(int d, int64_t s, int64_t k, const unsigned long long* n_dev, int64_t upper) {
    hipError_t e;
    if (next_slot < kCountPool) {
      cslot[d - 1] = next_slot++;  // zeroed by the search's init launch
    } else {  // fresh slots used up (many slices): list d - 1's own slot, cleared each time
      cslot[d - 1] = kCountPool + (d - 1);
      if ((e = hipMemsetAsync(count_dev(d - 1), 0, sizeof(unsigned long long), in.stream)) != hipSuccess) return e;
    }
    st->slices += 1;
    if (d == top_implicit)
      return launch_pyr_expand_top(in.L, d, top_nj, boxg.qs, in.n_used, in.scans, (const int32_t*)top_sums.p, s, k,
                                   inc_dev(), (int64_t*)top_thr.p, (uint64_t*)nodes[d - 1].p,
                                   count_dev(d - 1), capd[d - 1], in.stream);
    return launch_pyr_expand(in.L, d, (const uint64_t*)nodes[d].p + s, (const double*)vals[d].p + s, k, n_dev, upper,
                             inc_dev(), (uint64_t*)nodes[d - 1].p, count_dev(d - 1), capd[d - 1],
                             in.stream);
  }

  // counts[d - 1] and counts[d] to the host
  hipError_t read_counts(int d) {
    hipError_t e;
    if ((e = hipMemcpyAsync(h_counts(), count_dev(d - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            in.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(h_counts() + 1, count_dev(d), sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            in.stream)) != hipSuccess)
      return e;
    st->syncs += 1;
    return hipStreamSynchronize(in.stream);
  }

  // nodes[d] holds n nodes (n >= 0 known on the host; n < 0: counts[d]),
  // at most `upper`: bound them and descend. The host reads a count back
  // only when 4 * upper children might not fit the next list.
  hipError_t level_pass(int d, int64_t n, int64_t upper, bool top) {
    hipError_t e;
    const unsigned long long* nd = n >= 0 ? nullptr : count_dev(d);
    if (collecting && gating && d == 0)  // the same leaves, through their windows' keys
      return launch_pyr_gate(in.L, lev[0], in.scans, in.angles, in.pts, in.n_used, in.step,
                             (const uint64_t*)nodes[0].p, n, nd, upper, collect_T, wkey_dev(), (PyrHit*)hits.p,
                             hits_dev(), hit_cap, scored_dev(), in.stream);
    if (collecting && d == 0)  // the leaves at or above the threshold, appended; nothing to fold
      return launch_pyr_collect(in.L, lev[0], in.scans, in.angles, in.pts, in.n_used, in.step,
                                (const uint64_t*)nodes[0].p, n, nd, upper, collect_T, (PyrHit*)hits.p, hits_dev(),
                                hit_cap, scored_dev(), in.stream);
    if ((e = bound(d, (const uint64_t*)nodes[d].p, (double*)vals[d].p, n, nd, upper)) != hipSuccess) return e;
    return descend(d, n, upper, top, pyr_bound_blocks(upper, in.n_used));
  }

  // nodes[d] and vals[d] are in place, the block bests in partials.
  hipError_t descend(int d, int64_t n, int64_t upper, bool top, int64_t n_partials) {
    hipError_t e;
    const unsigned long long* nd = n >= 0 ? nullptr : count_dev(d);
    if (d == 0)
      return launch_pyr_final((const PyrPartial*)partials.p, n_partials, true, 0, inc_dev(), nullptr,
                              in.stream);
    if (!collecting && probes && (top || n >= probe_min) && (e = probe(d, n_partials)) != hipSuccess) return e;
    const int64_t child_upper = std::min(4 * upper, possible[d - 1]);
    if (child_upper <= capd[d - 1]) {
      if ((e = expand(d, 0, n, nd, upper)) != hipSuccess) return e;
      return level_pass(d - 1, -1, child_upper, false);
    }
    // optimistic: expand everything, then look at the count
    if ((e = expand(d, 0, n, nd, upper)) != hipSuccess) return e;
    if ((e = read_counts(d)) != hipSuccess) return e;
    const int64_t m = (int64_t)h_counts()[0];
    if (n < 0) n = (int64_t)h_counts()[1];
    if (m <= capd[d - 1]) return m > 0 ? level_pass(d - 1, m, m, false) : hipSuccess;
    // overflow (children dropped): slices of capacity / 4 parents, each descended
    const int64_t slice = std::max<int64_t>(1, capd[d - 1] / 4);
    for (int64_t s = 0; s < n; s += slice) {
      const int64_t k = std::min(slice, n - s);
      if ((e = expand(d, s, k, nullptr, k)) != hipSuccess) return e;
      if ((e = level_pass(d - 1, -1, 4 * k, false)) != hipSuccess) return e;
    }
    return hipSuccess;
  }

  // A search's device state set (the incumbent at {start, INT64_MAX}), then
  // the top level at x.depth bounded -- as beam boxes, as one whole-level
  // launch or as node lists -- and descended. run and collect share it; what
  // differs is the start, the probes and depth 0 (collecting). *top_scored:
  // top nodes bounded outside the scored counters; *msg: what failed.
  hipError_t search_levels(const PyrInputs& x, double start, int64_t* top_scored, const char** msg) {
    hipError_t e;
    auto bad = [&](hipError_t err, const char* m) {
      *msg = m;
      return err;
    };
    const int64_t nj = ((int64_t)x.L.n_space + (1 << x.depth) - 1) >> x.depth;
    const int64_t n_top = (int64_t)x.L.n_scans * x.L.n_angles * nj * nj;
    set_caps(x.L, x.depth);
    if ((e = ensure_lists(x.depth)) != hipSuccess) return bad(e, "pyramid node lists");
    for (int d = 0; d <= kPyrMaxDepth; ++d) cslot[d] = 0;
    next_slot = 1;
    if ((e = launch_pyr_init(inc_dev(), scored_dev(), kStateWords, x.stream, start)) != hipSuccess)
      return bad(e, "pyr_init_kernel");
    int32_t ktiles, kt, col_blocks;
    const int top_blocks = pyr_top_blocks(x.L, (int32_t)nj, &ktiles, &kt, &col_blocks);
    const int D = x.depth;
    // the top level as beam boxes: one-cell steps are given; the box test
    // needs |t| < 2^24 (box_ok), nj <= 32, a launch of n_scans * n_angles waves
    const int npc = pyr_topbox_pieces((int32_t)nj);
    const int64_t box_blocks = (int64_t)x.L.n_scans * x.L.n_angles;
    const bool use_box = x.top_mode == 0 && box_eligible(x, nj, n_top);
    if (use_box && (e = build_box(x, D, (int32_t)nj, npc)) == hipSuccess) {
      // the split waves' partial sums: only launches of few (window, angle)s split
      const size_t slab_ints = box_slab_ints(x, n_top);
      if ((e = top_sums.ensure_exact((size_t)n_top * sizeof(int32_t))) != hipSuccess ||
          (e = top_thr.ensure_exact(2 * sizeof(int64_t))) != hipSuccess ||
          (slab_ints && (e = top_slab.ensure_exact(slab_ints * sizeof(int32_t))) != hipSuccess))
        return bad(e, "pyramid top level");
      if ((e = partials.ensure_exact((size_t)std::max<int64_t>(box_blocks, pyr_blocks(INT64_MAX / 2)) *
                                 sizeof(PyrPartial))) != hipSuccess)
        return bad(e, "pyramid partials");
      if (x.timed && (e = mark_top(0, x.stream)) != hipSuccess) return bad(e, "hipEventRecord");
      if ((e = launch_pyr_topbox(x.L, boxg, D, (int32_t)nj, x.scans, x.angles, x.pts, x.n_used, x.step,
                                 (int32_t*)top_sums.p, slab_ints ? (int32_t*)top_slab.p : nullptr,
                                 (PyrPartial*)partials.p, x.stream)) != hipSuccess)
        return bad(e, "pyr_topbox_kernel");
      if (x.timed) {
        if ((e = mark_top(1, x.stream)) != hipSuccess) return bad(e, "hipEventRecord");
        std::snprintf(st->top_name, sizeof(st->top_name), "pyr_topbox_kernel<%d,%d>", npc,
                      (int)((nj * npc + 63) / 64));
        st->top_bytes = (double)n_top * (double)x.n_used * 2.0;
      }
      *top_scored = n_top;
      st->top_box = 1;
      top_implicit = D;
      top_nj = (int32_t)nj;
      e = descend(D, n_top, n_top, true, box_blocks);
      top_implicit = -1;
      if (e != hipSuccess) return bad(e, "pyramid level pass");
    } else if (use_box && e != hipErrorInvalidValue) {
      return bad(e, "pyramid box level");
    } else if (D > 0 && top_blocks > 0 && n_top <= ((int64_t)1 << 28)) {
      // the whole top level in one launch (column layout), then descend
      if ((e = nodes[D].ensure_exact((size_t)n_top * sizeof(uint64_t))) != hipSuccess ||
          (e = vals[D].ensure_exact((size_t)n_top * sizeof(double))) != hipSuccess)
        return bad(e, "pyramid top level");
      if ((e = partials.ensure_exact((size_t)std::max<int64_t>(top_blocks, pyr_blocks(INT64_MAX / 2)) *
                                 sizeof(PyrPartial))) != hipSuccess)
        return bad(e, "pyramid partials");
      if ((e = launch_pyr_top_bound(x.L, lev[D], D, (int32_t)nj, x.scans, x.angles, x.pts, x.n_used, x.step,
                                    (uint64_t*)nodes[D].p, (double*)vals[D].p, (PyrPartial*)partials.p,
                                    x.stream)) != hipSuccess)
        return bad(e, "pyr_top_bound_kernel");
      *top_scored = n_top;
      if ((e = descend(D, n_top, n_top, true, top_blocks)) != hipSuccess) return bad(e, "pyramid level pass");
    } else {
      for (int64_t first = 0; first < n_top; first += capd[D]) {
        const int64_t m = std::min(capd[D], n_top - first);
        if ((e = launch_pyr_top(x.L, (int32_t)nj, first, m, (uint64_t*)nodes[D].p, x.stream)) != hipSuccess)
          return bad(e, "pyr_top_kernel");
        if ((e = level_pass(D, m, m, true)) != hipSuccess) return bad(e, "pyramid level pass");
      }
    }
    return hipSuccess;
  }
};

PyramidSearch::PyramidSearch() : p_(new Impl) {}
PyramidSearch::~PyramidSearch() { delete p_; }

void PyramidSearch::release() {
  delete p_;
  p_ = new Impl;
}

void PyramidSearch::configure(int64_t node_capacity, int probe_min_nodes) {
  p_->cap = node_capacity > 0 ? std::max<int64_t>(node_capacity, 4) : ((int64_t)1 << 25);
  p_->probe_min = probe_min_nodes > 0 ? probe_min_nodes : 4096;
  p_->probes = probe_min_nodes >= 0;
}

int64_t PyramidSearch::level_cells(int32_t sx, int32_t sy, int d) {
  const int32_t w = sx + (1 << d), h = sy + (1 << d);
  return (int64_t)((w + 3) & ~3) * h;
}

hipError_t PyramidSearch::run(const PyrInputs& x, BestPartial* best, PyrStats* stats, std::string* what) {
  Impl& I = *p_;
  PyrStats local;
  I.st = stats ? stats : &local;
  *I.st = PyrStats{};
  I.n_ev_bound = 0;
  I.st->depth = x.depth;
  I.in = x;
  hipError_t e;
  auto fail = [&](hipError_t err, const char* msg) {
    if (what) *what = msg;
    return err;
  };
  if (x.depth < 0 || x.depth > kPyrMaxDepth) return fail(hipErrorInvalidValue, "pyramid depth out of range");
  if ((e = I.build(x)) != hipSuccess) return fail(e, "pyramid levels");
  int64_t top_scored = 0;
  const char* msg = nullptr;
  if ((e = I.search_levels(x, -DBL_MAX, &top_scored, &msg)) != hipSuccess) return fail(e, msg);
  const int D = x.depth;
  // the incumbent and the scored counts, one copy
  if ((e = hipMemcpyAsync(I.h_inc(), I.state.p, sizeof(BestPartial) + (kPyrMaxDepth + 1) * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, x.stream)) != hipSuccess)
    return fail(e, "incumbent copy");
  if ((e = hipStreamSynchronize(x.stream)) != hipSuccess) return fail(e, "pyramid search");
  unsigned long long* h_scored = I.h_scored();
  *best = I.h_inc()[0];
  for (int d = 0; d <= kPyrMaxDepth; ++d) I.st->nodes[d] = (int64_t)h_scored[d];
  if (x.timed && I.st->top_name[0]) {
    float ms = 0.f;
    if ((e = hipEventElapsedTime(&ms, I.ev_top[0], I.ev_top[1])) != hipSuccess) return fail(e, "hipEventElapsedTime");
    I.st->top_ms = ms;
  }
  for (int k = 0; k < I.n_ev_bound; ++k) {
    float ms = 0.f;
    if ((e = hipEventElapsedTime(&ms, I.ev_bound[2 * k], I.ev_bound[2 * k + 1])) != hipSuccess)
      return fail(e, "hipEventElapsedTime");
    const int d = I.ev_bound_depth[(size_t)k];
    I.st->bound_ms[d] += ms;
    I.st->bound_launches[d] += 1;
  }
  I.n_ev_bound = 0;
  I.st->nodes[D] += top_scored;
  return hipSuccess;
}

hipError_t PyramidSearch::collect(const PyrInputs& x0, double T, int64_t capacity, PyrHit* hits, int64_t* n_found,
                                  PyrStats* stats, std::string* what) {
  if (!hits) {
    if (what) *what = "collect: one window, a capacity and a threshold";
    return hipErrorInvalidValue;
  }
  return collect_impl(x0, T, capacity, hits, n_found, stats, what);
}

hipError_t PyramidSearch::collect_device(const PyrInputs& x0, double T, int64_t capacity, int64_t* n_found,
                                         PyrStats* stats, std::string* what) {
  return collect_impl(x0, T, capacity, nullptr, n_found, stats, what);
}

// hits: the host copy of the list's first `capacity` slots (null: the list stays on the device)
hipError_t PyramidSearch::collect_impl(const PyrInputs& x0, double T, int64_t capacity, PyrHit* hits, int64_t* n_found,
                                       PyrStats* stats, std::string* what) {
  Impl& I = *p_;
  auto fail = [&](hipError_t err, const char* msg) {
    I.collecting = false;
    I.st = nullptr;
    if (what) *what = msg;
    return err;
  };
  if (x0.depth < 0 || x0.depth > kPyrMaxDepth || x0.L.n_scans != 1 || capacity < 1 || !n_found || !(T == T))
    return fail(hipErrorInvalidValue, "collect: one window, a capacity and a threshold");
  // the levels run built for this grid: nothing is built here
  if (I.key_g != x0.level0.g || I.key_gen != x0.grid_gen || I.key_sx != x0.level0.width ||
      I.key_sy != x0.level0.height || I.key_grids != x0.n_grids || I.built < x0.depth)
    return fail(hipErrorInvalidValue, "collect: the pooled levels of this grid are not built (run first)");
  PyrInputs x = x0;
  x.timed = 0;
  PyrStats local;
  I.st = &local;
  I.in = x;
  I.lev[0] = x.level0;
  I.collecting = true;
  I.collect_T = T;
  I.hit_cap = capacity;
  hipError_t e;
  if ((e = I.hits.ensure_exact((size_t)capacity * sizeof(PyrHit))) != hipSuccess ||
      (hits && (e = I.h_hits.ensure_exact((size_t)capacity * sizeof(PyrHit))) != hipSuccess)) {
    I.hit_cap = 0;
    return fail(e, "collect list");
  }
  int64_t top_scored = 0;
  const char* msg = nullptr;
  if ((e = I.search_levels(x, T, &top_scored, &msg)) != hipSuccess) return fail(e, msg);
  // the count, the scored counts and (for a host copy) the list's first `capacity` slots, one wait
  if ((e = hipMemcpyAsync(I.h_counts(), I.hits_dev(), sizeof(unsigned long long), hipMemcpyDeviceToHost, x.stream)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(I.h_scored(), I.scored_dev(), (kPyrMaxDepth + 1) * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, x.stream)) != hipSuccess ||
      (hits && (e = hipMemcpyAsync(I.h_hits.p, I.hits.p, (size_t)capacity * sizeof(PyrHit), hipMemcpyDeviceToHost,
                                   x.stream)) != hipSuccess) ||
      (e = hipStreamSynchronize(x.stream)) != hipSuccess)
    return fail(e, "collect copy");
  const int64_t n = (int64_t)I.h_counts()[0];
  *n_found = n;
  if (hits) std::memcpy(hits, I.h_hits.p, (size_t)std::min(n, capacity) * sizeof(PyrHit));
  if (stats) {
    for (int d = 0; d <= kPyrMaxDepth; ++d) stats->collect_nodes[d] = (int64_t)I.h_scored()[d];
    stats->collect_nodes[x.depth] += top_scored;
  }
  I.collecting = false;
  I.st = nullptr;
  return hipSuccess;
}

hipError_t PyramidSearch::gate(const PyrInputs& x0, double T, int64_t capacity, bool keep_keys, GateOut* out,
                               PyrStats* stats, std::string* what) {
  Impl& I = *p_;
  auto fail = [&](hipError_t err, const char* msg) {
    I.collecting = I.gating = false;
    I.st = nullptr;
    if (what) *what = msg;
    return err;
  };
  static_assert(kGateLevels == kPyrMaxDepth + 1, "GateHead holds one count per level");
  const int64_t nw = x0.L.n_scans;
  if (x0.depth < 0 || x0.depth > kPyrMaxDepth || nw < 1 || capacity < 1 || !out || !(T == T))
    return fail(hipErrorInvalidValue, "gate: windows, a capacity and a threshold");
  PyrInputs x = x0;
  x.timed = 0;
  PyrStats local;
  I.st = &local;  // build and build_box note their time there
  I.in = x;
  hipError_t e;
  if ((e = I.build(x)) != hipSuccess) return fail(e, "pyramid levels");
  const size_t bytes = gate_state_bytes(nw);
  // a descent that keeps the keys needs the state the last one left
  if (keep_keys && (!I.gate_state.p || I.gate_state.cap < bytes))
    return fail(hipErrorInvalidValue, "gate: no keys to keep");
  if ((e = I.gate_state.ensure_exact(bytes)) != hipSuccess || (e = I.h_gate.ensure_exact(bytes)) != hipSuccess)
    return fail(e, "gate state");
  if ((e = I.hits.ensure_exact((size_t)capacity * sizeof(PyrHit))) != hipSuccess) {
    I.hit_cap = 0;
    return fail(e, "gate list");
  }
  I.collecting = I.gating = true;
  I.collect_T = T;
  I.hit_cap = capacity;
  if ((e = launch_gate_init(I.wkey_dev(), I.wflat_dev(nw), nw, keep_keys && CSM_GATE_MUTATION != 3, x.stream)) !=
      hipSuccess)
    return fail(e, "gate_init_kernel");
  int64_t top_scored = 0;
  const char* msg = nullptr;
  if ((e = I.search_levels(x, T, &top_scored, &msg)) != hipSuccess) return fail(e, msg);
  if ((e = launch_gate_window_best((const PyrHit*)I.hits.p, I.hits_dev(), capacity, x.L.n_cand, I.wkey_dev(),
                                   I.wflat_dev(nw), I.scored_dev(), I.gate_head(), x.stream)) != hipSuccess)
    return fail(e, "gate_window_best_kernel");
  // the keys, the flats, the count and the scored counts: one copy, one wait
  if ((e = hipMemcpyAsync(I.h_gate.p, I.gate_state.p, bytes, hipMemcpyDeviceToHost, x.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(x.stream)) != hipSuccess)
    return fail(e, "gate copy");
  const GateHead* h = I.h_gate.as<GateHead>();
  out->wkey = (const uint64_t*)(h + 1);
  out->wflat = (const int64_t*)(out->wkey + nw);
  out->listed = (int64_t)h->listed;
  if (stats) {
    for (int d = 0; d <= kPyrMaxDepth; ++d) stats->collect_nodes[d] = (int64_t)h->scored[d];
    stats->collect_nodes[x.depth] += top_scored;
    stats->build_ms = local.build_ms;
    stats->depth = x.depth;
  }
  I.collecting = I.gating = false;
  I.st = nullptr;
  return hipSuccess;
}

int64_t PyramidSearch::list_capacity() const { return (int64_t)(p_->hits.cap / sizeof(PyrHit)); }

hipError_t PyramidSearch::select(const SelectSpec& spec, int64_t n_upper, PyrHit* out, int64_t out_cap, int64_t* n_out,
                                 int* launches, hipStream_t stream, std::string* what) {
  Impl& I = *p_;
  auto fail = [&](hipError_t err, const char* msg) {
    if (what) *what = msg;
    return err;
  };
  if (!I.hits.p || !I.state.p || I.hit_cap < 1 || out_cap < 0 || (out_cap > 0 && !out) || !n_out || spec.k < 1)
    return fail(hipErrorInvalidValue, "select: no device list, or no output");
  hipError_t e;
  const size_t bytes = select_out_bytes(out_cap);
  if ((e = I.sel_state.ensure_exact(sizeof(SelectState))) != hipSuccess ||
      (e = I.sel_out.ensure_exact(bytes)) != hipSuccess || (e = I.h_sel.ensure_exact(bytes)) != hipSuccess)
    return fail(e, "select buffers");
  if ((e = launch_list_select((const PyrHit*)I.hits.p, I.hits_dev(), I.hit_cap, std::max<int64_t>(n_upper, 1), spec,
                              (SelectState*)I.sel_state.p, (SelectHead*)I.sel_out.p, out_cap, stream, launches)) !=
      hipSuccess)
    return fail(e, "list select kernels");
  // the count and the compacted entries, one copy, one wait
  if ((e = hipMemcpyAsync(I.h_sel.p, I.sel_out.p, bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
      (e = hipStreamSynchronize(stream)) != hipSuccess)
    return fail(e, "select copy");
  SelectHead* h = I.h_sel.as<SelectHead>();
  *n_out = (int64_t)h->count;
  if (out_cap > 0) std::memcpy(out, select_entries(h), (size_t)std::min(*n_out, out_cap) * sizeof(PyrHit));
  return hipSuccess;
}

hipError_t PyramidSearch::fetch(int64_t n, PyrHit* out, hipStream_t stream, std::string* what) {
  Impl& I = *p_;
  auto fail = [&](hipError_t err, const char* msg) {
    if (what) *what = msg;
    return err;
  };
  if (n < 0 || n > I.hit_cap || !I.hits.p || (n > 0 && !out)) return fail(hipErrorInvalidValue, "fetch: beyond the device list");
  if (n == 0) return hipSuccess;
  hipError_t e;
  if ((e = I.h_hits.ensure_exact((size_t)n * sizeof(PyrHit))) != hipSuccess) return fail(e, "collect list");
  if ((e = hipMemcpyAsync(I.h_hits.p, I.hits.p, (size_t)n * sizeof(PyrHit), hipMemcpyDeviceToHost, stream)) != hipSuccess ||
      (e = hipStreamSynchronize(stream)) != hipSuccess)
    return fail(e, "collect copy");
  std::memcpy(out, I.h_hits.p, (size_t)n * sizeof(PyrHit));
  return hipSuccess;
}

hipError_t PyramidSearch::load_list(const PyrHit* hits, int64_t n, hipStream_t stream, std::string* what) {
  Impl& I = *p_;
  auto fail = [&](hipError_t err, const char* msg) {
    if (what) *what = msg;
    return err;
  };
  if (n < 0 || (n > 0 && !hits)) return fail(hipErrorInvalidValue, "load_list: no hits");
  const int64_t cap = std::max<int64_t>(n, 1);
  hipError_t e;
  if ((e = I.state.ensure_exact(sizeof(BestPartial) + Impl::kStateWords * sizeof(unsigned long long))) != hipSuccess ||
      (e = I.hits.ensure_exact((size_t)cap * sizeof(PyrHit))) != hipSuccess ||
      (e = I.h_hits.ensure_exact((size_t)cap * sizeof(PyrHit) + sizeof(unsigned long long))) != hipSuccess)
    return fail(e, "collect list");
  // pinned: the hits, then their count
  std::memcpy(I.h_hits.p, hits, (size_t)n * sizeof(PyrHit));
  unsigned long long* h_n = (unsigned long long*)((char*)I.h_hits.p + (size_t)cap * sizeof(PyrHit));
  *h_n = (unsigned long long)n;
  if ((n > 0 && (e = hipMemcpyAsync(I.hits.p, I.h_hits.p, (size_t)n * sizeof(PyrHit), hipMemcpyHostToDevice, stream)) !=
                    hipSuccess) ||
      (e = hipMemcpyAsync(I.hits_dev(), h_n, sizeof(unsigned long long), hipMemcpyHostToDevice, stream)) != hipSuccess ||
      (e = hipStreamSynchronize(stream)) != hipSuccess)
    return fail(e, "load_list copy");
  I.hit_cap = cap;
  return hipSuccess;
}

hipError_t PyramidSearch::top_bounds(const PyrInputs& x, int kernel, double* bounds, int64_t* sums, int64_t n_out,
                                     bool* unsupported, std::string* what) {
  Impl& I = *p_;
  PyrStats local;
  I.st = &local;  // build and build_box note their time there
  hipError_t e;
  // every return frees the hook's buffers (each hipFree waits for the device:
  // fine for a test hook), so a context's memory after the call is what a
  // search left it with
  auto done = [&](hipError_t err, const char* msg, bool unsup = false) {
    I.st = nullptr;
    I.hook_nodes.release();
    I.hook_vals.release();
    I.hook_sums.release();
    I.hook_slab.release();
    I.hook_partials.release();
    if (what && msg) *what = msg;
    if (unsupported) *unsupported = unsup;
    return err;
  };
  const int D = x.depth;
  if (D < 1 || D > kPyrMaxDepth || kernel < 0 || kernel > 2) return done(hipErrorInvalidValue, "depth or kernel out of range");
  const int64_t nj = ((int64_t)x.L.n_space + (1 << D) - 1) >> D;
  const int64_t n_top = (int64_t)x.L.n_scans * x.L.n_angles * nj * nj;
  if (n_out != n_top) return done(hipErrorInvalidValue, "n_out is not the top level's node count");
  if (n_top > ((int64_t)1 << 28)) return done(hipSuccess, "top level too large for one launch", true);
  if ((e = I.build(x)) != hipSuccess) return done(e, "pyramid levels");
  if (kernel == 0) {
    if (!Impl::box_eligible(x, nj, n_top)) return done(hipSuccess, "the box path does not take this input", true);
    const int npc = pyr_topbox_pieces((int32_t)nj);
    if ((e = I.build_box(x, D, (int32_t)nj, npc)) == hipErrorInvalidValue)
      return done(hipSuccess, "the box copy does not fit", true);
    if (e != hipSuccess) return done(e, "pyramid box level");
    const size_t slab_ints = Impl::box_slab_ints(x, n_top);
    if ((e = I.hook_sums.ensure_exact((size_t)n_top * sizeof(int32_t))) != hipSuccess ||
        (slab_ints && (e = I.hook_slab.ensure_exact(slab_ints * sizeof(int32_t))) != hipSuccess) ||
        (e = I.hook_partials.ensure_exact((size_t)x.L.n_scans * x.L.n_angles * sizeof(PyrPartial))) != hipSuccess)
      return done(e, "pyramid top level");
    if ((e = launch_pyr_topbox(x.L, I.boxg, D, (int32_t)nj, x.scans, x.angles, x.pts, x.n_used, x.step,
                               (int32_t*)I.hook_sums.p, slab_ints ? (int32_t*)I.hook_slab.p : nullptr,
                               (PyrPartial*)I.hook_partials.p, x.stream)) != hipSuccess)
      return done(e, "pyr_topbox_kernel");
    std::vector<int32_t> h((size_t)n_top);
    if ((e = hipMemcpyAsync(h.data(), I.hook_sums.p, (size_t)n_top * sizeof(int32_t), hipMemcpyDeviceToHost,
                            x.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(x.stream)) != hipSuccess)
      return done(e, "top sums copy");
    for (int64_t i = 0; i < n_top; ++i) sums[i] = h[(size_t)i];
    return done(hipSuccess, nullptr);
  }
  if ((e = I.hook_nodes.ensure_exact((size_t)n_top * sizeof(uint64_t))) != hipSuccess ||
      (e = I.hook_vals.ensure_exact((size_t)n_top * sizeof(double))) != hipSuccess)
    return done(e, "pyramid top level");
  if (kernel == 1) {
    int32_t ktiles, kt, col_blocks;
    const int top_blocks = pyr_top_blocks(x.L, (int32_t)nj, &ktiles, &kt, &col_blocks);
    if (top_blocks <= 0) return done(hipSuccess, "top level too large for one launch", true);
    if ((e = I.hook_partials.ensure_exact((size_t)top_blocks * sizeof(PyrPartial))) != hipSuccess)
      return done(e, "pyramid partials");
    if ((e = launch_pyr_top_bound(x.L, I.lev[D], D, (int32_t)nj, x.scans, x.angles, x.pts, x.n_used, x.step,
                                  (uint64_t*)I.hook_nodes.p, (double*)I.hook_vals.p, (PyrPartial*)I.hook_partials.p,
                                  x.stream)) != hipSuccess)
      return done(e, "pyr_top_bound_kernel");
  } else {
    if ((e = I.hook_partials.ensure_exact((size_t)pyr_bound_blocks(n_top, x.n_used) * sizeof(PyrPartial))) != hipSuccess)
      return done(e, "pyramid partials");
    if ((e = launch_pyr_top(x.L, (int32_t)nj, 0, n_top, (uint64_t*)I.hook_nodes.p, x.stream)) != hipSuccess)
      return done(e, "pyr_top_kernel");
    if ((e = launch_pyr_bound(x.L, I.lev[D], D, x.scans, x.angles, x.pts, x.n_used, x.step,
                              (const uint64_t*)I.hook_nodes.p, n_top, nullptr, n_top, (double*)I.hook_vals.p,
                              (PyrPartial*)I.hook_partials.p, nullptr, x.stream)) != hipSuccess)
      return done(e, "pyr_bound_kernel");
  }
  if ((e = hipMemcpyAsync(bounds, I.hook_vals.p, (size_t)n_top * sizeof(double), hipMemcpyDeviceToHost, x.stream)) !=
          hipSuccess ||
      (e = hipStreamSynchronize(x.stream)) != hipSuccess)
    return done(e, "top bounds copy");
  return done(hipSuccess, nullptr);
}

}  // namespace csm
