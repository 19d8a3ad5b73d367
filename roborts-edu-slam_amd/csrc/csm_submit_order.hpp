// csm_submit_order.hpp — the order csm_scan_matchers_submit takes its steps
// in, and how many parts a submitted batch is cut into: pure functions of a
// few integers, no device and no context (tests/cpp/submit_order_check.cpp),
// like csm_level_decision.hpp.
//
// A submit of batch B with batch A pending (A's levels launched up to its last
// part's last hand-off, its completion owed) interleaves the two so that every
// wait of the host falls under a launch of the other batch:
//
//   two parts  B.begin(0) | A.last launches | B.begin(1) | A.finish | B's hand-offs
//   one part   B.begin(0) | A.last launches | B's first hand-off | A.finish | B's other hand-offs
//
// With two parts B's second part's coarse level covers A's completion and B's
// parts cover each other's hand-offs. With one part nothing of B would run
// while its coarse -> fine hand-off is planned, so that hand-off goes before
// A's completion: the device runs A's last level meanwhile, and A is completed
// while B's fine level scores. Either way the last part's last hand-off is
// left to the next submit when deferred (csm_ctx::defer_last_handoff).
#pragma once

namespace csmh {

// Level transition l -> l + 1 of part h is left to the next call (the last
// part's last one, when deferred).
constexpr bool handoff_deferred(int l, int h, int parts, int levels, bool defer) {
  return defer && l + 2 == levels && h == parts - 1;
}

enum class SubmitStep : unsigned char {
  kBegin,         // the new batch's part `part`: its first level planned and launched
  kHandoff,       // the new batch's part `part`: level `level` completed, level + 1 launched
  kPriorLast,     // the pending batch's deferred last hand-off (its last launch)
  kPriorFinish,   // the pending batch completed: its outputs are final
};

struct SubmitOp {
  SubmitStep step;
  int level, part;
  constexpr bool operator==(const SubmitOp& o) const { return step == o.step && level == o.level && part == o.part; }
};

constexpr int kSubmitMaxParts = 4;  // (csm_ctx::kMaxParts)
constexpr int kSubmitMaxLevels = 3;

struct SubmitOrder {
  SubmitOp op[kSubmitMaxParts * kSubmitMaxLevels + 2]{};
  int n = 0;
  constexpr void add(SubmitStep s, int level = 0, int part = 0) { op[n++] = SubmitOp{s, level, part}; }
};

// parts: the new batch's (1 .. kSubmitMaxParts); pending_parts: the pending
// batch's, 0 when nothing is pending; levels: the new batch's (1 ..
// kSubmitMaxLevels); defer: the new batch's last hand-off is left out (the
// pending batch's kPriorLast launches whatever that batch left, nothing when
// it deferred nothing).
constexpr SubmitOrder submit_order(int parts, int pending_parts, int levels, bool defer) {
  SubmitOrder o;
  o.add(SubmitStep::kBegin, 0, 0);
  if (pending_parts > 0) o.add(SubmitStep::kPriorLast);
  for (int h = 1; h < parts; ++h) o.add(SubmitStep::kBegin, 0, h);
  // one part: its first hand-off before the pending batch's completion
  const bool early_handoff = parts == 1 && levels > 1 && !handoff_deferred(0, 0, parts, levels, defer);
  if (early_handoff) o.add(SubmitStep::kHandoff, 0, 0);
  if (pending_parts > 0) o.add(SubmitStep::kPriorFinish);
  for (int l = 0; l + 1 < levels; ++l)
    for (int h = 0; h < parts; ++h) {
      if (handoff_deferred(l, h, parts, levels, defer) || (early_handoff && l == 0)) continue;
      o.add(SubmitStep::kHandoff, l, h);
    }
  return o;
}

// How many parts a submitted batch takes. forced: CSM_SUBMIT_PARTS (1 or 2; 0:
// by the rule); pipeline_parts_set: CSM_PIPELINE_PARTS was given, and wins
// over the rule; coarse_device_bound: the coarse level sums more than
// first_windows_submit_min_use beams, the line between device-bound and
// host-bound levels that also decides its spans (job_setup). One part only
// where a launch gives the device enough to run to cover the host.
constexpr int submit_parts(int forced, bool pipeline_parts_set, int pipeline_parts, bool coarse_device_bound) {
  if (forced == 1 || forced == 2) return forced;
  if (pipeline_parts_set || !coarse_device_bound) return pipeline_parts < 2 ? 2 : pipeline_parts;
  return 1;
}

}  // namespace csmh
