// submit_order_check.cpp — the order of a submit's steps
// (csrc/csm_submit_order.hpp) checked without a device, over every combination
// of 1 or 2 parts for the new and the pending batch (and none pending), 1 or 3
// levels, deferral on or off:
//   - every hand-off follows the launch of the level it completes (the part's
//     begin for level 0, its previous hand-off otherwise);
//   - exactly the hand-offs that are not deferred appear, each once; every
//     part begins once; no step appears twice;
//   - the pending batch's last launch precedes its completion, and both are in
//     the list exactly when a batch is pending;
//   - the new batch's first launch precedes everything of the pending batch
//     (the device has it queued before the host waits for anything);
//   - with one part and a hand-off to make, the new batch's first hand-off
//     precedes the pending batch's completion; with two parts the completion
//     comes after the second part's begin and before the hand-offs.
// The checker is then shown two wrong orders and must refuse both: the pending
// batch's completion moved back in front of a single part's hand-off, and a
// hand-off moved in front of its part's begin. Last, submit_parts' rule.
#include <cstdio>
#include <string>
#include <vector>

#include "csm_submit_order.hpp"

using namespace csmh;

namespace {

const char* name(SubmitStep s) {
  switch (s) {
    case SubmitStep::kBegin: return "begin";
    case SubmitStep::kHandoff: return "handoff";
    case SubmitStep::kPriorLast: return "prior_last";
    case SubmitStep::kPriorFinish: return "prior_finish";
  }
  return "?";
}

std::string show(const std::vector<SubmitOp>& v) {
  std::string s;
  for (const SubmitOp& o : v) {
    char b[48];
    if (o.step == SubmitStep::kBegin)
      std::snprintf(b, sizeof(b), "begin(p%d) ", o.part);
    else if (o.step == SubmitStep::kHandoff)
      std::snprintf(b, sizeof(b), "handoff(l%d,p%d) ", o.level, o.part);
    else
      std::snprintf(b, sizeof(b), "%s ", name(o.step));
    s += b;
  }
  return s;
}

int find(const std::vector<SubmitOp>& v, SubmitStep s, int level, int part) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == SubmitOp{s, level, part}) return (int)i;
  return -1;
}

// empty: the order is right; otherwise what is wrong with it
std::string wrong(const std::vector<SubmitOp>& v, int parts, int pending, int levels, bool defer) {
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t j = i + 1; j < v.size(); ++j)
      if (v[i] == v[j]) return "a step appears twice";
  size_t expect = 0;
  for (int h = 0; h < parts; ++h) {
    if (find(v, SubmitStep::kBegin, 0, h) < 0) return "a part never begins";
    ++expect;
  }
  for (int l = 0; l + 1 < levels; ++l)
    for (int h = 0; h < parts; ++h) {
      const int at = find(v, SubmitStep::kHandoff, l, h);
      const bool deferred = defer && l + 2 == levels && h == parts - 1;  // restated, not handoff_deferred()
      if (deferred != (at < 0)) return deferred ? "the deferred hand-off is in the list" : "a hand-off is missing";
      if (at < 0) continue;
      ++expect;
      const int before = l == 0 ? find(v, SubmitStep::kBegin, 0, h) : find(v, SubmitStep::kHandoff, l - 1, h);
      if (before < 0 || before > at) return "a hand-off precedes the launch of the level it completes";
    }
  const int last = find(v, SubmitStep::kPriorLast, 0, 0), fin = find(v, SubmitStep::kPriorFinish, 0, 0);
  if (pending > 0) {
    expect += 2;
    if (last < 0) return "the pending batch's last launch is missing";
    if (fin < 0) return "the pending batch is not finished inside the call";
    if (last > fin) return "the pending batch's finish precedes its last launch";
    if (find(v, SubmitStep::kBegin, 0, 0) > last) return "the pending batch's last launch precedes the new batch's first";
    const int h0 = find(v, SubmitStep::kHandoff, 0, 0);
    if (parts == 1 && h0 >= 0 && h0 > fin) return "one part: the pending batch's finish precedes the new batch's hand-off";
    if (parts == 2) {
      if (find(v, SubmitStep::kBegin, 0, 1) > fin) return "two parts: the finish precedes the second part's begin";
      if (h0 >= 0 && h0 < fin) return "two parts: a hand-off precedes the pending batch's finish";
    }
  } else if (last >= 0 || fin >= 0) {
    return "nothing pending, yet a step of a pending batch";
  }
  if (v.size() != expect) return "a step that belongs to no batch";
  return "";
}

std::vector<SubmitOp> listed(const SubmitOrder& o) { return std::vector<SubmitOp>(o.op, o.op + o.n); }

int failures = 0;
void fail(const char* what, const std::string& detail) {
  std::printf("FAIL %s: %s\n", what, detail.c_str());
  ++failures;
}

}  // namespace

int main() {
  int combos = 0, refused_finish_first = 0, refused_handoff_first = 0;
  for (int parts = 1; parts <= 2; ++parts)
    for (int pending = 0; pending <= 2; ++pending)
      for (int levels : {1, 3})
        for (int defer = 0; defer <= 1; ++defer) {
          const std::vector<SubmitOp> v = listed(submit_order(parts, pending, levels, defer != 0));
          char tag[64];
          std::snprintf(tag, sizeof(tag), "parts=%d pending=%d levels=%d defer=%d", parts, pending, levels, defer);
          std::printf("%s: %s\n", tag, show(v).c_str());
          const std::string w = wrong(v, parts, pending, levels, defer != 0);
          if (!w.empty()) fail(tag, w);
          ++combos;
          // mutant 1: the pending batch's finish back in front of a single part's first hand-off
          const int fin = find(v, SubmitStep::kPriorFinish, 0, 0), h0 = find(v, SubmitStep::kHandoff, 0, 0);
          if (parts == 1 && fin >= 0 && h0 >= 0) {
            std::vector<SubmitOp> m = v;
            m.erase(m.begin() + fin);
            m.insert(m.begin() + h0, SubmitOp{SubmitStep::kPriorFinish, 0, 0});
            if (wrong(m, parts, pending, levels, defer != 0).empty())
              fail(tag, "the checker accepted the finish in front of the hand-off: " + show(m));
            else
              ++refused_finish_first;
          }
          // mutant 2: a hand-off in front of its part's begin
          if (h0 >= 0) {
            std::vector<SubmitOp> m = v;
            m.erase(m.begin() + h0);
            m.insert(m.begin(), SubmitOp{SubmitStep::kHandoff, 0, 0});
            if (wrong(m, parts, pending, levels, defer != 0).empty())
              fail(tag, "the checker accepted a hand-off in front of its begin: " + show(m));
            else
              ++refused_handoff_first;
          }
        }
  // the two orders, as literals
  {
    const std::vector<SubmitOp> one = listed(submit_order(1, 1, 3, true));
    const std::vector<SubmitOp> want1 = {{SubmitStep::kBegin, 0, 0}, {SubmitStep::kPriorLast, 0, 0},
                                         {SubmitStep::kHandoff, 0, 0}, {SubmitStep::kPriorFinish, 0, 0}};
    if (one != want1) fail("one part", show(one));
    const std::vector<SubmitOp> two = listed(submit_order(2, 2, 3, true));
    const std::vector<SubmitOp> want2 = {{SubmitStep::kBegin, 0, 0},   {SubmitStep::kPriorLast, 0, 0},
                                         {SubmitStep::kBegin, 0, 1},   {SubmitStep::kPriorFinish, 0, 0},
                                         {SubmitStep::kHandoff, 0, 0}, {SubmitStep::kHandoff, 0, 1},
                                         {SubmitStep::kHandoff, 1, 0}};
    if (two != want2) fail("two parts", show(two));
  }
  // the most steps fit the list
  if (submit_order(kSubmitMaxParts, 2, kSubmitMaxLevels, false).n != kSubmitMaxParts * kSubmitMaxLevels + 2)
    fail("capacity", "the longest order does not fill the list exactly");
  // submit_parts: forced wins, then an explicit CSM_PIPELINE_PARTS, then the rule
  int rules = 0;
  for (int forced = 0; forced <= 2; ++forced)
    for (int set = 0; set <= 1; ++set)
      for (int pp = 2; pp <= 4; ++pp)
        for (int bound = 0; bound <= 1; ++bound) {
          const int k = submit_parts(forced, set != 0, pp, bound != 0);
          const int want = forced ? forced : (!set && bound) ? 1 : pp;
          if (k != want) {
            char b[96];
            std::snprintf(b, sizeof(b), "forced=%d set=%d parts=%d bound=%d: %d, want %d", forced, set, pp, bound, k, want);
            fail("submit_parts", b);
          }
          ++rules;
        }
  std::printf("combos=%d refused_finish_first=%d refused_handoff_first=%d rules=%d\n", combos, refused_finish_first,
              refused_handoff_first, rules);
  if (failures) return 1;
  std::printf("submit_order_check ok\n");
  return 0;
}
