// wave_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/test_wave_plan.cpp): the passes of a wave of sums
// of products, out[g] = sum_{t in [seg[g], seg[g+1])} pool[a_idx[t]] x other[b_idx[t]], for fhesi_ct_plain_sum_dev (other = prepared plaintexts,
// addressed directly) and fhesi_ct_mul_sum_relin_dev (other = the pool again: b's are operands gathered and transformed like a's).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

// groups [g, g + ng) in one launch: nua (+ nub) distinct operands, nt terms, its index words at ix + off; accumulate: the sums add to what an earlier
// piece of the same group left; close: the sums are complete behind this pass
struct WavePass { int64_t g, ng, nua, nub, nt; size_t off; bool accumulate, close; };
// ix, per pass: [distinct a][distinct b, or nothing][local a slot per term][local b slot per term, or b_idx verbatim][segment bounds, ng + 1]
struct WavePlan { std::vector<WavePass> passes; std::vector<int> ix; };

// Consecutive groups share a pass while they number at most max_groups and their distinct operands -- a's, plus b's counted apart when b_is_operand --
// at most max_operands; distinct operands are numbered in order of first appearance.  A pass always takes one group: a group that alone exceeds
// max_operands is summed piecewise into one accumulator, max_operands terms a piece (half of that when every term brings two operands).
// Empty groups are legal.
inline WavePlan wave_plan(const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, int64_t max_groups, int64_t max_operands, bool b_is_operand) {
  WavePlan plan;
  std::vector<int>& ix = plan.ix;
  std::map<int, int> slot_a, slot_b;
  auto add_pass = [&](int64_t g, int64_t ng, int64_t t0, int64_t t1, bool accumulate, bool close) {
    WavePass P{g, ng, 0, 0, t1 - t0, ix.size(), accumulate, close};
    slot_a.clear(); slot_b.clear();
    for (int64_t t = t0; t < t1; ++t) if (slot_a.emplace(a_idx[t], (int)slot_a.size()).second) ix.push_back(a_idx[t]);
    for (int64_t t = t0; b_is_operand && t < t1; ++t) if (slot_b.emplace(b_idx[t], (int)slot_b.size()).second) ix.push_back(b_idx[t]);
    P.nua = (int64_t)slot_a.size(); P.nub = (int64_t)slot_b.size();
    for (int64_t t = t0; t < t1; ++t) ix.push_back(slot_a[a_idx[t]]);
    for (int64_t t = t0; t < t1; ++t) ix.push_back(b_is_operand ? slot_b[b_idx[t]] : b_idx[t]);
    if (ng == 1) { ix.push_back(0); ix.push_back((int)(t1 - t0)); }                        // (one group, or a piece of one)
    else for (int64_t i = 0; i <= ng; ++i) ix.push_back(seg[g + i] - seg[g]);
    plan.passes.push_back(P);
  };
  max_groups = std::max<int64_t>(max_groups, 1);
  const int64_t step = std::max<int64_t>(b_is_operand ? max_operands / 2 : max_operands, 1);
  std::set<int> seen_a, seen_b, new_a, new_b;
  for (int64_t g = 0; g < ngroups;) {
    seen_a.clear(); seen_b.clear();
    int64_t g2 = g;
    while (g2 < ngroups && g2 - g < max_groups) {
      new_a.clear(); new_b.clear();
      for (int64_t t = seg[g2]; t < seg[g2 + 1]; ++t) {
        if (!seen_a.count(a_idx[t])) new_a.insert(a_idx[t]);
        if (b_is_operand && !seen_b.count(b_idx[t])) new_b.insert(b_idx[t]);
      }
      if (g2 > g && (int64_t)(seen_a.size() + new_a.size() + seen_b.size() + new_b.size()) > max_operands) break;
      seen_a.insert(new_a.begin(), new_a.end()); seen_b.insert(new_b.begin(), new_b.end());
      ++g2;
    }
    if (g2 - g == 1 && (int64_t)(seen_a.size() + seen_b.size()) > max_operands) {
      for (int64_t t0 = seg[g]; t0 < seg[g + 1]; t0 += step) { const int64_t t1 = std::min<int64_t>(t0 + step, seg[g + 1]); add_pass(g, 1, t0, t1, t0 != seg[g], t1 == seg[g + 1]); }
    } else add_pass(g, g2 - g, seg[g], seg[g2], false, true);
    g = g2;
  }
  return plan;
}
