// poly_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/poly_plan_check.cpp): the Paterson-Stockmeyer plan and schedule
// of fhesi_ct_poly_eval_dev, and the term lists of fhesi_ct_lin_comb_dev.  tests/poly_model.py is the normative statement; this header follows it.
//
// y = f(x) = sum_{k <= d} c_k x^k slot by slot, with B baby powers x^1 .. x^B and the giants x^(gB), g = 2 .. G - 1, G = floor(d / B) + 1:
//   f(x) = sum_{g < G} u_g(x) x^(gB),  u_g(x) = sum_{j < B, gB + j <= d} c_(gB+j) x^j.
// Every power is the product of two earlier ones (halving), an inner sum u_g a scalar linear combination of the babies with its constant, the outer sum
// over g >= 1 ONE sum of products with one key switch; group 0, the groups that are a constant alone and that sum close in one more combination.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int kPolyMaxDegree = 4096;

inline int poly_clog2(int v) { int r = 0; while ((1 << r) < v) ++r; return r; }      // ceil(log2 v), v >= 1

// the plan of a DENSE polynomial of degree d with B baby powers (1 <= B <= d): every coefficient counted non-zero
struct PolyCounts { int B, G, nprod, nks, depth; };
inline PolyCounts poly_counts(int d, int B) {
  const int G = d / B + 1;
  const int npairs = B >= 2 ? (G - 1) - (d % B == 0 ? 1 : 0) : 0;      // the groups g >= 1 that hold a term x^j, j >= 1: g B + 1 <= d
  const int powers = (B - 1) + std::max(G - 2, 0);
  return {B, G, powers + npairs, powers + (npairs ? 1 : 0), poly_clog2(B) + poly_clog2(std::max(G - 1, 1)) + (npairs ? 1 : 0)};
}
// baby = 0: the B of least key switches; of equal key switches the smaller depth; of equal depth the larger B
inline PolyCounts poly_plan(int d, int baby) {
  if (baby) return poly_counts(d, baby);
  PolyCounts best = poly_counts(d, 1);
  for (int B = 2; B <= d; ++B) {
    const PolyCounts c = poly_counts(d, B);
    if (c.nks < best.nks || (c.nks == best.nks && c.depth <= best.depth)) best = c;
  }
  return best;
}

// ---- the schedule of one item.  A ciphertext is named by its entry in the item's pool: the babies x^1 .. x^B at 0 .. B - 1, the giants x^(gB), g >= 2, at
// B + g - 2, then the inner sums u_g in the order of `inner`, then W.
struct PolyProduct { int dst, a, b; };                         // pool[dst] = MulRelin(pool[a], pool[b])
struct PolyTerm { int64_t c; int entry; };                     // c * pool[entry]
struct PolyInner { int g; std::vector<PolyTerm> terms; int64_t konst; };
struct PolySchedule {
  int B = 0, G = 0, npowers = 0, w_entry = 0, nentries = 0;    // npowers = B + G - 2; entries of one item: the powers, the inner sums, W
  std::vector<std::vector<PolyProduct>> levels;                // one call of the sum-of-products wave each; the destinations of a level are consecutive entries
  std::vector<PolyInner> inner;                                // ascending g; inner[i] lives at entry npowers + i and pairs with x^(g B)
  std::vector<PolyTerm> final_terms;                           // group 0's terms in ascending j, the constant-only groups in ascending g, then (1, W) if any pair exists
  int64_t final_konst = 0;
  int power_entry(int k) const { return k <= B ? k - 1 : B + k / B - 2; }
};
// c mod p in [0, p) and its centred representative in (-p/2, p/2]; p < 2^62
inline void poly_residues(int64_t c, uint64_t p, int64_t* cbar, int64_t* chat) {
  const int64_t P = (int64_t)p, r = ((c % P) + P) % P;
  *cbar = r;
  *chat = 2 * r <= P ? r : r - P;
}
inline PolySchedule poly_schedule(const int64_t* coef, int d, uint64_t p, int B) {
  PolySchedule s;
  const int G = d / B + 1;
  s.B = B; s.G = G; s.npowers = B + G - 2;
  for (int lv = 1; lv <= poly_clog2(B); ++lv) {
    std::vector<PolyProduct> level;
    for (int j = (1 << (lv - 1)) + 1; j <= std::min(1 << lv, B); ++j) level.push_back({s.power_entry(j), s.power_entry((j + 1) / 2), s.power_entry(j / 2)});
    s.levels.push_back(level);
  }
  for (int lv = 1; lv <= poly_clog2(std::max(G - 1, 1)); ++lv) {
    std::vector<PolyProduct> level;
    for (int g = (1 << (lv - 1)) + 1; g <= std::min(1 << lv, G - 1); ++g) level.push_back({s.power_entry(g * B), s.power_entry((g + 1) / 2 * B), s.power_entry(g / 2 * B)});
    s.levels.push_back(level);
  }
  std::vector<PolyTerm> lone;                                  // the groups g >= 1 that are a constant alone
  for (int g = 0; g < G; ++g) {
    std::vector<PolyTerm> terms;
    int64_t cbar, chat;
    for (int j = 1; j < B && g * B + j <= d; ++j) {
      poly_residues(coef[g * B + j], p, &cbar, &chat);
      if (chat) terms.push_back({chat, s.power_entry(j)});
    }
    poly_residues(coef[g * B], p, &cbar, &chat);
    if (g == 0) { s.final_terms = terms; s.final_konst = cbar; }
    else if (!terms.empty()) s.inner.push_back({g, terms, cbar});
    else if (chat) lone.push_back({chat, s.power_entry(g * B)});
  }
  s.final_terms.insert(s.final_terms.end(), lone.begin(), lone.end());
  s.w_entry = s.npowers + (int)s.inner.size();
  s.nentries = s.w_entry + 1;
  if (!s.inner.empty()) s.final_terms.push_back({1, s.w_entry});
  return s;
}

// ---- the term lists of a scalar linear combination as ct_lin_comb_kernel reads them: per group the terms of negative coefficient first, then the positive
// ones (sums modulo 2^(64 nl) are exact, so the order cannot matter), as (pool index, magnitude); terms of coefficient 0 dropped.
// bounds[3 g .. 3 g + 2] = first term, first positive term, end.
struct LinCombLists { std::vector<int32_t> idx; std::vector<uint64_t> mag; std::vector<int32_t> bounds; };
inline uint64_t lin_comb_mag(int64_t c) { return c < 0 ? (uint64_t)(-(c + 1)) + 1 : (uint64_t)c; }
inline LinCombLists lin_comb_lists(const int32_t* a_idx, const int64_t* coef, const int32_t* seg, int64_t ngroups) {
  LinCombLists L;
  L.bounds.reserve((size_t)ngroups * 3);
  for (int64_t g = 0; g < ngroups; ++g) {
    L.bounds.push_back((int32_t)L.idx.size());
    for (int sign = -1; sign <= 1; sign += 2) {
      for (int32_t t = seg[g]; t < seg[g + 1]; ++t)
        if (sign < 0 ? coef[t] < 0 : coef[t] > 0) { L.idx.push_back(a_idx[t]); L.mag.push_back(lin_comb_mag(coef[t])); }
      L.bounds.push_back((int32_t)L.idx.size());
    }
  }
  return L;
}
