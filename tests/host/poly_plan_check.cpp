// poly_plan_check.cpp -- the Paterson-Stockmeyer planner and schedule of fhe-si_amd/csrc/poly_plan.h on the host, under AddressSanitizer / UBSan (no GPU, no
// library).  Reads cases from standard input, one per line, and prints one line per case:
//   plan  d baby                    -> B G nprod nks depth
//   sched p baby d c_0 .. c_d       -> B G npowers ninner | per level "L dst a b ..." | per inner sum "I g konst c entry ..." | "F konst c entry ..."
// entries as PolySchedule numbers them (powers, inner sums, W).  tests/test_poly_plan_host.py draws the cases and renders the model's schedule the same way.
#include "../../fhe-si_amd/csrc/poly_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

static long long num() {
  std::string t;
  if (!(std::cin >> t)) { std::fprintf(stderr, "truncated case\n"); std::exit(2); }
  return std::strtoll(t.c_str(), nullptr, 0);
}

int main() {
  std::string op;
  while (std::cin >> op) {
    if (op == "plan") {
      const int d = (int)num(), baby = (int)num();
      if (d < 1 || d > kPolyMaxDegree || baby < 0 || baby > d) { std::fprintf(stderr, "refused shape\n"); return 2; }
      const PolyCounts c = poly_plan(d, baby);
      std::printf("%d %d %d %d %d\n", c.B, c.G, c.nprod, c.nks, c.depth);
    } else if (op == "sched") {
      const uint64_t p = (uint64_t)num();
      const int baby = (int)num(), d = (int)num();
      if (d < 1 || d > kPolyMaxDegree || baby < 0 || baby > d || p < 2) { std::fprintf(stderr, "refused shape\n"); return 2; }
      std::vector<int64_t> coef((size_t)d + 1);
      for (int64_t& c : coef) c = (int64_t)num();
      const PolySchedule s = poly_schedule(coef.data(), d, p, poly_plan(d, baby).B);
      std::printf("%d %d %d %d", s.B, s.G, s.npowers, (int)s.inner.size());
      for (const auto& level : s.levels) {
        std::printf(" | L");
        for (const PolyProduct& q : level) std::printf(" %d %d %d", q.dst, q.a, q.b);
      }
      for (const PolyInner& u : s.inner) {
        std::printf(" | I %d %lld", u.g, (long long)u.konst);
        for (const PolyTerm& t : u.terms) std::printf(" %lld %d", (long long)t.c, t.entry);
      }
      std::printf(" | F %lld", (long long)s.final_konst);
      for (const PolyTerm& t : s.final_terms) std::printf(" %lld %d", (long long)t.c, t.entry);
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown case %s\n", op.c_str()); return 2; }
  }
  return 0;
}
