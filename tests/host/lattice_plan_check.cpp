// lattice_plan_check.cpp -- the plans of a strided / dilated convolution and of a sum pooling of fhe-si_amd/csrc/lattice_plan.h and their refusals on the
// host, under AddressSanitizer / UBSan (no GPU, no library).  Reads cases from standard input, one per line, and prints one line per case:
//   conv cols H W Cin Cout kh kw ah aw sy sx ty tx ey ex form   -> form nh key_switches terms oy ox amounts ..         or   refused <the condition>
//   pool cols H W kh kw sy sx form                              -> form nh nhor key_switches levels oy ox amounts ..   or   refused <the condition>
// tests/test_lattice_plan_host.py draws the cases and renders the model (tests/lattice_model.py) the same way.
#include "../../fhe-si_amd/csrc/lattice_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

static long long num() {
  std::string t;
  if (!(std::cin >> t)) { std::fprintf(stderr, "truncated case\n"); std::exit(2); }
  return std::strtoll(t.c_str(), nullptr, 0);
}

int main() {
  std::string op;
  char why[256];
  while (std::cin >> op) {
    if (op == "conv") {
      LatticeShape s;
      s.c.cols = num(); s.c.H = num(); s.c.W = num(); s.c.Cin = num(); s.c.Cout = num(); s.c.kh = num(); s.c.kw = num(); s.c.ah = num(); s.c.aw = num();
      s.g.sy = num(); s.g.sx = num(); s.g.ty = num(); s.g.tx = num(); s.g.ey = num(); s.g.ex = num();
      const int form = (int)num();
      if (lattice_refused(s, form, why, sizeof why)) { std::printf("refused %s\n", why); continue; }
      const LatticeConvPlan pl = lattice_conv_plan(s, form);
      if ((size_t)pl.p.nh != pl.p.amounts.size()) { std::fprintf(stderr, "nh and the amounts disagree\n"); return 2; }
      std::printf("%d %d %lld %lld %lld %lld", pl.p.form, pl.p.nh, (long long)pl.p.key_switches, (long long)pl.p.terms, (long long)pl.oy, (long long)pl.ox);
      for (const int64_t a : pl.p.amounts) std::printf(" %lld", (long long)a);
      std::printf("\n");
    } else if (op == "pool") {
      PoolShape s;
      s.cols = num(); s.H = num(); s.W = num(); s.kh = num(); s.kw = num(); s.sy = num(); s.sx = num();
      const int form = (int)num();
      if (pool_refused(s, form, why, sizeof why)) { std::printf("refused %s\n", why); continue; }
      const PoolPlan pl = pool_plan(s, form);
      if ((size_t)pl.nh != pl.amounts.size() || pl.nhor > pl.nh) { std::fprintf(stderr, "nh and the amounts disagree\n"); return 2; }
      std::printf("%d %d %d %lld %d %lld %lld", pl.form, pl.nh, pl.nhor, (long long)pl.key_switches, pl.levels, (long long)pl.oy, (long long)pl.ox);
      for (const int64_t a : pl.amounts) std::printf(" %lld", (long long)a);
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown case %s\n", op.c_str()); return 2; }
  }
  return 0;
}
