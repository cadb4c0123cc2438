// conv_plan_check.cpp -- the convolution plan, its refusals and the index lists of the plaintext sum of fhe-si_amd/csrc/conv_plan.h on the host, under
// AddressSanitizer / UBSan (no GPU, no library).  Reads cases from standard input, one per line, and prints one line per case:
//   plan  cols H W Cin Cout kh kw ah aw form   -> form nh key_switches terms amounts ..      or   refused <the condition>
//   lists nI nJ nk B G cnt                     -> nterms ngroups | a_idx .. | b_idx .. | seg ..
// tests/test_conv_plan_host.py draws the cases and renders the model (tests/conv_model.py) the same way.
#include "../../fhe-si_amd/csrc/conv_plan.h"
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
      ConvShape s;
      s.cols = num(); s.H = num(); s.W = num(); s.Cin = num(); s.Cout = num(); s.kh = num(); s.kw = num(); s.ah = num(); s.aw = num();
      const int form = (int)num();
      char why[256];
      if (conv_refused(s, form, why, sizeof why)) { std::printf("refused %s\n", why); continue; }
      const ConvPlan pl = conv_plan(s, form);
      if ((size_t)pl.nh != pl.amounts.size()) { std::fprintf(stderr, "nh and the amounts disagree\n"); return 2; }
      std::printf("%d %d %lld %lld", pl.form, pl.nh, (long long)pl.key_switches, (long long)pl.terms);
      for (const int64_t a : pl.amounts) std::printf(" %lld", (long long)a);
      std::printf("\n");
    } else if (op == "lists") {
      const int nI = (int)num(), nJ = (int)num(), nk = (int)num(), B = (int)num(), G = (int)num();
      const int64_t cnt = num();
      if (nI < 1 || nJ < 1 || nk < 1 || B < 1 || G < 1 || cnt < 1 || (int64_t)(G - 1) * B >= nk || (int64_t)G * B < nk) { std::fprintf(stderr, "refused shape\n"); return 2; }
      // exactly the sizes matvec_run allocates: an index past them is the sanitizer's to find
      const size_t nterms = (size_t)nI * nJ * nk * cnt, ngroups = (size_t)nI * G * cnt;
      std::vector<int32_t> a(nterms), b(nterms), seg(ngroups + 1);
      grid_sum_lists(nI, nJ, nk, B, G, cnt, a.data(), b.data(), seg.data());
      std::printf("%zu %zu |", nterms, ngroups);
      for (const int32_t v : a) std::printf(" %d", v);
      std::printf(" |");
      for (const int32_t v : b) std::printf(" %d", v);
      std::printf(" |");
      for (const int32_t v : seg) std::printf(" %d", v);
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown case %s\n", op.c_str()); return 2; }
  }
  return 0;
}
