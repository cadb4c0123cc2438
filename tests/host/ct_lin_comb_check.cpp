// ct_lin_comb_check.cpp -- the scalar linear combination of fhe-si_amd/csrc/ct_wide.h (ctw_lin_comb: what one thread of ct_lin_comb_kernel computes) behind the
// host's term lists (lin_comb_lists, fhe-si_amd/csrc/poly_plan.h), on the host under AddressSanitizer / UBSan (no GPU, no library).
// Reads cases from standard input, one per line, numbers in C notation (0x.. for limbs), and prints the stored limbs in hex, one line per case:
//   M nl logQ p with_const konst nterms  { coef a[nl] } * nterms      -> centred store of sum coef a + floor(konst 2^logQ / p)
// M is the compile-time bound of the registers (the kernel's limb classes 2, 8, 16, 32).  tests/test_ct_lin_comb_host.py draws the cases and holds the expected
// values.
#include "../../fhe-si_amd/csrc/ct_wide.h"
#include "../../fhe-si_amd/csrc/poly_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

static u64 num() {
  std::string t;
  if (!(std::cin >> t)) { std::fprintf(stderr, "truncated case\n"); std::exit(2); }
  return t[0] == '-' ? (u64)std::strtoll(t.c_str(), nullptr, 0) : (u64)std::strtoull(t.c_str(), nullptr, 0);
}

template <int M> static void run() {
  const int nl = (int)num(), logQ = (int)num();
  const u64 p = num();
  const bool with_const = num() != 0;
  const i64 konst = (i64)num();
  const int nterms = (int)num();
  if (nl > M) { std::fprintf(stderr, "%d limbs in a bound of %d\n", nl, M); std::exit(2); }
  std::vector<int32_t> a_idx((size_t)nterms);
  std::vector<int64_t> coef((size_t)nterms);
  std::vector<std::vector<u64>> a((size_t)nterms, std::vector<u64>((size_t)nl));
  for (int t = 0; t < nterms; ++t) {
    a_idx[(size_t)t] = t;
    coef[(size_t)t] = (i64)num();
    for (u64& v : a[(size_t)t]) v = num();
  }
  const int32_t seg[2] = {0, nterms};
  const LinCombLists L = lin_comb_lists(a_idx.data(), coef.data(), seg, 1);
  if (L.bounds.size() != 3 || L.idx.size() != L.mag.size() || (size_t)L.bounds[2] != L.idx.size()) { std::fprintf(stderr, "malformed lists\n"); std::exit(2); }
  u64 x[M];
  // (at(): a step that reads limb nl or beyond, or a term outside its bounds, ends the program; mag.data() of an empty list is never read)
  ctw_lin_comb(x, nl, L.mag.data(), L.bounds[0], L.bounds[1], L.bounds[2], [&](int t) {
    const std::vector<u64>& v = a.at((size_t)L.idx.at((size_t)t));
    return [&v](int i) { return v.at((size_t)i); };
  }, with_const, konst, logQ, p);
  std::vector<u64> o((size_t)nl);
  ctw_store_centred(x, nl, logQ, o.data());
  for (u64 v : o) std::printf("%llx ", (unsigned long long)v);
}

int main() {
  std::string m;
  while (std::cin >> m) {
    switch (std::atoi(m.c_str())) {
      case 2: run<2>(); break;
      case 8: run<8>(); break;
      case 16: run<16>(); break;
      case 32: run<32>(); break;
      default: std::fprintf(stderr, "no such limb class\n"); return 2;
    }
    std::printf("\n");
  }
  return 0;
}
