// ct_wide_check.cpp -- the multi-limb steps of fhe-si_amd/csrc/ct_wide.h on the host, under AddressSanitizer / UBSan (no GPU, no library).
// Reads cases from standard input, one per line, numbers in C notation (0x.. for limbs), and prints the resulting limbs in hex, one line per case:
//   add    M nl logQ carry two  x[nl] f[nl] g[nl]  x + f + g + carry (two = 0: x + f + carry)   -> carry out, centred store of x
//   mul    M nl logQ w neg  x[nl] f[nl]            x + f * w, then its negation if neg       -> limb nl of the sum, centred store of x
//   gather M nl logQ s1 s2  x[nl] a1[nl] a2[nl]    x, then x += s1 a1 + s2 a2 (one term of the rotated sum)   -> centred store of x
//   quot   M logQ cv p                             floor(cv 2^logQ / p)             -> M limbs
//   round  M nw logQ p      z[nw]                  Decrypt's rounding               -> carry, quotient, P[nw], |residual|[nw]
//   resid  M nw logQ        P[nw]                  the residual of a given P        -> |residual|[nw]
// M is the compile-time bound of the registers (the kernels' limb classes).  tests/test_ct_wide.py draws the cases and holds the expected values.
#include "../../fhe-si_amd/csrc/ct_wide.h"
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
static std::vector<u64> limbs(int n) {
  std::vector<u64> v((size_t)n);
  for (u64& x : v) x = num();
  return v;
}
static void put(u64 v) { std::printf("%llx ", (unsigned long long)v); }
static void put(const std::vector<u64>& v) { for (u64 x : v) put(x); }
template <int M> static void put(const u64 (&x)[M], int n) { for (int i = 0; i < n; ++i) put(x[i]); }

template <int M> static void run(const std::string& op) {
  u64 x[M];
  if (op == "quot") {
    const int logQ = (int)num();
    const i64 cv = (i64)num();
    ctw_floor_quotient(x, cv, logQ, num());
    put(x, M);
    return;
  }
  const int nl = (int)num(), logQ = (int)num();
  if (nl > M) { std::fprintf(stderr, "%d limbs in a bound of %d\n", nl, M); std::exit(2); }
  auto src = [](const std::vector<u64>& v) { return [&v](int i) { return v.at((size_t)i); }; };      // (at(): a step that reads limb nl or beyond ends the program)
  std::vector<u64> o((size_t)nl);
  if (op == "add" || op == "gather") {
    const u64 c = num(), d = num();
    const std::vector<u64> x0 = limbs(nl), f = limbs(nl), g = limbs(nl);
    if (op == "add") put(d ? ctw_sum(x, nl, c, src(x0), src(f), src(g)) : ctw_sum(x, nl, c, src(x0), src(f)));      // (d = 0: two sources, g is read and dropped)
    else {
      const int s1 = (int)(i64)c, s2 = (int)(i64)d;
      ctw_sum(x, nl, 0, src(x0));
      ctw_sum(x, nl, ctw_neg_carry(s1, s2), [&](int i) { return x[i]; }, [&](int i) { return ctw_signed(f.at((size_t)i), s1); }, [&](int i) { return ctw_signed(g.at((size_t)i), s2); });
    }
    ctw_store_centred(x, nl, logQ, o.data());
    put(o);
  } else if (op == "mul") {
    const u64 w = num(), neg = num();
    const std::vector<u64> x0 = limbs(nl), f = limbs(nl);
    put(ctw_muladd(x, nl, src(x0), src(f), w));
    if (neg) ctw_neg(x, nl);
    ctw_store_centred(x, nl, logQ, o.data());
    put(o);
  } else if (op == "round") {
    const u64 p = num();
    const std::vector<u64> z = limbs(nl);
    u64 a[M];
    u64 carry;
    round_product(z.data(), 0, nl, logQ, p, x, carry);
    put(carry);
    put(round_quotient(x, carry, nl, logQ));
    put(x, nl);
    round_residual(x, nl, logQ, a);
    put(a, nl);
  } else if (op == "resid") {
    const std::vector<u64> P = limbs(nl);
    u64 a[M];
    ctw_sum(x, nl, 0, src(P));
    round_residual(x, nl, logQ, a);
    put(a, nl);
  } else { std::fprintf(stderr, "unknown case %s\n", op.c_str()); std::exit(2); }
}

int main() {
  std::string op;
  while (std::cin >> op) {
    switch ((int)num()) {
      case 2: run<2>(op); break;
      case 4: run<4>(op); break;
      case 8: run<8>(op); break;
      case 9: run<9>(op); break;
      case 16: run<16>(op); break;
      case 17: run<17>(op); break;
      case 32: run<32>(op); break;
      case 34: run<34>(op); break;
      default: std::fprintf(stderr, "no such limb class\n"); return 2;
    }
    std::printf("\n");
  }
  return 0;
}
