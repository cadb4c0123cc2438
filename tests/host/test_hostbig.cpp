// test_hostbig.cpp -- TEST HARNESS (no GPU, no library): the host's big-integer helpers (fhe-si_amd/csrc/hostbig.h) on operands read from a
// file, one operation per line; the results go to standard output, one line each, for tests/test_hostbig.py to compare with Python's
// integers.  Built with -fsanitize=address,undefined.
//   operand: <limbs>:<hex>, the value on exactly that many limbs (two's complement where the operation is signed)
//   mul_small A b | mod_small A q | mod A q | bitlen A | shl A s | sub A B | ge A B | half A | pow64 q count first | inv_mod k m
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../fhe-si_amd/csrc/hostbig.h"

static hm::Big parse(const std::string& tok) {
  const size_t c = tok.find(':');
  const int n = std::atoi(tok.substr(0, c).c_str());
  std::string hex = tok.substr(c + 1);
  hm::Big v((size_t)n, 0);
  for (int i = 0; i < n && !hex.empty(); ++i) {
    const size_t take = hex.size() < 16 ? hex.size() : 16;
    v[i] = std::strtoull(hex.substr(hex.size() - take).c_str(), nullptr, 16);
    hex.resize(hex.size() - take);
  }
  return v;
}
static void print(const hm::Big& v) {
  for (size_t i = v.size(); i-- > 0;) std::printf("%016" PRIx64, v[i]);
  std::printf("\n");
}
static uint64_t word(const std::string& tok) { return std::strtoull(tok.c_str(), nullptr, 0); }

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: test_hostbig <operations file>\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string op, a, b, c;
    ss >> op >> a >> b >> c;
    if (op == "mul_small") print(hm::bn_mul_small(parse(a), word(b)));
    else if (op == "mod_small") std::printf("%" PRIu64 "\n", hm::bn_mod_small(parse(a), word(b)));
    else if (op == "mod") { const hm::Big v = parse(a); std::printf("%" PRIu64 "\n", hm::bn_mod(v.data(), (int)v.size(), word(b))); }
    else if (op == "bitlen") std::printf("%d\n", hm::bn_bitlen(parse(a)));
    else if (op == "shl") { hm::Big v = parse(a); hm::bn_shl(v, (int)word(b)); print(v); }
    else if (op == "sub") { hm::Big v = parse(a); hm::bn_sub(v, parse(b)); print(v); }
    else if (op == "ge") std::printf("%d\n", hm::bn_ge(parse(a), parse(b)) ? 1 : 0);
    else if (op == "half") print(hm::bn_half(parse(a)));
    else if (op == "pow64") print(hm::pow64_table(word(a), (int)word(b), word(c)));
    else if (op == "inv_mod") std::printf("%lld\n", (long long)hm::inv_mod((int64_t)std::strtoll(a.c_str(), nullptr, 0), (int64_t)word(b)));
    else { std::fprintf(stderr, "unknown operation: %s\n", line.c_str()); return 2; }
  }
  return 0;
}
