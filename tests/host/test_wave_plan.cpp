// test_wave_plan.cpp -- TEST HARNESS (no GPU, no library): the pass planner of the sum waves (fhe-si_amd/csrc/wave_plan.h) on cases read from a
// file; the passes and the index array go to standard output for tests/test_wave_plan.py to compare with a restatement of the two planners
// this header replaced.  Built with -fsanitize=address,undefined.
//   case, one line:  b_is_operand max_groups max_operands ngroups  seg[0 .. ngroups]  a_idx[0 .. nterms)  b_idx[0 .. nterms)
//   answer:          "passes <count>", per pass "g ng nua nub nt off accumulate close", then "ix <words ...>"
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fhe-si_amd/csrc/wave_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: test_wave_plan <cases file>\n"); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    long long b_op, max_groups, max_operands, ngroups;
    if (!(ss >> b_op >> max_groups >> max_operands >> ngroups) || ngroups < 0) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    // exact-size heap arrays: a read past either end is the sanitizer's to report
    std::vector<int32_t> seg((size_t)ngroups + 1);
    for (int32_t& v : seg) ss >> v;
    const size_t nt = (size_t)seg[ngroups];
    std::vector<int32_t> a(nt), b(nt);
    for (int32_t& v : a) ss >> v;
    for (int32_t& v : b) ss >> v;
    if (!ss) { std::fprintf(stderr, "short case: %s\n", line.c_str()); return 2; }
    const WavePlan plan = wave_plan(a.data(), b.data(), seg.data(), ngroups, max_groups, max_operands, b_op != 0);
    std::printf("passes %zu\n", plan.passes.size());
    for (const WavePass& P : plan.passes)
      std::printf("%lld %lld %lld %lld %lld %zu %d %d\n", (long long)P.g, (long long)P.ng, (long long)P.nua, (long long)P.nub, (long long)P.nt, P.off, (int)P.accumulate, (int)P.close);
    std::printf("ix");
    for (int v : plan.ix) std::printf(" %d", v);
    std::printf("\n");
  }
  return 0;
}
