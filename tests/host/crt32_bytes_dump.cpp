// crt32_bytes_dump.cpp -- TEST HARNESS (no GPU, no library): the operand tables of crt32_mfma_kernel as the library's own host routine builds them
// (fhe-si_amd/csrc/crt32_bytes.h over the table rows of ring32_tables.h), for the primes given on the command line; tests/test_crt32_mfma_model.py compares them with
// Python's integers and runs its model of the kernel on them.  Built by that test with -fsanitize=address,undefined.
//   crt32_bytes_dump <prime> <prime> ...      (28-bit words, 38 per row, window of 21 words from word 16: the compiled shape)
// Output: "d <slot> <a> <72 bytes>" for every slot and byte plane, then "aop <tile> <kstep> <lane> <4 words, hex>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fhe-si_amd/csrc/crt32_bytes.h"
#include "../../fhe-si_amd/csrc/ring32_tables.h"

int main(int argc, char** argv) {
  const int R = 28, WT = 38, J0 = 16, NW = 21;
  std::vector<uint64_t> primes;
  for (int i = 1; i < argc; ++i) primes.push_back(std::strtoull(argv[i], nullptr, 0));
  const int NP = (int)primes.size();
  if (NP < 32 || NP + 2 > hm::C32B_SLOTS) { std::fprintf(stderr, "32 .. 38 primes\n"); return 2; }
  // the table rows from the library's own builder (ring32_tables.h, what t32_config uploads): M / p_i, and 2^(R WT) - M behind them
  const std::vector<uint32_t> p32(primes.begin(), primes.end());
  const std::vector<uint32_t> Mw = hm::crt32_mw(p32.data(), NP, R, WT);
  const hm::Crt32Bytes t = hm::crt32_bytes_build(Mw.data(), NP, WT, R, J0, NW);
  for (int s = 0; s < hm::C32B_SLOTS; ++s)
    for (int a = 0; a < 4; ++a) {
      std::printf("d %d %d", s, a);
      for (int c = 0; c < hm::C32B_COLS; ++c) std::printf(" %d", (int)t.d[((size_t)s * 4 + a) * hm::C32B_COLS + c]);
      std::printf("\n");
    }
  for (int tile = 0; tile < hm::C32B_TILES; ++tile)
    for (int ks = 0; ks < hm::C32B_KSTEPS; ++ks)
      for (int l = 0; l < 64; ++l) {
        const uint32_t* w = &t.aop[(((size_t)tile * hm::C32B_KSTEPS + ks) * 64 + l) * 4];
        std::printf("aop %d %d %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", tile, ks, l, w[0], w[1], w[2], w[3]);
      }
  return 0;
}
