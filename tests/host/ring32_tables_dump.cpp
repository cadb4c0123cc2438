// ring32_tables_dump.cpp -- TEST HARNESS (no GPU, no library): the host tables of the 30-bit rows as the library's own builders make them
// (fhe-si_amd/csrc/ring32_tables.h: ring32_build, conv32_build), for tests/test_ring32_tables.py to compare with its model in Python's integers.
// Built by that test (make ring32_tables_dump) with -fsanitize=address,undefined.
//   ring32_tables_dump ring <S> <prime> ...                         the transform tables
//   ring32_tables_dump conv <S> <R> <WT> <nl> <lift> <prime> ...    ... and the tensor half's conversion tables over them
// Output: one line per value, "name index... : hex words"; the large tables (fwd, inv: [prime][2^S][2^14] pairs) as "name prime length sha256",
// the SHA-256 of the prime's block as little-endian 32-bit words (w, then floor(w 2^32 / p)).  The hash lives here, not in the library.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fhe-si_amd/csrc/ring32_tables.h"

// FIPS 180-4, over a whole buffer
static std::string sha256(const unsigned char* msg, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
      0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
      0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
      0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
      0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::vector<unsigned char> m(msg, msg + len);
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int i = 7; i >= 0; --i) m.push_back((unsigned char)(((uint64_t)len * 8) >> (8 * i)));
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  for (size_t blk = 0; blk < m.size(); blk += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)m[blk + 4 * i] << 24 | (uint32_t)m[blk + 4 * i + 1] << 16 | (uint32_t)m[blk + 4 * i + 2] << 8 | m[blk + 4 * i + 3];
    for (int i = 16; i < 64; ++i) w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t v[8];
    memcpy(v, h, sizeof v);
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + K[i] + w[i];
      const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int j = 7; j > 0; --j) v[j] = v[j - 1];
      v[4] += t1; v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += v[i];
  }
  char out[65];
  for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08" PRIx32, h[i]);
  return out;
}
static std::string le_bytes_hash(const Tw32* t, size_t count) {
  std::vector<unsigned char> b(count * 8);
  for (size_t i = 0; i < count; ++i)
    for (int k = 0; k < 4; ++k) { b[8 * i + k] = (unsigned char)(t[i].w >> (8 * k)); b[8 * i + 4 + k] = (unsigned char)(t[i].wp >> (8 * k)); }
  return sha256(b.data(), b.size());
}
static void words(const char* name, int a, const uint32_t* w, size_t n) {
  std::printf("%s %d :", name, a);
  for (size_t i = 0; i < n; ++i) std::printf(" %" PRIx32, w[i]);
  std::printf("\n");
}
static void pairs(const char* name, int a, const Tw32* t, size_t n) {
  std::printf("%s %d :", name, a);
  for (size_t i = 0; i < n; ++i) std::printf(" %" PRIx32 " %" PRIx32, t[i].w, t[i].wp);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "ring <S> <prime> ... | conv <S> <R> <WT> <nl> <lift> <prime> ...\n"); return 2; }
  const bool conv = !std::strcmp(argv[1], "conv");
  const int S = std::atoi(argv[2]), first = conv ? 7 : 3;
  if (S < 0 || S > 6 || argc <= first) return 2;
  std::vector<uint32_t> primes;
  for (int i = first; i < argc; ++i) primes.push_back((uint32_t)std::strtoull(argv[i], nullptr, 0));
  const int NP = (int)primes.size(), NS = 1 << S;
  hm::Ring32Tables t;
  if (!hm::ring32_build(primes, S, t)) { std::fprintf(stderr, "no 2n-th root\n"); return 1; }
  if (!conv) {
    const size_t per = (size_t)A32_N << S;
    std::printf("sizes : %zu %zu %zu %zu\n", t.fwd.size(), t.inv.size(), t.ht.size(), t.hs.size());
    for (int a = 0; a < NP; ++a) {
      const hm::Ring32Prime& q = t.k.pp[a];
      const Tw32 pp[4] = {q.head, q.head1[0], q.head1[1], q.tail};
      pairs("pp", a, pp, 4);
      words("ninv", a, &q.ninv, 1);
      words("last", a, &t.k.last[(size_t)a * NS], NS);
      pairs("ht", a, &t.ht[(size_t)a * A32_HT], A32_HT);
      if (S >= 3) pairs("hs", a, &t.hs[(size_t)a * 2 * A32_HSN(S)], 2 * A32_HSN(S));
      std::printf("fwd %d %zu %s\n", a, per, le_bytes_hash(&t.fwd[(size_t)a * per], per).c_str());
      std::printf("inv %d %zu %s\n", a, per, le_bytes_hash(&t.inv[(size_t)a * per], per).c_str());
    }
    return 0;
  }
  const int R = std::atoi(argv[3]), WT = std::atoi(argv[4]), nl = std::atoi(argv[5]);
  const uint64_t lift = std::strtoull(argv[6], nullptr, 0);
  const hm::Conv32Tables c = hm::conv32_build(t.k, NP, lift, nl, R, WT);
  std::printf("sizes : %d %zu %zu %zu %zu\n", c.stride, c.rns.size(), c.cinv.size(), c.inv57.size(), c.Mw.size());
  for (int cls = 0; cls < 2; ++cls)
    for (int a = 0; a < NP; ++a) words(cls ? "rns1" : "rns0", a, &c.rns[((size_t)cls * NP + a) * c.stride], c.stride);
  for (int a = 0; a < NP; ++a) {
    pairs("cinv", a, &c.cinv[(size_t)a * 2], 2);
    const uint32_t k[2] = {c.inv57[a], c.mu61[a]};
    words("consts", a, k, 2);
    pairs("closing", a, &c.closing[(size_t)a * 2], 2);
  }
  for (int a = 0; a <= NP; ++a) words("Mw", a, &c.Mw[(size_t)a * WT], WT);
  words("pad", 0, &c.Mw[(size_t)(NP + 1) * WT], c.Mw.size() - (size_t)(NP + 1) * WT);
  return 0;
}
