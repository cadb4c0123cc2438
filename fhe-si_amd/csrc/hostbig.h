// hostbig.h -- the host's big integers: little-endian 64-bit limbs in a std::vector, non-negative unless a function says otherwise.
// Host-only and free of HIP headers, so that a plain C++ program can test it (tests/host/test_hostbig.cpp); fhesi_internal.h includes it,
// and every table builder of the library takes its wide constants from here.
#pragma once
#include <cstdint>
#include <vector>

namespace hm {
typedef uint64_t bn_limb;
typedef unsigned __int128 bn_wide;
typedef std::vector<bn_limb> Big;

// ---- word-sized number theory: the one definition (fhesi_internal.h and hostmath.cpp take it from here)
inline bn_limb mulmod(bn_limb a, bn_limb b, bn_limb q) { return (bn_limb)(((bn_wide)a * b) % q); }
inline bn_limb powmod(bn_limb a, bn_limb e, bn_limb q) {
  bn_limb r = 1 % q;
  a %= q;
  for (; e; e >>= 1) {
    if (e & 1) r = mulmod(r, a, q);
    a = mulmod(a, a, q);
  }
  return r;
}
inline bn_limb invmod(bn_limb a, bn_limb q) { return powmod(a % q, q - 2, q); }      // q prime
// k^-1 modulo any m >= 1 (extended Euclid; k of either sign), in [0, m); 0 when gcd(k, m) != 1
inline int64_t inv_mod(int64_t k, int64_t m) {
  int64_t a = ((k % m) + m) % m, b = m, x0 = 1, x1 = 0;
  while (b) { const int64_t q = a / b; int64_t t = a - q * b; a = b; b = t; t = x0 - q * x1; x0 = x1; x1 = t; }
  return a == 1 ? ((x0 % m) + m) % m : 0;
}
inline bool is_prime(bn_limb n) {
  static const bn_limb bases[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};   // deterministic below 3.3e24
  if (n < 2) return false;
  for (bn_limb p : bases)
    if (n % p == 0) return n == p;
  bn_limb d = n - 1;
  int s = 0;
  while (!(d & 1)) { d >>= 1; ++s; }
  for (bn_limb a : bases) {
    bn_limb x = powmod(a, d, n);
    if (x == 1 || x == n - 1) continue;
    bool composite = true;
    for (int r = 1; r < s && composite; ++r) {
      x = mulmod(x, x, n);
      if (x == n - 1) composite = false;
    }
    if (composite) return false;
  }
  return true;
}
// the low `bits` bits of x in reverse order
inline bn_limb brv(bn_limb x, int bits) {
  bn_limb r = 0;
  for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
  return r;
}

// a * b, trimmed to its significant limbs (at least one)
inline Big bn_mul_small(const Big& a, bn_limb b) {
  Big r(a.size() + 1, 0);
  bn_limb c = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const bn_wide s = (bn_wide)a[i] * b + c;
    r[i] = (bn_limb)s;
    c = (bn_limb)(s >> 64);
  }
  r[a.size()] = c;
  while (r.size() > 1 && r.back() == 0) r.pop_back();
  return r;
}
// the magnitude a[0..n) modulo a word q > 0
inline bn_limb bn_mod_small(const bn_limb* a, int n, bn_limb q) {
  bn_limb r = 0;
  for (int i = n - 1; i >= 0; --i) r = (bn_limb)((((bn_wide)r << 64) | a[i]) % q);
  return r;
}
inline bn_limb bn_mod_small(const Big& a, bn_limb q) { return bn_mod_small(a.data(), (int)a.size(), q); }
// a signed two's complement value of n >= 1 limbs -> [0, q)  (role of NTL rem(ZZ, long))
inline bn_limb bn_mod(const bn_limb* limbs, int n, bn_limb q) {
  if (!(limbs[n - 1] >> 63)) return bn_mod_small(limbs, n, q);
  Big mag(limbs, limbs + n);                      // the magnitude ~x + 1 (2^(64 n - 1) for the most negative value: it fits)
  bn_limb c = 1;
  for (int i = 0; i < n; ++i) { const bn_limb v = ~mag[i] + c; c = (c && v == 0); mag[i] = v; }
  const bn_limb r = bn_mod_small(mag, q);
  return r ? q - r : 0;
}
// bits of a: 0 for zero
inline int bn_bitlen(const Big& a) {
  for (int i = (int)a.size() - 1; i >= 0; --i)
    if (a[i]) return 64 * i + 64 - __builtin_clzll(a[i]);
  return 0;
}
// a <<= sh (sh >= 0) at a's own width: modulo 2^(64 a.size())
inline void bn_shl(Big& a, int sh) {
  const int n = (int)a.size(), w = sh >> 6, b = sh & 63;
  Big r(n, 0);
  for (int i = n - 1; i >= w; --i) r[i] = (a[i - w] << b) | ((b && i - w - 1 >= 0) ? (a[i - w - 1] >> (64 - b)) : 0);
  a.swap(r);
}
// a -= b at a's own width: modulo 2^(64 a.size()); limbs b does not have count as zero, limbs of b beyond a's width are ignored
inline void bn_sub(Big& a, const Big& b) {
  bn_limb borrow = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const bn_limb bi = i < b.size() ? b[i] : 0, d = a[i] - bi, b1 = a[i] < bi, d2 = d - borrow, b2 = d < borrow;
    a[i] = d2; borrow = b1 | b2;
  }
}
// a >= b as magnitudes of any two widths
inline bool bn_ge(const Big& a, const Big& b) {
  for (size_t i = a.size() > b.size() ? a.size() : b.size(); i-- > 0;) {
    const bn_limb ai = i < a.size() ? a[i] : 0, bi = i < b.size() ? b[i] : 0;
    if (ai != bi) return ai > bi;
  }
  return true;
}
// floor(a / 2) at a's width: (P - 1) / 2 of an odd P
inline Big bn_half(const Big& a) {
  Big r(a.size(), 0);
  for (size_t i = 0; i < a.size(); ++i) r[i] = (a[i] >> 1) | (i + 1 < a.size() ? a[i + 1] << 63 : 0);
  return r;
}
// a at exactly n limbs (zero-filled; the caller knows that nothing significant is cut, or wants the value modulo 2^(64 n))
inline Big bn_resized(Big a, size_t n) { a.resize(n, 0); return a; }
// a += b at a's own width: modulo 2^(64 a.size()); limbs of b beyond a's width are ignored
inline void bn_add(Big& a, const Big& b) {
  bn_limb c = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const bn_wide s = (bn_wide)a[i] + (i < b.size() ? b[i] : 0) + c;
    a[i] = (bn_limb)s;
    c = (bn_limb)(s >> 64);
  }
}
// word l of the radix-2^R form of a (R <= 32; words beyond a are zero)
inline uint32_t bn_word(const Big& a, int l, int R) {
  const int bit = R * l, w = bit >> 6, o = bit & 63;
  bn_limb v = (size_t)w < a.size() ? a[w] >> o : 0;
  if (o + R > 64 && (size_t)w + 1 < a.size()) v |= a[w + 1] << (64 - o);
  return (uint32_t)(v & (((bn_limb)1 << R) - 1));
}
// sum_l w[l] 2^(R l) over count words below 2^R (R <= 32): the inverse of bn_word
inline Big bn_from_words(const uint32_t* w, int count, int R) {
  Big r(((size_t)count * R + 63) / 64 + 1, 0);
  for (int l = 0; l < count; ++l) {
    const int bit = R * l, i = bit >> 6, o = bit & 63;
    r[i] |= (bn_limb)w[l] << o;
    if (o + R > 64) r[i + 1] |= (bn_limb)w[l] >> (64 - o);
  }
  return r;
}
// a modulo 2^(8 n) in balanced bytes: out[c] in [-128, 127] with sum_c out[c] 256^c = a (mod 2^(8 n)); n <= 8 a.size()
inline void bn_balanced_bytes(const Big& a, int n, int8_t* out) {
  int carry = 0;
  for (int c = 0; c < n; ++c) {
    const int b = (int)((a[c >> 3] >> (8 * (c & 7))) & 255) + carry;      // 0 .. 256
    carry = b >= 128 ? 1 : 0;
    out[c] = (int8_t)(b - 256 * carry);
  }
}
// first * 2^(64 k) mod q for k < count: the weights of the limbs of a coefficient modulo a prime
inline Big pow64_table(bn_limb q, int count, bn_limb first = 1) {
  Big r((size_t)count);
  const bn_limb b = (bn_limb)(((bn_wide)1 << 64) % q);
  bn_limb cur = first % q;
  for (int k = 0; k < count; ++k) { r[k] = cur; cur = (bn_limb)((bn_wide)cur * b % q); }
  return r;
}
}  // namespace hm
