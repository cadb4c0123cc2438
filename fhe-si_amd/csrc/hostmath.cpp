// hostmath.cpp -- host-side number theory for table construction (setup only; nothing here is on the hot path).
// Mirrors what FHEcontext / PAlgebra / Cmodulus compute at setup in the reference:
//   PAlgebra::init (PAlgebra.cpp:40-56), Cyclotomic (NumbTh.cpp:142-158), ProbPrime check (FHEContext.cpp:34).
#include "fhesi_internal.h"
#include <cmath>

#include <cstdarg>
#include <cstring>

static thread_local char g_err[512] = "";
void fhesi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* fhesi_last_error(void) { return g_err; }

namespace hm {

// (mulmod, powmod, invmod, is_prime, brv: hostbig.h)

// m = q^k or 2 q^k with q an odd prime, k >= 1: the rings whose Phi_m is Phi_q(+-X^s), s = q^(k-1) (PAlgebra.cpp:40-56 builds Phi_m for any m;
// these are the ones whose remainder is a three-term fold).  Returns q (0: m is not of that form) and k.
i64 prime_power_ring(i64 m, int* k) {
  if (m < 3) return 0;
  i64 Q = (m & 1) ? m : m / 2;
  if (!(Q & 1) || Q < 3) return 0;
  i64 q = 0;
  for (i64 d = 3; d * d <= Q; d += 2) if (Q % d == 0) { q = d; break; }
  if (!q) q = Q;                                   // Q itself is prime
  int e = 0;
  while (Q % q == 0) { Q /= q; ++e; }
  if (Q != 1) return 0;
  if (k) *k = e;
  return q;
}

u64 shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
u64 shoup63(u64 w, u64 q) { return (u64)(((u128)w << 63) / q); }

int ilog2_ceil(i64 n) {
  int k = 0;
  while ((1ll << k) < n) ++k;
  return k;
}

static u64 gcd(u64 a, u64 b) {
  while (b) { u64 t = a % b; a = b; b = t; }
  return a;
}

std::vector<int> zms_idx(i64 m, i64* phim) {
  std::vector<int> idx(m, -1);
  int k = 0;
  for (i64 i = 0; i < m; ++i)
    if (gcd((u64)i, (u64)m) == 1) idx[i] = k++;
  *phim = k;
  return idx;
}

static int mobius(i64 n) {
  int mu = 1;
  for (i64 p = 2; p * p <= n; ++p) {
    if (n % p == 0) {
      n /= p;
      if (n % p == 0) return 0;
      mu = -mu;
    }
  }
  return n > 1 ? -mu : mu;
}

// Phi_m = prod_{d | m} (X^{m/d} - 1)^{mu(d)}: the factors with mu = 1 are multiplied in, those with mu = -1 divided out ONE AT A TIME --
// both are O(degree) for a binomial X^e - 1 (quotient: Q[i] = Q[i - e] - A[i]), and every partial quotient is exact because the product
// of the mu = -1 binomials divides the numerator.  (A dense division by that product was quadratic: 46 s at m = 2^19, 194 s at the
// largest ring FHEContext.cpp:89 admits.)  Coefficients of cyclotomic polynomials for m <= 2^20 fit easily in 64 bits.
std::vector<i64> cyclotomic(i64 m) {
  std::vector<i64> t(1, 1);
  std::vector<i64> neg;
  for (i64 d = 1; d <= m; ++d) {
    if (m % d) continue;
    const int mu = mobius(d);
    const i64 e = m / d;
    if (mu == 1) {
      std::vector<i64> r(t.size() + e, 0);
      for (size_t i = 0; i < t.size(); ++i) { r[i + e] += t[i]; r[i] -= t[i]; }
      t.swap(r);
    } else if (mu == -1) neg.push_back(e);
  }
  for (const i64 e : neg) {
    std::vector<i64> q(t.size() - (size_t)e);
    for (size_t i = 0; i < q.size(); ++i) q[i] = (i >= (size_t)e ? q[i - e] : 0) - t[i];
    t.swap(q);
  }
  return t;
}

// Psi_m = (X^m - 1) / Phi_m = prod_{mu(d) = -1} (X^{m/d} - 1) / prod_{mu(d) = 1, d > 1} (X^{m/d} - 1), degree m - phi(m): the same
// binomial products and exact binomial divisions.  1 / Phi_m = -Psi_m (1 + X^m + X^2m + ...) as a power series, which is what makes the
// quotient of a division by Phi_m one product with Psi_m (bluestein.hip, the reduction modulo Phi_m for general m).
std::vector<i64> cyclotomic_cofactor(i64 m) {
  std::vector<i64> t(1, 1);
  std::vector<i64> pos;
  for (i64 d = 1; d <= m; ++d) {
    if (m % d) continue;
    const int mu = mobius(d);
    const i64 e = m / d;
    if (mu == -1) {
      std::vector<i64> r(t.size() + e, 0);
      for (size_t i = 0; i < t.size(); ++i) { r[i + e] += t[i]; r[i] -= t[i]; }
      t.swap(r);
    } else if (mu == 1 && d > 1) pos.push_back(e);
  }
  for (const i64 e : pos) {
    std::vector<i64> q(t.size() - (size_t)e);
    for (size_t i = 0; i < q.size(); ++i) q[i] = (i >= (size_t)e ? q[i - e] : 0) - t[i];
    t.swap(q);
  }
  return t;
}

bool is_primitive_2m_root(u64 root, i64 m, u64 q) {
  if (root == 0 || root >= q) return false;
  // order divides 2m; it is exactly 2m iff root^(2m/f) != 1 for every prime f | 2m
  if (powmod(root, 2 * (u64)m, q) != 1) return false;
  u64 e = 2 * (u64)m, t = e;
  for (u64 f = 2; f * f <= t; ++f) {
    if (t % f == 0) {
      if (powmod(root, e / f, q) == 1) return false;
      while (t % f == 0) t /= f;
    }
  }
  if (t > 1 && powmod(root, e / t, q) == 1) return false;
  return true;
}

// ---- plaintext slots (PlaintextSpace::Init / FindSlots / ReorderSlots, PlaintextSpace.cpp:20-110) for p prime, p = 1 mod m: Phi_m splits
// into linear factors X - r over Z_p, slot j sits on the root rho0^(g^j mod m).  Everything here is O(m) and runs once per slot space.
static std::vector<u64> prime_factors(u64 n) {
  std::vector<u64> f;
  for (u64 d = 2; d * d <= n; ++d)
    if (n % d == 0) { f.push_back(d); while (n % d == 0) n /= d; }
  if (n > 1) f.push_back(n);
  return f;
}
// 0, or why the ring is refused (each message names the failed condition)
const char* slot_space(i64 m, u64 p, i64 g, SlotSpace* out) {
  if (m < 2 || m > (1 << 20)) return "m outside [2, 2^20]";
  if (p >= (1ull << 32)) return "plaintext modulus p >= 2^32 (slot arithmetic is 32-bit)";
  if (!is_prime(p)) return "plaintext modulus p is not prime (p^r and composite moduli are not supported)";
  if ((p - 1) % (u64)m != 0) return "p != 1 mod m: ord_m(p) > 1, the slots would live in an extension field GF(p^d)";
  // (Z/m)^* cyclic  <=>  m = 2, 4, q^k or 2 q^k with q an odd prime
  SlotSpace S;
  S.m = m; S.p = p;
  {
    i64 odd = m;
    int twos = 0;
    while (odd % 2 == 0) { odd /= 2; ++twos; }
    const std::vector<u64> f = prime_factors((u64)odd);
    if (odd == 1) {
      if (twos > 2) return "(Z/m)^* is not cyclic (m = 2^k, k >= 3): no single generator walks all slots";
      S.kind = 0; S.q = 2;
    } else {
      if (f.size() != 1 || twos > 1) return "(Z/m)^* is not cyclic (m is not 2, 4, q^k or 2 q^k): no single generator walks all slots";
      S.kind = twos; S.q = (i64)f[0];
    }
    S.s = (S.kind ? m / 2 : m) / S.q;
    S.phim = (S.q - 1) * S.s;
  }
  const i64 n = S.phim;
  S.usable = 1;
  while (S.usable * 2 <= n) S.usable *= 2;
  // g generates (Z/m)^*: coprime to m and of order phi(m)  (PlaintextSpace.cpp:103 asserts that the walk visits every slot)
  {
    const u64 gm = (u64)(((g % m) + m) % m);
    bool ok = gcd(gm, (u64)m) == 1;
    if (ok && n > 1)
      for (u64 f : prime_factors((u64)n)) ok = ok && powmod(gm, (u64)n / f, (u64)m) != 1;
    if (!ok) return "the generator does not generate (Z/m)^*: its powers do not reach every slot";
    S.g = gm;
  }
  // rho0 = the least integer in [1, p) of multiplicative order m: the primitive m-th roots are z^j, gcd(j, m) = 1, for any z of order m
  {
    const std::vector<u64> fm = prime_factors((u64)m);
    u64 z = 0;
    for (u64 h = 2; h < p; ++h) {
      const u64 c = powmod(h, (p - 1) / (u64)m, p);
      bool ok = true;
      for (u64 f : fm) ok = ok && powmod(c, (u64)m / f, p) != 1;
      if (ok) { z = c; break; }
    }
    if (!z) return "no element of order m modulo p";
    u64 best = p, x = 1;
    for (i64 j = 1; j < m; ++j) {
      x = mulmod(x, z, p);
      if (gcd((u64)j, (u64)m) == 1 && x < best) best = x;
    }
    S.rho0 = best;
  }
  S.exps.resize(n);
  S.slot_of_exp.assign(m, -1);
  u64 e = 1 % (u64)m;
  for (i64 j = 0; j < n; ++j) {
    S.exps[j] = (int)e;
    S.slot_of_exp[e] = (int)j;
    e = mulmod(e, S.g, (u64)m);
  }
  // the chirp convolution has at most m terms below p^2: one auxiliary prime near 2^60 holds it exactly when m p^2 < 2^59, else two
  S.naux = ((u128)m * p * p < ((u128)1 << 59)) ? 1 : 2;
  *out = S;
  return nullptr;
}

// ---- two-row slot spaces of the power-of-two rings.  (Z/2^k)^* = <-1> x <g> for g = 3 or 5 mod 8 (g then has order h = m/4 and -1 is no
// power of it), so the n = m/2 roots of X^n + 1 modulo p = 1 mod m are rho0^(+-g^j): row 0 on g^j, row 1 on -g^j, j = 0 .. h-1.
const char* slot_space_pow2(i64 m, u64 p, i64 g, SlotSpace* out) {
  if (m < 1 || (m & (m - 1)) != 0) return "m is not a power of two (the two-row space is the one of X^(m/2) + 1)";
  if (m < 8) return "m = 2^k with k < 3: (Z/m)^* is cyclic there, the single-generator space covers it";
  if (m > (1 << 20)) return "m outside [8, 2^20]";
  if (p >= (1ull << 32)) return "plaintext modulus p >= 2^32 (slot arithmetic is 32-bit)";
  if (!is_prime(p)) return "plaintext modulus p is not prime (p^r and composite moduli are not supported)";
  if ((p - 1) % (u64)m != 0) return "p != 1 mod m: ord_m(p) > 1, the slots would live in an extension field GF(p^d)";
  const u64 gm = (u64)(((g % m) + m) % m);
  if (gm % 8 != 3 && gm % 8 != 5) return "the generator is not 3 or 5 mod 8: its powers and their negatives do not reach every slot";
  SlotSpace S;
  S.m = m; S.p = p; S.g = gm;
  S.kind = 0; S.q = 2; S.s = m / 2;
  S.phim = S.usable = m / 2;
  S.rows = 2;
  const i64 n = S.phim, h = n / 2;
  // rho0 = the least integer in [1, p) of order m: z^j, j odd, for any z of order m (z^(m/2) = -1)
  {
    u64 z = 0;
    for (u64 c = 2; c < p && !z; ++c) {
      const u64 x = powmod(c, (p - 1) / (u64)m, p);
      if (powmod(x, (u64)m / 2, p) != 1) z = x;
    }
    if (!z) return "no element of order m modulo p";
    const u64 z2 = mulmod(z, z, p);
    u64 best = p, x = z;
    for (i64 j = 1; j < m; j += 2) {
      if (x < best) best = x;
      x = mulmod(x, z2, p);
    }
    S.rho0 = best;
  }
  S.exps.resize(n);
  S.slot_of_exp.assign(m, -1);
  u64 e = 1;
  for (i64 j = 0; j < h; ++j) {
    S.exps[j] = (int)e;
    S.exps[h + j] = (int)((u64)m - e);
    S.slot_of_exp[e] = (int)j;
    S.slot_of_exp[(u64)m - e] = (int)(h + j);
    e = mulmod(e, gm, (u64)m);
  }
  S.naux = ((u128)m * p * p < ((u128)1 << 59)) ? 1 : 2;
  // the whole row of n 32-bit words sits in one workgroup's LDS up to n = 2^15, and lazy values below 2p fit a word up to p < 2^31
  S.direct = n <= (1 << 15) && p < (1ull << 31);
  *out = S;
  return nullptr;
}

// ---- slot bases: k distinct primes p_c = 1 mod m on one two-row ring, P = prod p_c; a slot holds an integer modulo P, channel c its residue
// modulo p_c in the two-row space of (m, p_c, g).  Scope = the direct transform of every channel: m = 2^3 .. 2^16, p_c < 2^31.
static const char* basis_ring(i64 m, i64 g, u64* gm) {
  if (m < 1 || (m & (m - 1)) != 0) return "m is not a power of two (a slot basis lives on a two-row ring)";
  if (m < 8) return "m = 2^k with k < 3: no two-row space there";
  if (m > (1 << 16)) return "m above 2^16: the channels of a slot basis run the direct transform, which needs n <= 2^15";
  *gm = (u64)(((g % m) + m) % m);
  if (*gm % 8 != 3 && *gm % 8 != 5) return "the generator is not 3 or 5 mod 8: its powers and their negatives do not reach every slot";
  return nullptr;
}
const char* slot_basis(i64 m, const u64* primes, int k, i64 g, SlotBasis* out) {
  static thread_local char why[256];
  u64 gm = 0;
  if (const char* w = basis_ring(m, g, &gm)) return w;
  if (k < 1) return "no primes: a slot basis needs at least one";
  if (k > SlotBasis::MAXK) return "more than 32 primes";
  if (!primes) return "null prime list";
  SlotBasis B;
  B.m = m; B.g = gm; B.k = k;
  B.primes.assign(primes, primes + k);
  B.ch.resize(k);
  for (int c = 0; c < k; ++c) {
    const u64 p = primes[c];
    const char* w = nullptr;
    if (p >= (1ull << 31)) w = "p >= 2^31 (the direct transform keeps lazy values below 2p in a 32-bit word)";
    else if (!is_prime(p)) w = "not prime (p^r and composite moduli are not supported)";
    else if ((p - 1) % (u64)m != 0) w = "p != 1 mod m: ord_m(p) > 1, the slots would live in an extension field GF(p^d)";
    for (int j = 0; j < c && !w; ++j)
      if (primes[j] == p) w = "given twice (the residues modulo equal primes carry nothing new)";
    if (!w) w = slot_space_pow2(m, p, (i64)gm, &B.ch[c]);
    if (!w && !B.ch[c].direct) w = "outside the direct transform";
    if (w) { snprintf(why, sizeof(why), "prime %d (%llu): %s", c, (unsigned long long)p, w); return why; }
  }
  std::vector<u64> P(1, 1);
  for (int c = 0; c < k; ++c) P = bn_mul_small(P, primes[c]);
  B.limbs = (bn_bitlen(P) + 1 + 63) / 64;
  P.resize(B.limbs, 0);
  B.P = P;
  B.halfP = bn_half(P);                                      // floor(P / 2)
  B.garner.assign((size_t)k * k, 0);                         // [c][j], j < c: p_j^-1 mod p_c
  for (int c = 0; c < k; ++c)
    for (int j = 0; j < c; ++j) B.garner[(size_t)c * k + j] = invmod(primes[j] % primes[c], primes[c]);
  *out = B;
  return nullptr;
}
const char* slot_basis_plan(i64 m, int bits, int prime_bits, i64 g, std::vector<u64>* primes, int* limbs) {
  u64 gm = 0;
  if (const char* w = basis_ring(m, g, &gm)) return w;
  if (bits < 1 || bits > 31 * SlotBasis::MAXK) return "bits outside [1, 992]: 32 primes below 2^31 hold no more";
  if (prime_bits < 4 || prime_bits > 31) return "prime_bits outside [4, 31]";
  std::vector<u64> P(1, 1);
  primes->clear();
  u64 cand = (((1ull << prime_bits) - 2) / (u64)m) * (u64)m + 1;      // the largest 1 mod m below 2^prime_bits
  while (bn_bitlen(P) < bits + 2) {                          // P > 2^(bits + 1)  <=>  P >= 2^(bits + 1) + 1 (P is odd)  <=>  bitlen(P) >= bits + 2
    while (cand > (u64)m && !is_prime(cand)) cand -= (u64)m;
    if (cand <= (u64)m) return "not enough primes 1 mod m below 2^prime_bits for that many bits";
    if ((int)primes->size() == SlotBasis::MAXK) return "more than 32 primes would be needed: raise prime_bits";
    primes->push_back(cand);
    P = bn_mul_small(P, cand);
    cand -= (u64)m;
  }
  *limbs = (bn_bitlen(P) + 1 + 63) / 64;                    // at most 16: P < 2^(31 * 32)
  return nullptr;
}

}  // namespace hm

// The capacity rule of a sum of ciphertext x plaintext products (fhesi_plain_sum_bits, fhesi_ct_plain_sum_dev): every coefficient of
// sum_t part * w_t rem Phi_m is at most terms * growth * n * 2^(logQ-1) * maxabs in magnitude -- n products of a centred ciphertext
// coefficient and a plaintext coefficient per term, and the remainder modulo Phi_m multiplies a coefficient by at most growth = 1 (X^n + 1),
// 2 (the two-term folds of m = q^k, 2 q^k) or, conservatively, n (a general Phi_m), as Ciphertext *= ZZX sizes its product.  A centred
// representative needs that bound below HALF the chain product: the bits returned are log2(2 * bound).
double plain_sum_bits(i64 n, bool pow2, bool two_term, int logQ, u64 maxabs, i64 terms) {
  if (!maxabs || terms < 1) return 0.0;
  const double growth = pow2 ? 0.0 : (two_term ? 1.0 : std::log2((double)n));
  return 1.0 + std::log2((double)terms) + growth + std::log2((double)n) + (double)(logQ - 1) + std::log2((double)maxabs);
}
