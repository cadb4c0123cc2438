// ct_wide.h -- the multi-limb steps of the coefficient-domain ciphertext kernels (kernels_ct.hip), each written once.
//
// A value is u64 x[MAXNL], little-endian two's complement, of which the run-time nl <= MAXNL limbs count (the rest is never read): every loop unrolls over the
// compile-time bound and is guarded by the run-time count, so every index is static and the array stays in registers.  A limb SOURCE is
// anything callable int -> u64 (a pointer's limbs, a sign fill, a masked or shifted view of them), called with static indices only.
// A source that reads memory captures its pointer by value ([=]): captured by reference a kernel argument loses its __restrict__ inside the step
// (ct_mul_long_kernel<8> 623 -> 660 instructions, profiles/ct_wide_refactor_isa.txt).
// The header includes no HIP header and compiles as plain C++ too: tests/host/ct_wide_check.cpp runs every step on the host under the
// sanitizers against Python integers (tests/test_ct_wide.py).
#pragma once
#include <cstdint>

typedef uint64_t u64;
typedef int64_t i64;
typedef unsigned __int128 u128;
#if defined(__HIPCC__)
#define CTW_FN __device__ __forceinline__
CTW_FN u64 ctw_mulhi(u64 a, u64 b) { return __umul64hi(a, b); }
#else
#define CTW_FN inline
CTW_FN u64 ctw_mulhi(u64 a, u64 b) { return (u64)(((u128)a * b) >> 64); }
#endif

// Reduce (Util.cpp:3-26) of limb i of a value modulo 2^logQ: sign-extend from bit logQ-1 (sbit = that bit: the centred residue) or clear
// everything from bit logQ upwards (sbit = 0: the positive residue).  The one limb rule of every run-time store loop.
CTW_FN u64 reduce_limb(u64 val, int i, int logQ, u64 sbit) {
  const int bits_left = logQ - 64 * i;
  if (bits_left <= 0) return sbit ? ~0ull : 0ull;
  if (bits_left < 64) { const u64 mask = (1ull << bits_left) - 1; return sbit ? (val | ~mask) : (val & mask); }
  return val;
}

template <int MAXNL> CTW_FN void ctw_zero(u64 (&x)[MAXNL]) {
#pragma unroll
  for (int i = 0; i < MAXNL; ++i) x[i] = 0;
}
// x[0..nl) = the sum of the sources + carry (carry <= 2: the +1 of one or two negated sources; at most three sources); returns what leaves at
// limb nl.  A source may read x itself (x += ...): limb i is read before it is written.
template <int MAXNL, class... F> CTW_FN u64 ctw_sum(u64 (&x)[MAXNL], int nl, u64 carry, F... f) {
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i < nl) {
      u64 s = carry, c = 0;
      auto term = [&](u64 v) { s += v; c += s < v; };
      (term(f(i)), ...);
      x[i] = s;
      carry = c;
    }
  return carry;
}
// x[0..nl) = acc + f * w; returns limb nl of the value (acc + f w < 2^(64 (nl + 1)): it fits).  acc may read x itself.
template <int MAXNL, class A, class F> CTW_FN u64 ctw_muladd(u64 (&x)[MAXNL], int nl, A acc, F f, u64 w) {
  u64 carry = 0;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i < nl) {
      const u64 a = f(i), lo = a * w, hi = ctw_mulhi(a, w);      // hi <= 2^64 - 2: the two carries below fit
      const u64 s = lo + carry, s2 = s + acc(i);
      carry = hi + (s < lo) + (s2 < s);
      x[i] = s2;
    }
  return carry;
}
struct CtwNone { CTW_FN u64 operator()(int) const { return 0; } };      // the absent source
// x[0..nl) = -x, two's complement
template <int MAXNL> CTW_FN void ctw_neg(u64 (&x)[MAXNL], int nl) {
  u64 c = 1;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i < nl) { const u64 v = ~x[i] + c; c = (c && v == 0); x[i] = v; }
}
// A limb of a gathered term s a, s in {-1, 0, 1}: the limb, its complement (the +1 of the negation is ctw_neg_carry, the carry-in of the sum), or 0
CTW_FN u64 ctw_signed(u64 v, int s) { return (v ^ (s < 0 ? ~0ull : 0ull)) & (s ? ~0ull : 0ull); }
CTW_FN u64 ctw_neg_carry(int s1, int s2) { return (u64)(s1 < 0) + (u64)(s2 < 0); }
// the sign of the centred residue modulo 2^logQ: bit logQ - 1
template <int MAXNL> CTW_FN u64 ctw_sign_bit(const u64 (&x)[MAXNL], int logQ) {
  u64 sb = 0;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i == (logQ - 1) >> 6) sb = (x[i] >> ((logQ - 1) & 63)) & 1;
  return sb;
}
// ReduceCoefficients of one coefficient: the centred residue of x modulo 2^logQ, limb i to o[i * stride]
template <int MAXNL> CTW_FN void ctw_store_centred(const u64 (&x)[MAXNL], int nl, int logQ, u64* o, i64 stride = 1) {
  const u64 sb = ctw_sign_bit(x, logQ);
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i < nl) o[i * stride] = reduce_limb(x[i], i, logQ, sb);
}

// ---- Ciphertext += ZZX (Ciphertext.cpp:147-156): q = floor(cv 2^logQ / p) modulo 2^(64 MAXNL), NTL's floor division.  |cv| 2^logQ occupies
// limbs sh, sh + 1 (sh = logQ / 64; MAXNL >= sh + 2 holds them), divided limb by limb from the top by 128 / 64-bit long division; a negative
// constant takes -(q + [remainder != 0]) (floor, not truncation).  A smaller MAXNL gives the same quotient modulo 2^(64 MAXNL): the limbs above leave the shift
// below, the remainders they hand down are the same (ctw_lin_comb, which needs the quotient modulo 2^logQ only; tests/host/ct_lin_comb_check.cpp).
template <int MAXNL> CTW_FN void ctw_floor_quotient(u64 (&q)[MAXNL], i64 cv, int logQ, u64 p) {
  const u64 mag = cv < 0 ? (u64)(-(cv + 1)) + 1 : (u64)cv;
  const int sh = logQ >> 6, bs = logQ & 63;
  const u64 lo = bs ? mag << bs : mag, hi = bs ? mag >> (64 - bs) : 0;
  ctw_zero(q);
  u64 rem = 0;
  for (int i = sh + 1; i >= 0; --i) {
    const u64 limb = i == sh + 1 ? hi : (i == sh ? lo : 0);
    const u128 cur = ((u128)rem << 64) | limb;
    const u64 ql = (u64)(cur / p);
    rem = (u64)(cur % p);
#pragma unroll
    for (int t = MAXNL - 1; t > 0; --t) q[t] = q[t - 1];         // q = q 2^64 + ql: after the last step limb i sits at index i; static indices only (a placement by index cost up to 26 VGPRs, profiles/ct_wide_refactor_isa.txt)
    q[0] = ql;
  }
  if (cv < 0) {
    ctw_sum(q, MAXNL, rem != 0, [&](int i) { return q[i]; });
    ctw_neg(q, MAXNL);
  }
}

// ---- a scalar linear combination with a constant (ct_lin_comb_kernel): x[0..nl) = -sum_{t in [t0, ts)} mag[t] a_t + sum_{t in [ts, t1)} mag[t] a_t
// (+ floor(cv 2^logQ / p) when with_const) modulo 2^(64 nl) -- exact modulo 2^logQ, which divides it.  The terms of negative coefficient come first: their sum is
// negated ONCE, where the positive ones begin.  src(t) is the limb source of a_t; mag is read at t only.  The quotient is taken modulo 2^(64 MAXNL) (limbs
// from MAXNL upwards leave ctw_floor_quotient's shift), of which the low nl limbs count.
template <int MAXNL, class S> CTW_FN void ctw_lin_comb(u64 (&x)[MAXNL], int nl, const u64* mag, int t0, int ts, int t1, S src, bool with_const, i64 cv, int logQ, u64 p) {
  ctw_zero(x);
  for (int t = t0; t < ts; ++t) ctw_muladd(x, nl, [&](int i) { return x[i]; }, src(t), mag[t]);
  if (ts > t0) ctw_neg(x, nl);
  for (int t = ts; t < t1; ++t) ctw_muladd(x, nl, [&](int i) { return x[i]; }, src(t), mag[t]);
  if (with_const) {
    u64 q[MAXNL];
    ctw_floor_quotient(q, cv, logQ, p);
    ctw_sum(x, nl, 0, [&](int i) { return x[i]; }, [&](int i) { return q[i]; });
  }
}

// ---- the rounding of Decrypt (FHE-SI.cpp:110-116): m = floor((2 p z + q) / (2 q)) mod p, q = 2^logQ.
// Writing z = zh * 2q + zl with zl = z mod 2q in [0, 2q) gives floor(...) = 2 p zh + floor((2 p zl + q) / 2q), and the first
// term vanishes modulo p: only the low logQ+1 bits of z matter, and the quotient is at most 2p.
// z: [..][nw] limbs, nw = ceil((logQ+1)/64), coefficient j.  Limbs 0 .. nw-1 of 2 p zl + q go to P, limb nw to `carry`.
// (The call form -- index and carry by reference -- and the add of q spelled out are the parent's: with a pointer to the coefficient, the carry returned
// and the add through ctw_sum, decrypt_noise_kernel<32> held 54 SGPRs in VGPR lanes for 48, profiles/ct_wide_refactor_isa.txt.)
template <int MAXNL> CTW_FN void round_product(const u64* __restrict__ z, i64 j, int nw, int logQ, u64 p, u64 (&P)[MAXNL], u64& carry) {
  const int top_bits = logQ + 1 - 64 * (nw - 1);                  // bits of zl in its top limb (1..64)
  const u64 top_mask = top_bits < 64 ? (1ull << top_bits) - 1 : ~0ull;
  carry = ctw_muladd(P, nw, CtwNone{}, [&](int i) { return i == nw - 1 ? z[j * nw + i] & top_mask : z[j * nw + i]; }, 2 * p);
  const int wq = logQ >> 6;                                       // q = 2^logQ sits in limb wq = nw - 1
  u64 add = 1ull << (logQ & 63);
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i < nw && i >= wq) { const u64 s = P[i] + add; add = s < add; P[i] = s; }
  carry += add;
}
// bits from logQ+1 upward: at most 2p, fits one word
template <int MAXNL> CTW_FN u64 round_quotient(const u64 (&P)[MAXNL], u64 carry, int nw, int logQ) {
  const int ws = (logQ + 1) >> 6, bs = (logQ + 1) & 63;
  u64 lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i) {
    if (i == ws) lo = (i < nw) ? P[i] : carry;
    if (i == ws + 1) hi = (i < nw) ? P[i] : (i == nw ? carry : 0);
  }
  if (ws == MAXNL) lo = carry;
  if (ws + 1 == MAXNL) hi = (nw == MAXNL) ? carry : hi;
  return bs ? ((lo >> bs) | (hi << (64 - bs))) : lo;
}
// ---- the noise of a ciphertext, from the same product: P = (2 p z + q) mod 2q is the remainder the rounding above throws away, r = P - q in
// [-q, q) the decryption residual (invariant noise v = r / 2q in [-1/2, 1/2)).  |r| takes logQ+1 bits, nw limbs as z does: bit logQ of P set
// means r >= 0 and |r| is P with that bit cleared; otherwise |r| = q - P, which is q at the half-way point P = 0.
// The residual equals the true noise only while the true noise is below 1/2: past that the message has already rounded to a neighbour and the
// residual measured is the distance to THAT message, so a budget of 0 reads "at or within one bit of failure", never "failed by this much".
template <int MAXNL> CTW_FN void round_residual(const u64 (&P)[MAXNL], int nw, int logQ, u64 (&a)[MAXNL]) {
  const int wq = logQ >> 6;                                       // (= nw - 1: the limb of bit logQ is the top limb)
  const u64 qbit = 1ull << (logQ & 63), top_mask = (qbit << 1) - 1;
  u64 nonneg = 0;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i)
    if (i == wq) nonneg = P[i] & qbit;
  u64 borrow = 0;
#pragma unroll
  for (int i = 0; i < MAXNL; ++i) {
    a[i] = 0;
    if (i < nw) {
      const u64 x = i == wq ? P[i] & top_mask : P[i];             // limb i of P mod 2q
      const u64 qi = i == wq ? qbit : 0;
      const u64 d = qi - x, d2 = d - borrow;
      borrow = (qi < x) | (d < borrow);
      a[i] = nonneg ? (i == wq ? x & ~qbit : x) : d2;
    }
  }
}
