// crt_wide.h -- the wide-integer steps and the stores of the closing kernels (kernels_crt.hip), each written once.
//
// A value is W little-endian 64-bit limbs in one of two storage forms, and every step is one body over both:
//   WideRegs<N>      a register array u64[N]: the loops unroll over the compile-time bound N and are guarded by the run-time limb range, so every
//                    index is static (crt_kernel, crt_sum_kernel, ks_recombine_kernel);
//   WideCol<STRIDE>  limb i at p[i * STRIDE]: a thread's column of a limb-major LDS tile (ks_recombine_generic_kernel, STRIDE = 128) or its
//                    private array (modswitch_delta_kernel, STRIDE = 1); the loops run over the run-time range.
// The steps differ between the forms in the loop driver only (wide_up; wide_cmp carries its two drivers itself, the column form leaves at the
// first differing limb): unrolling the LDS form over its bound would cost it 20 or 44 guarded copies of every step, a run-time loop over
// registers would send them to scratch memory.
#pragma once
#include "fhesi_internal.h"

template <int N> struct WideRegs {
  u64 (&v)[N];
  static constexpr int BOUND = N;
  __device__ __forceinline__ u64 get(int i) const { return v[i]; }
  __device__ __forceinline__ void set(int i, u64 a) const { v[i] = a; }
};
template <int N> __device__ __forceinline__ WideRegs<N> wide_regs(u64 (&v)[N]) { return WideRegs<N>{v}; }
template <int STRIDE> struct WideCol {
  u64* p;
  static constexpr int BOUND = 0;
  __device__ __forceinline__ u64 get(int i) const { return p[i * STRIDE]; }
  __device__ __forceinline__ void set(int i, u64 a) const { p[i * STRIDE] = a; }
};

// f(i) for i = lo .. hi - 1, ascending
template <class X, class F> __device__ __forceinline__ void wide_up(int lo, int hi, F f) {
  if constexpr (X::BOUND > 0) {
#pragma unroll
    for (int i = 0; i < X::BOUND; ++i)
      if (i >= lo && i < hi) f(i);
  } else {
    for (int i = lo; i < hi; ++i) f(i);
  }
}
// x[0..W) > c[0..W), or >= with OR_EQUAL: most significant limb first, the first differing limb decides
template <bool OR_EQUAL, class X> __device__ __forceinline__ bool wide_cmp(const X& x, const u64* c, int W) {
  bool gt = false, decided = false;
  if constexpr (X::BOUND > 0) {
#pragma unroll
    for (int i = X::BOUND - 1; i >= 0; --i) {
      if (i < W) {
        const u64 h = c[i];
        if (!decided && x.get(i) != h) { gt = x.get(i) > h; decided = true; }
      }
    }
  } else {
    for (int i = W - 1; i >= 0 && !decided; --i) {
      const u64 h = c[i], xi = x.get(i);
      if (xi != h) { gt = xi > h; decided = true; }
    }
  }
  return OR_EQUAL ? (gt || !decided) : gt;
}
template <class X> __device__ __forceinline__ bool wide_gt(const X& x, const u64* c, int W) { return wide_cmp<false>(x, c, W); }
template <class X> __device__ __forceinline__ bool wide_ge(const X& x, const u64* c, int W) { return wide_cmp<true>(x, c, W); }
// x[0..W) -= p[0..W), borrow chain (modulo 2^(64 W))
template <class X> __device__ __forceinline__ void wide_sub(const X& x, const u64* p, int W) {
  u64 borrow = 0;
  wide_up<X>(0, W, [&](int i) {
    const u64 pi = p[i], xi = x.get(i), d = xi - pi, b1 = xi < pi, d2 = d - borrow, b2 = d < borrow;
    x.set(i, d2);
    borrow = b1 | b2;
  });
}
// x[lo..hi) -= (k * p)[lo..hi): the carry of the product and the borrow of the difference run together; what lies below lo is not formed and
// what leaves at hi is dropped.  K: a 32- or 64-bit unsigned word.
template <class X, class K> __device__ __forceinline__ void wide_mulsub(const X& x, K k, const u64* p, int lo, int hi) {
  u64 carry = 0, borrow = 0;
  wide_up<X>(lo, hi, [&](int i) {
    const u128 t = (u128)k * p[i] + carry;
    carry = (u64)(t >> 64);
    const u64 xi = x.get(i), tl = (u64)t, d = xi - tl, b1 = xi < tl, d2 = d - borrow, b2 = d < borrow;
    x.set(i, d2);
    borrow = b1 | b2;
  });
}
// Quotient estimate of x / P from the top two limbs t1:t0 of x (limbs W-1, W-2) and r1:r0 = floor(2^(64 (W-2) + 128) / P): the low word of
// floor(t * r / 2^128), never above the true quotient and at most 2 below it.
__device__ __forceinline__ u64 wide_qhat(u64 t0, u64 t1, u64 r0, u64 r1) {
  const u128 mid = (u128)t1 * r0 + (u64)(((u128)t0 * r0) >> 64);
  const u128 add = (u128)t0 * r1;
  const u128 mid2 = mid + add;
  const u128 qh = (u128)t1 * r1 + (mid2 >> 64) + ((mid2 < add) ? ((u128)1 << 64) : 0);
  return (u64)qh;
}

// ------------------------------------------------------------------------------------------------------------------ stores
// The stores of a finished two's complement value whose limb count and logQ are compile-time constants (crt_store_fixed): X(i) is limb i,
// sign-filled beyond the value, and takes static indices only -- limbs [0, BOUND) unroll, and the limbs the caller wants beyond BOUND (bit logQ
// lies below limb BOUND) hold `beyond`.
template <int BOUND, class F> __device__ __forceinline__ void crt_store_limbs(u64* o, i64 stride, int nl_out, u64 beyond, F f) {
#pragma unroll
  for (int i = 0; i < BOUND; ++i)
    if (i < nl_out) o[(i64)i * stride] = f(i);
  for (int i = BOUND; i < nl_out; ++i) o[(i64)i * stride] = beyond;
}
// bit logQ-1: the rounding carry of mode 1, the sign of the centred residue of mode 2
template <class F> __device__ __forceinline__ u64 crt_round_bit(const F& X, int logQ) { return (X((logQ - 1) >> 6) >> ((logQ - 1) & 63)) & 1; }
// mode 1, ScaleDown: y = floor((2x + q) / 2q) = (x >> logQ) + bit_{logQ-1}(x), q = 2^logQ (arithmetic shift = floor); the positive residue
// modulo 2^logQ, limb-major [nl_out][n]
template <int BOUND, class F> __device__ __forceinline__ void crt_store_scaled(const F& X, int logQ, u64* out, i64 poly, i64 n, i64 j, int nl_out) {
  const int w = logQ >> 6, b = logQ & 63;
  u64 carry = crt_round_bit(X, logQ);
  crt_store_limbs<BOUND>(out + poly * nl_out * n + j, n, nl_out, 0, [&](int i) {
    const u64 lo = X(i + w), hi = X(i + w + 1);
    u64 val = b ? ((lo >> b) | (hi << ((64 - b) & 63))) : lo;
    val += carry;
    carry = (carry && val == 0);
    return reduce_limb(val, i, logQ, 0);
  });
}
// mode 3: the positive residue modulo 2^logQ of the value itself, limb-major [nl_out][n] -- what ByteDecompPart (Ciphertext.cpp:94) takes of an
// unscaled part (the key switch after Ciphertext::operator>>=, Regression.h:171-172)
template <int BOUND, class F> __device__ __forceinline__ void crt_store_positive(const F& X, int logQ, u64* out, i64 poly, i64 n, i64 j, int nl_out) {
  crt_store_limbs<BOUND>(out + poly * nl_out * n + j, n, nl_out, 0, [&](int i) { return reduce_limb(X(i), i, logQ, 0); });
}
// The run-time epilogue: mode 0 (the value as it is, coefficient-major [n][nl_out]) and the three stores above with limb indices and logQ
// known at run time only.  The finished value is the thread's column of a limb-major LDS tile: limb i < W at col[i * stride], sign-filled beyond.
// (Modes 1 and 3 are written twice, here and in crt_store_scaled / crt_store_positive above: one body under both loop drivers cost
// crt_kernel<28 / 44, 0, 0, 0> SGPR spills, profiles/crt_wide_refactor_isa.txt.  A change to the rounding, the shift or the limb rule goes to both.)
__device__ __forceinline__ void crt_store_rt(const u64* col, int stride, int W, int mode, int logQ, u64* out, i64 poly, i64 n, i64 j, int nl_out) {
  const u64 sign_fill = (col[(W - 1) * stride] >> 63) ? ~0ull : 0ull;
  auto X = [&](int i) -> u64 { return i < W ? col[i * stride] : sign_fill; };
  if (mode == 0) {
    u64* o = out + (poly * n + j) * nl_out;
    for (int i = 0; i < nl_out; ++i) o[i] = X(i);
  } else if (mode == 1) {
    const int w = logQ >> 6, b = logQ & 63;
    u64 carry = crt_round_bit(X, logQ);
    u64* o = out + poly * nl_out * n + j;
    for (int i = 0; i < nl_out; ++i) {
      const u64 lo = X(i + w), hi = X(i + w + 1);
      u64 val = b ? ((lo >> b) | (hi << ((64 - b) & 63))) : lo;
      val += carry;
      carry = (carry && val == 0);
      o[(i64)i * n] = reduce_limb(val, i, logQ, 0);
    }
  } else if (mode == 3) {
    u64* o = out + poly * nl_out * n + j;
    for (int i = 0; i < nl_out; ++i) o[(i64)i * n] = reduce_limb(X(i), i, logQ, 0);
  } else {
    // the centred residue modulo 2^logQ, two's complement, coefficient-major [n][nl_out]
    const u64 sbit = crt_round_bit(X, logQ);
    u64* o = out + (poly * n + j) * nl_out;
    for (int i = 0; i < nl_out; ++i) o[i] = reduce_limb(X(i), i, logQ, sbit);
  }
}
// Coefficient-major output of mode 2: v holds the reduced limbs of the centred residue, sbit its sign: the fill of the limbs the caller wants beyond NV.
// A lane owns nl_out consecutive 8-byte limbs, so a direct store instruction of the wave touches 32-64 cache lines for 8-16 bytes each.  A
// whole wave (n a multiple of 64, one thread per coefficient, `whole_waves` from the caller's workgroup shape) whose caller takes exactly NW
// limbs hands its 64 x NW limbs -- one contiguous block of memory -- through LDS rows of its own (NWAVES = the most waves a workgroup of the caller has;
// stride NW + 1:
// conflict-free) and stores 512 contiguous bytes per instruction.  NW = the limbs below bit logQ; staged only when a power of two (the index
// split is shifts) within NV.  Every other caller takes the direct stores.
template <int NW, int NWAVES, int NV>
__device__ __forceinline__ void crt_store_coeff_major(const u64 (&v)[NV], u64 sbit, bool whole_waves, u64* out, i64 poly, i64 n, i64 j, int nl_out) {
  u64* o = out + (poly * n + j) * nl_out;
  if constexpr (NW <= NV && (NW & (NW - 1)) == 0) {
    if (nl_out == NW && (n & 63) == 0 && whole_waves) {
      __shared__ u64 stg[NWAVES][64 * (NW + 1)];
      const u32 lane = threadIdx.x & 63, wv = (threadIdx.x >> 6) % NWAVES;
      u64* __restrict__ st = stg[wv];
#pragma unroll
      for (int i = 0; i < NW; ++i) st[lane * (NW + 1) + i] = v[i];
      __builtin_amdgcn_wave_barrier();
      u64* __restrict__ ow = out + (poly * n + (j - lane)) * NW;      // the wave's block
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const u32 e = k * 64 + lane, tl = e / NW, ii = e % NW;
        ow[e] = st[tl * (NW + 1) + ii];
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < nl_out) o[i] = v[i];
  for (int i = NV; i < nl_out; ++i) o[i] = sbit ? ~0ull : 0ull;
}
