// ntt32_core.inc -- 32-bit negacyclic row transforms of 2^14 points over primes below 2^30 (Harvey butterflies on lazy values
// below 4p): the third-form forward / inverse kernels and their helpers, shared by the key switch through four auxiliary primes
// (kernels_aux32.hip) and the tensor half of the fused multiplication through ~35 of them (kernels_tensor32.hip).
// Included inside a translation unit after fhesi_internal.h; everything is static / templated.
// Tw32, A32_LOGN, A32_N, A32_HT, A32_HSN, t32_shift and every host table these kernels read -- a32_bitrev_powers, a32_permute_phase_c,
// hm::ring32_build -- live in ring32_tables.h (host-only, tested on the CPU); Ring32Dev below owns their device copies for both users.
#pragma once
#include <algorithm>
#include <type_traits>

#include "ring32_tables.h"

struct Aux32Primes { u32 p[4]; u32 ninv[4], ninv_p[4]; u64 pinv64[4] /* floor((2^64 - 1) / p) */, r64[4] /* 2^64 mod p */, r48[4] /* 2^48 mod p */;
                     u32 mont[4] /* -p^-1 mod 2^32 */, ninv_m[4], ninv_m_p[4] /* n^-1 2^32 mod p and its quotient: undoes the 2^-32 of dot32_kernel2's Montgomery step */;
                     u32 ninv_mw[4][4], ninv_mw_p[4][4] /* ... times the last inverse stage's twiddle, per sub-block (ntt32_inv_kernel3, MONT) */; };

// n = 2^15 (S = 1): one head stage (distance 2^14, a single twiddle per prime) in front of two independent 2^14-point sub-transforms
// with their own twiddle slices -- the structure of the 64-bit path (ntt_tile.inc); sub-row h of a row holds the evaluations of sub-block h.
struct Aux32Head { Tw32 head[4], tail_sum[4], tail_dif[4];         // psi^brv(1);  1/2 and psi^-brv(1) / 2  (the tail of the inverse)
                   Tw32 head1[4][2]; };                            // n = 2^16 (S = 2): the second head stage's twiddles psi^brv(2), psi^brv(3)
// n = 2^16 (S = 2: zero-padded rows of the linear-convolution rings with 2^15 < 2 phi(m) - 1 <= 2^16): TWO head stages (distances 2^15, 2^14;
// twiddles psi^brv(1); psi^brv(2), psi^brv(3)) in front of four 2^14-point sub-transforms; sub-block h runs stage t of its own on the
// table entries (2^t << S) + h 2^t + i.  The head and the tail of plain rows are passes of their own at this size (ntt32_head2_kernel,
// ntt32_tail2_kernel: kernels_aux32.hip); the digit loader and rns32_reduce take the head in their loaders (the upper half of a padded
// polynomial is zero, so the first head stage is a duplication and the second the x +- w y of the 2^15-point rows).
// the primes of the tensor half (kernels_tensor32.hip): up to 72 of them, passed by value like the four above
static constexpr int T32_MAXP = 76;
// mu61: floor(2^(32 + sh) / p) with sh = 29 for primes of 30 bits, sh = 28 for primes of 29 bits (t32_shift): the quotient estimate of a value
// below 2^(32 + sh) is  umulhi(v >> sh, mu61), at most 2 short
// closing != 0 (rows of 2^14, T32_ROWS_CRT): the last stage of ntt32_inv_kernel3 takes its pair of constants from here instead of the shared
// table's entries 0 and 1 -- ninv = (M / p_i)^-1 / n and ninv_w = that times the last stage's twiddle, each with its Shoup word: the rows leave
// the inverse already multiplied by the CRT constant of their prime (which depends on the number of primes: per configuration, not per ring)
struct T32Primes { u32 p[T32_MAXP], ninv[T32_MAXP], ninv_p[T32_MAXP], mu61[T32_MAXP], ninv_w[T32_MAXP], ninv_w_p[T32_MAXP]; u32 closing; };
static constexpr u32 T32_ROWS_PLAIN = 0, T32_ROWS_CRT = 1;      // what a row of the tensor half's inverse holds: x / n, or x (M / p_i)^-1 / n
// a host vector into a fresh device buffer; false (and *d null or to be freed by its owner) when either step fails
template <class T, class V>
static inline bool a32_upload(T** d, const V& v) {
  const size_t bytes = v.size() * sizeof(v[0]);
  return hipMalloc((void**)d, bytes) == hipSuccess && hipMemcpy(*d, v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
}
// The device copies of one hm::Ring32Tables, owned once for both users.  upload() fills fresh buffers and swaps them in only when every step has
// succeeded (then it frees the old ones); on failure it frees what it allocated and the old tables stay in force.
struct Ring32Dev {
  Tw32* d_fwd = nullptr;               // [primes][2^S][2^14]  psi^brv(idx), idx = m + i (stage with m groups, group i), per sub-block
  Tw32* d_inv = nullptr;               // [primes][2^S][2^14]  the inverses
  Tw32* d_ht = nullptr;                // S >= 2: [primes][A32_HT] head / tail constants of the stand-alone passes of S = 2
  u32* d_p = nullptr;                  // S >= 2: the primes
  Tw32* d_hs = nullptr;                // S >= 3: [primes][2][A32_HSN(S)] head / tail twiddles of ntt32_headS_kernel / ntt32_tailS_kernel
  void release() { hipFree(d_fwd); hipFree(d_inv); hipFree(d_ht); hipFree(d_p); hipFree(d_hs); *this = Ring32Dev(); }
  int upload(const hm::Ring32Tables& t) {
    Ring32Dev n;
    const int S = t.k.S;
    if (!(a32_upload(&n.d_fwd, t.fwd) && a32_upload(&n.d_inv, t.inv) && (S < 2 || (a32_upload(&n.d_ht, t.ht) && a32_upload(&n.d_p, t.k.primes))) &&
          (S < 3 || a32_upload(&n.d_hs, t.hs)))) {
      n.release();
      FHESI_FAIL("30-bit rows: uploading the transform tables of %d primes failed", (int)t.k.primes.size());
    }
    release();
    *this = n;
    return 0;
  }
};
struct fhesi_aux32 {
  Aux32Primes pr;
  Aux32Head hd;
  int S = 0;                           // log2 of the sub-transforms per row (0: rows of 2^14 elements, 1: rows of 2^15, 2: rows of 2^16, 3 .. 6: the simple path up to rows of 2^20)
  Ring32Dev tab;                       // the four primes' tables
};

static constexpr int A32_T = 512, A32_P = 592;      // LDS stride of a 512-element sub-problem (padded)
__device__ __forceinline__ u32 a32_f(u32 t_id) { return t_id + ((t_id >> 5) << 2); }       // position inside a sub-problem (4 pad words per 32)
__device__ __forceinline__ u32 mul_lazy32(u32 y, Tw32 t, u32 p) { return y * t.w - __umulhi(y, t.wp) * p; }     // y any 32-bit value -> [0, 2p)
__device__ __forceinline__ int a32_bfly_k(int b, int h) { return ((b / h) * 2 * h) + (b % h); }
// low 32 bits of a * b + c with c a 64-bit register pair of which only the low half matters: ONE v_mad_u64_u32 where a 32-bit
// expression needs a multiply and an add
__device__ __forceinline__ u64 mad64(u32 a, u32 b, u64 c) {
  u64 r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ u64 mul64(u32 a, u32 b) {
  u64 r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r), "=s"(carry) : "v"(a), "v"(b));
  return r;
}
// ... with a wave-uniform second factor taken straight from its scalar register (the "v" form costs a v_mov per uniform twiddle)
__device__ __forceinline__ u64 mul64_s(u32 a, u32 b_uniform) {
  u64 r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r), "=s"(carry) : "v"(a), "s"(b_uniform));
  return r;
}
// Cooley-Tukey butterfly on lazy values (below 4p < 2^32):  X' = X + w Y,  Y' = X - w Y.
// NEGW (the forward tables of the auxiliary primes and of the tensor half's primes): the table holds (-w mod 2^32, floor(w 2^32 / p)):  -T = Q p - y w  is two chained
//   multiply-adds, X' = X - (-T), Y' = X + (-T) + 2p one three-operand add: 7 instructions, 4.5 % on the digit transform.  The 64-bit
//   pairs cost registers (the plain-row variants used to spill with it; since the flat-index divisions left the kernels they do not).
// step (a constant after unrolling): the range step of this stage -- 1: min(x, x - 2p), [0, 4p) -> [0, 2p), every stage of a prime of 30 bits;
//   primes below 2^29 leave room up to 8p < 2^32, so a stage may take x as it is (0: outputs below x + 2p) and every other stage takes
//   2: min(x, x - 4p), [0, 8p) -> [0, 4p)  (a32_fwd_step29: six range steps in fourteen stages instead of fourteen)
template <bool NEGW = true, bool UNI = false, bool SMALLX = false>       // UNI: the twiddle is wave-uniform (phase A); SMALLX: x is known to be below 2p
__device__ __forceinline__ void a32_ct(u32& x, u32& y, Tw32 t, u32 p, int step = 1) {
  const u32 twop = 2 * p;
  if constexpr (NEGW) {
    const u32 X = (SMALLX || step == 0) ? x : (step == 2 ? min(x, x - 2 * twop) : min(x, x - twop));   // (unsigned: x - 2p wraps above x when x < 2p)
    const u32 Q = __umulhi(y, t.wp);
    const u32 nT = (u32)mad64(Q, p, UNI ? mul64_s(y, t.w) : mul64(y, t.w));  // -T mod 2^32, T in [0, 2p)
    x = X - nT;
    y = X + nT + twop;
  } else {
    const u32 X = x >= twop ? x - twop : x;
    const u32 T = mul_lazy32(y, t, p);
    x = X + T;
    y = X - T + twop;
  }
}
// Gentleman-Sande butterfly on values below 2p:  X' = X + Y,  Y' = (X - Y) w   (inverse tables hold w itself)
// Eight instructions (sum, difference + 2p as two, range step as two, three multiplies): the product d w and the correction -Q p as two
// chained multiply-adds, the conditional subtraction as a minimum.  The
// 64-bit temporaries do not fit the 80 registers of three workgroups per CU next to the 32 values and the 16 twiddle pairs the compiler
// keeps in flight (36-68 bytes of scratch in every variant, 3x slower rows), so the inverse kernels are built for 96 registers = two
// workgroups per CU (A32_INV_WAVES = 5): 10.6 -> 9.86 ms per step for the four inverse launches, +2 % on the pipeline, against the
// older form (one more: mul_lo, mul_hi, mul_lo, sub) at three workgroups (profiles/r03_ab_inverse_butterfly.txt; that form left the source in round 6).
#ifndef A32_INV_WAVES
#define A32_INV_WAVES 5
#endif
// SMALLIN: both inputs are known to be below p (the dot product's outputs): the sum needs no range step.  UNI: the twiddle is wave-uniform
// (phase A) and enters the multiply-add from its scalar register (the "v" form costs a v_mov per butterfly: 80 per thread and transform).
template <bool SMALLIN = false, bool UNI = false>
__device__ __forceinline__ void a32_gs(u32& x, u32& y, Tw32 t, u32 p) {
  const u32 twop = 2 * p;
  const u32 s = x + y, d = x - y + twop;
  x = SMALLIN ? s : min(s, s - twop);
  const u32 Q = __umulhi(d, t.wp);
  y = (u32)mad64(Q, 0u - p, UNI ? mul64_s(d, t.w) : mul64(d, t.w));
}

// Primes below 2^29 (PB = 29: the tensor half, kernels_tensor32.hip): lazy values may grow to 8p < 2^32.
// Forward (every output of a stage is below its x input + 2p): rows enter below 4p; stage g = 0 .. 13 takes its x as it is except the even
// stages from 2 on, which take min(x, x - 4p):  4p -> 6p -> 8p -> (step) 6p -> 8p -> (step) ...  -> below 8p after stage 13.
__device__ __forceinline__ constexpr int a32_fwd_step29(int g) { return (g >= 2 && !(g & 1)) ? 2 : 0; }
// Inverse: the product output y' is always below 2p, the sum output x' below 4p.  `fresh`: both inputs are product outputs of the stage
// before (below 2p): the sum needs no range step.  Otherwise both are taken as below 4p: d = x - y + 4p and x' = min(s, s - 4p).  Inside a phase
// the pairs of a stage are two sum outputs or two product outputs of the stage before (the register index says which: a constant after
// unrolling); the first stage after an exchange across threads takes everything as below 4p.  6 of the 13 range steps of a row go.
template <bool UNI = false>
__device__ __forceinline__ void a32_gs29(u32& x, u32& y, Tw32 t, u32 p, bool fresh) {
  const u32 twop = 2 * p, fourp = 4 * p;
  const u32 s = x + y, d = x - y + (fresh ? twop : fourp);
  x = fresh ? s : min(s, s - fourp);
  const u32 Q = __umulhi(d, t.wp);
  y = (u32)mad64(Q, 0u - p, UNI ? mul64_s(d, t.w) : mul64(d, t.w));
}

// rows of 2^16 elements (S = 2): the two head stages of a plain row in place, four elements per thread; p_arr / ht: the primes and the
// constants [prime][A32_HT] (ntt32_core.inc).  Inputs any lazy value below 4p, outputs below 4p.
static __global__ void __launch_bounds__(256) ntt32_head2_kernel(u32* __restrict__ rows, int nslots, int a0, const u32* __restrict__ p_arr, const Tw32* __restrict__ ht) {
  const i64 row = blockIdx.y;
  const int a = a0 + (int)(row % nslots);
  const u32 p = p_arr[a], twop = 2 * p;
  const Tw32 w0 = ht[a * A32_HT], w1a = ht[a * A32_HT + 1], w1b = ht[a * A32_HT + 2];
  u32* g = rows + row * 4 * A32_N;
  auto red = [&](u32 x) { return x >= twop ? x - twop : x; };
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < A32_N; e += (i64)gridDim.x * blockDim.x) {
    const u32 x0 = red(g[e]), x1 = red(g[e + A32_N]);
    const u32 t2 = mul_lazy32(g[e + 2 * A32_N], w0, p), t3 = mul_lazy32(g[e + 3 * A32_N], w0, p);
    const u32 a0v = x0 + t2, a2v = x0 + twop - t2, a1v = x1 + t3, a3v = x1 + twop - t3;         // below 4p
    const u32 ta = mul_lazy32(a1v, w1a, p), tb = mul_lazy32(a3v, w1b, p);
    const u32 c0 = red(a0v), c2 = red(a2v);
    g[e] = c0 + ta; g[e + A32_N] = c0 + twop - ta;
    g[e + 2 * A32_N] = c2 + tb; g[e + 3 * A32_N] = c2 + twop - tb;
  }
}
// ... and the two tail stages of the inverse: from the four sub-inverses A0..A3 (each already scaled by 2^-14, below p)
//   L0 = (A0 + A1) / 2, L1 = (A0 - A1) w1a^-1 / 2, U0 = (A2 + A3) / 2, U1 = (A2 - A3) w1b^-1 / 2;
//   x[e] = (L0 + U0) / 2, x[e + 2^14] = (L1 + U1) / 2, x[e + 2^15] = (L0 - U0) w0^-1 / 2, x[e + 3 2^14] = (L1 - U1) w0^-1 / 2
static __global__ void __launch_bounds__(256) ntt32_tail2_kernel(u32* __restrict__ rows, int nslots, int a0, const u32* __restrict__ p_arr, const Tw32* __restrict__ ht) {
  const i64 row = blockIdx.y;
  const int a = a0 + (int)(row % nslots);
  const u32 p = p_arr[a], twop = 2 * p;
  const Tw32 th = ht[a * A32_HT + 4], t1a = ht[a * A32_HT + 5], t1b = ht[a * A32_HT + 6], t0 = ht[a * A32_HT + 7];
  u32* g = rows + row * 4 * A32_N;
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < A32_N; e += (i64)gridDim.x * blockDim.x) {
    const u32 A0 = g[e], A1 = g[e + A32_N], A2 = g[e + 2 * A32_N], A3 = g[e + 3 * A32_N];      // all below p
    const u32 L0 = mul_lazy32(A0 + A1, th, p), L1 = mul_lazy32(A0 + p - A1, t1a, p), U0 = mul_lazy32(A2 + A3, th, p), U1 = mul_lazy32(A2 + p - A3, t1b, p);      // below 2p
    u32 v0 = mul_lazy32(L0 + U0, th, p), v1 = mul_lazy32(L1 + U1, th, p), v2 = mul_lazy32(L0 + twop - U0, t0, p), v3 = mul_lazy32(L1 + twop - U1, t0, p);
    g[e] = v0 >= p ? v0 - p : v0; g[e + A32_N] = v1 >= p ? v1 - p : v1;
    g[e + 2 * A32_N] = v2 >= p ? v2 - p : v2; g[e + 3 * A32_N] = v3 >= p ? v3 - p : v3;
  }
}

// ---- rows of 2^(14 + S) elements, S = 3 .. 6 (padded rows of the linear-convolution rings with 2^16 < 2 phi(m) - 1 <= 2^20: m up to 2^20 is
// allowed, FHEContext.cpp:89, and every reference driver uses m = p - 1): the SIMPLE path -- head and tail stages as passes of their own over
// materialised rows, 2^S sub-transforms of 2^14 points in between (the fused loaders stop at S = 2).  The first S stages of the row transform pair
// elements 2^14 or more apart: for a fixed position e < 2^14 they are an S-stage network over the 2^S values v[h] = row[h 2^14 + e], entirely
// inside one thread.  hs: per prime [2][A32_HSN(S)] (ring32_tables.h).
template <int S>
__device__ __forceinline__ void a32_head_net(u32 (&v)[1 << S], const Tw32* __restrict__ tw, u32 p) {
  const u32 twop = 2 * p;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int t = 1 << (S - 1 - s);
#pragma unroll
    for (int i = 0; i < (1 << s); ++i) {
      const Tw32 w = tw[(1 << s) + i];
#pragma unroll
      for (int j = 0; j < t; ++j) {
        const int h = 2 * i * t + j;
        const u32 x = v[h] >= twop ? v[h] - twop : v[h];
        const u32 T = mul_lazy32(v[h + t], w, p);          // any 32-bit value -> [0, 2p)
        v[h] = x + T; v[h + t] = x + twop - T;              // below 4p
      }
    }
  }
}
// plain rows in place: inputs any lazy value below 4p, outputs below 4p
template <int S>
static __global__ void __launch_bounds__(256) ntt32_headS_kernel(u32* __restrict__ rows, int nslots, int a0, const u32* __restrict__ p_arr, const Tw32* __restrict__ hs) {
  const i64 row = blockIdx.y;
  const int a = a0 + (int)(row % nslots);
  const u32 p = p_arr[a];
  u32* g = rows + (row << (A32_LOGN + S));
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  u32 v[1 << S];
#pragma unroll
  for (int h = 0; h < (1 << S); ++h) v[h] = g[(i64)h * A32_N + e];
  a32_head_net<S>(v, hs + (i64)a * 2 * A32_HSN(S), p);
#pragma unroll
  for (int h = 0; h < (1 << S); ++h) g[(i64)h * A32_N + e] = v[h];
}
// the S tail stages of the inverse over the 2^S sub-inverses (each scaled by 2^-14, below p): Gentleman-Sande stages S-1 .. 1, the last one
// (distance 2^(S-1), ONE twiddle) with the scaling 2^-S [2^32] folded into its two multiplications; outputs below p
template <int S>
static __global__ void __launch_bounds__(256) ntt32_tailS_kernel(u32* __restrict__ rows, int nslots, int a0, const u32* __restrict__ p_arr, const Tw32* __restrict__ hs, int mont) {
  const i64 row = blockIdx.y;
  const int a = a0 + (int)(row % nslots);
  const u32 p = p_arr[a], twop = 2 * p;
  const Tw32* __restrict__ tw = hs + ((i64)a * 2 + 1) * A32_HSN(S);
  u32* g = rows + (row << (A32_LOGN + S));
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  u32 v[1 << S];
#pragma unroll
  for (int h = 0; h < (1 << S); ++h) v[h] = g[(i64)h * A32_N + e];
#pragma unroll
  for (int s = S - 1; s >= 1; --s) {
    const int t = 1 << (S - 1 - s);
#pragma unroll
    for (int i = 0; i < (1 << s); ++i) {
      const Tw32 w = tw[(1 << s) + i];
#pragma unroll
      for (int j = 0; j < t; ++j) {
        const int h = 2 * i * t + j;
        const u32 x = v[h], y = v[h + t];                   // below 2p
        const u32 sm = x + y;
        v[h] = min(sm, sm - twop);
        v[h + t] = mul_lazy32(x + twop - y, w, p);
      }
    }
  }
  const Tw32 c = tw[(1 << S) + (mont ? 2 : 0)], wc = tw[(1 << S) + (mont ? 3 : 1)];
#pragma unroll
  for (int j = 0; j < (1 << (S - 1)); ++j) {
    const u32 x = v[j], y = v[j + (1 << (S - 1))];
    u32 r0 = mul_lazy32(x + y, c, p), r1 = mul_lazy32(x + twop - y, wc, p);
    v[j] = min(r0, r0 - p); v[j + (1 << (S - 1))] = min(r1, r1 - p);
  }
#pragma unroll
  for (int h = 0; h < (1 << S); ++h) g[(i64)h * A32_N + e] = v[h];
}

// ---- host side: the row-length exponent S as a compile-time constant, and the stand-alone head / tail passes
// f(std::integral_constant<int, S>) for the run-time S in LO .. HI; f reads it as decltype(s)::value.  false, and f not called, for any other S
template <int LO, int HI, class F>
static inline bool a32_with_S(int S, F&& f) {
  if (S == LO) { f(std::integral_constant<int, LO>{}); return true; }
  if constexpr (LO < HI) return a32_with_S<LO + 1, HI>(S, f);
  return false;
}
// nrows rows of 2^(14 + S) elements in launches of at most 65535 rows (grid.y), each a multiple of nslots: launch(first row, rows); false as soon as a launch says so
template <class F>
static inline bool a32_row_launches(u32* rows, i64 nrows, int nslots, int S, F&& launch) {
  const i64 step = (65535 / nslots) * (i64)nslots;
  for (i64 r0 = 0; r0 < nrows; r0 += step)
    if (!launch(rows + (r0 << (A32_LOGN + S)), (unsigned)std::min(step, nrows - r0))) return false;
  return true;
}
// The head stages of rows of 2^16 and longer (S >= 2) as a pass of their own, in place: row r belongs to prime a0 + r % nslots, nrows is a
// multiple of nslots.  t.d_ht: the constants of S = 2 (ntt32_head2_kernel / ntt32_tail2_kernel), t.d_hs: the twiddles of S >= 3.  false: no such pass for this S
static inline bool launch_ntt32_head_pass(hipStream_t stream, int S, u32* rows, i64 nrows, int nslots, int a0, const Ring32Dev& t) {
  return a32_row_launches(rows, nrows, nslots, S, [&](u32* rp, unsigned ny) {
    if (S == 2) { ntt32_head2_kernel<<<dim3(16, ny), 256, 0, stream>>>(rp, nslots, a0, t.d_p, t.d_ht); return true; }
    return a32_with_S<3, 6>(S, [&](auto s) { ntt32_headS_kernel<decltype(s)::value><<<dim3(A32_N / 256, ny), 256, 0, stream>>>(rp, nslots, a0, t.d_p, t.d_hs); });
  });
}
// ... and the tail stages of the inverse over the sub-inverses; mont: the rows carry dot32's factor 2^-32, undone here (S >= 3; at S = 2 the sub-inverses undo it)
static inline bool launch_ntt32_tail_pass(hipStream_t stream, int S, u32* rows, i64 nrows, int nslots, int a0, const Ring32Dev& t, int mont) {
  return a32_row_launches(rows, nrows, nslots, S, [&](u32* rp, unsigned ny) {
    if (S == 2) { ntt32_tail2_kernel<<<dim3(16, ny), 256, 0, stream>>>(rp, nslots, a0, t.d_p, t.d_ht); return true; }
    return a32_with_S<3, 6>(S, [&](auto s) { ntt32_tailS_kernel<decltype(s)::value><<<dim3(A32_N / 256, ny), 256, 0, stream>>>(rp, nslots, a0, t.d_p, t.d_hs, mont); });
  });
}

// element at a 32-bit BYTE offset from a wave-uniform base: `global_load/store v, v_off, s[base]`.  The offset is made opaque so that the
// compiler keeps it a 32-bit register (one add per access) instead of forming every 64-bit address with an add / add-with-carry pair.
__device__ __forceinline__ u32 ld32(const u32* __restrict__ base, u32 boff) { asm("" : "+v"(boff)); return *(const u32*)((const char*)base + boff); }
__device__ __forceinline__ void st32(u32* __restrict__ base, u32 boff, u32 v) {
  asm("" : "+v"(boff));
  __builtin_nontemporal_store(v, (u32*)((char*)base + boff));
}
struct Dig32Src { const u64* parts; int nl, digit_bits, nd; u32 n_src; u32 sub_units = 0 /* digit rows tiled per sub-chunk of this many units (0: the whole launch) */;
                  u32 nd_inv = 0, sub_inv = 0 /* floor(2^32 / nd), floor(2^32 / sub_units): div32() */; };     // limb-major scaled-down parts [npolys][nl][n_src]; elements from n_src upwards are zero (n_src < 2^14: linear convolution)

// x / d for a wave-uniform x < 2^32 with inv = floor(2^32 / d): the estimate is at most one short.  (The SALU multiplies but does not
// divide; a plain `/` of uniform values becomes ~25 VALU instructions per wave, 64-bit operands more -- a few per cent of a row transform.)
__host__ __device__ __forceinline__ u32 div32_inv(u32 d) { return d > 1 ? (u32)(((u64)1 << 32) / d) : 0xffffffffu; }
__device__ __forceinline__ u32 div32(u32 x, u32 d, u32 inv) {
  const u32 q = (u32)(((u64)x * inv) >> 32);
  return x - q * d >= d ? q + 1 : q;
}

// rows of 2^(14 + S), S >= 3: ByteDecomp (Ciphertext.cpp:82-105) + the head stages of the digit polynomial `unit` for all four auxiliary primes
// (the digits are read once): dst plain rows [unit][prime][2^S][2^14], values below 4p.  ntt32_fwd_kernel3<DIGITS, S >= 3> reads those rows,
// runs the sub-transforms and stores the tiled layout the dot product reads.
template <int S, bool WM>
static __global__ void __launch_bounds__(256) dig32_headS_kernel(Dig32Src ds, u32* __restrict__ dst, Aux32Primes pr, const Tw32* __restrict__ hs) {
  const i64 c = blockIdx.y;
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 poly = div32((u32)c, (u32)ds.nd, ds.nd_inv);
  const u32 d = (u32)c - (u32)poly * (u32)ds.nd;
  const u32 bit = d * (u32)ds.digit_bits, g0 = bit >> 5, sh = bit & 31;
  const u32 nbyt = (u32)ds.digit_bits >> 3, bo = sh >> 3;
  u32 sel = 0;
#pragma unroll
  for (u32 i = 0; i < 4; ++i) sel |= (i < nbyt ? bo + i : 0x0cu) << (8 * i);
  const u32* __restrict__ p32 = reinterpret_cast<const u32*>(ds.parts);
  constexpr u32 ES = WM ? 1 : 2;                    // words between consecutive coefficients of a word row
  auto wrow = [&](u32 g) -> const u32* { return WM ? p32 + (poly * (2 * ds.nl) + g) * (i64)ds.n_src : p32 + (((poly * ds.nl + (g >> 1)) * (i64)ds.n_src) << 1) + (g & 1); };
  const u32* __restrict__ w0 = wrow(g0);
  const bool two = (sh + ds.digit_bits > 32) && (int)((g0 + 1) >> 1) < ds.nl;
  const u32* __restrict__ w1 = two ? wrow(g0 + 1) : w0;
  u32 dig[1 << S];
#pragma unroll
  for (int h = 0; h < (1 << S); ++h) {
    const i64 el = (i64)h * A32_N + e;
    u32 v = 0;
    if (el < (i64)ds.n_src) v = __builtin_amdgcn_perm(two ? w1[el * ES] : 0u, w0[el * ES], sel);
    dig[h] = v;
  }
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    u32 v[1 << S];
#pragma unroll
    for (int h = 0; h < (1 << S); ++h) v[h] = dig[h];
    a32_head_net<S>(v, hs + (i64)a * 2 * A32_HSN(S), pr.p[a]);
    u32* g = dst + ((c * 4 + a) << (A32_LOGN + S));
#pragma unroll
    for (int h = 0; h < (1 << S); ++h) g[(i64)h * A32_N + e] = v[h];
  }
}
// ---- third form of the forward transform: the same butterflies and the same output order, laid out for THREE workgroups per CU.
// The row passes through an LDS buffer of HALF its size (16 sub-problem rows, 37.9 KB):
//   exchange 1 (across the workgroup) in two passes -- registers 0..15 of every thread, read by the threads of sub-problems 0..15
//   (waves 0..3), then registers 16..31 through the same rows for waves 4..7;
//   exchange 2 stays inside a wave (the 16 threads of a sub-problem only trade among themselves): every wave owns two rows and
//   moves its four sub-problems through them two at a time, with wave-level ordering only (LDS operations of a wave execute in order).
// Twiddles are fetched stage by stage instead of far ahead, which keeps the kernel below 80 registers (6 waves per SIMD).
static constexpr int A32_HR = 16;                   // rows of the half buffer
// The per-lane twiddles of the last four stages (table entries 1024 .. 16383) are stored in the ORDER THE WAVES LOAD THEM.  At
// stage v (groups of 16 >> v ... distance 8 >> v) thread t needs the 2^(v+1) consecutive entries from (1024 << v) + (t << (v + 1)): in the natural
// order a 16-byte load instruction of a wave touches 8 << v different 128-byte lines (64 at the last stage), 680 line requests per wave and
// transform where 120 carry the same bytes.  The builder (a32_permute_phase_c, ring32_tables.h) transposes every wave's block so that load q of
// stage v reads 64 lanes x 16 contiguous bytes:  pair (t, q) of stage v  ->  position ((t >> 6) * 2^v + q) * 64 + (t & 63)  of that stage's region.
static constexpr int A32_TBL = 992;
__device__ __forceinline__ u32 a32_tbl_pos(u32 e) {      // entry e (0 .. 991) of the phase-B table -> its LDS slot
  return e;
}
__device__ __forceinline__ void a32_stage_tbl(Tw32* __restrict__ tbl, const Tw32* __restrict__ tab, u32 tid) {
  tbl[a32_tbl_pos(tid)] = tab[32 + tid];
  if (tid < 992 - 512) tbl[a32_tbl_pos(512 + tid)] = tab[32 + 512 + tid];
}
// slot of entry i of sub-problem kq at phase-B stage u
__device__ __forceinline__ u32 a32_tbl_idx(int u, u32 kq, int i) {
  return (32 << u) - 32 + (kq << u) + i;
}
// the 2^(v+1) twiddles of thread (wave wv, lane) at phase-C stage v: tc[ii], ii = gq * 2^v + i
// the 2^(v+1) twiddles of thread (wave wv, lane) at phase-C stage v (the caller's loop over v is unrolled): tc[gq][i], entry ii = gq * 2^v + i
// buffer loads: the descriptor of the prime's table and the stage / wave / load offsets are scalar, the lane's 16 bytes are the ONE vector
// offset of all 15 loads (with global loads the compiler re-associates base + lane into 64-bit vector addresses and the kernel spills)
typedef unsigned int a32_v4u __attribute__((ext_vector_type(4)));
#define A32_LOAD_TC(tc, tab, v, tid, wv, lane)                                                                              \
  {                                                                                                                         \
    const u32 so_ = ((1024u << (v)) * 8u) + (((wv) << (v)) * 1024u);                                                        \
    _Pragma("unroll") for (int q_ = 0; q_ < (1 << (v)); ++q_) {                                                             \
      const a32_v4u x_ = __builtin_amdgcn_raw_buffer_load_b128(tab, lane, so_ + q_ * 1024u, 0);                             \
      const int i0_ = 2 * q_, i1_ = 2 * q_ + 1;                                                                             \
      tc[i0_ >> (v)][i0_ & ((1 << (v)) - 1)] = Tw32{x_.x, x_.y};                                                  \
      tc[i1_ >> (v)][i1_ & ((1 << (v)) - 1)] = Tw32{x_.z, x_.w};                                                  \
    }                                                                                                                       \
  }
// PAD: the source polynomials have fewer than 2^14 coefficients (linear-convolution rings): elements from n_src upwards are zero
// PR: where the primes come from (Aux32Primes: the four auxiliary primes of the key switch; T32Primes: the tensor half's primes)
// WM: the source polynomials are 32-bit WORD rows [npolys][2 nl][n_src] (the fused pipeline: crt32_scale writes them so) instead of 64-bit limb rows
// [npolys][nl][n_src]: a wave's load is 256 contiguous bytes (two cache lines) where the 8-byte stride of a limb row touches four for the same data
// PB: 30, or 29 = every prime of PR is below 2^29 (fewer range steps: a32_fwd_step29); plain rows only
template <bool DIGITS, int S, bool PAD = false, class PR = Aux32Primes, bool NEGW = true, bool WM = false, int PB = 30>
#ifndef A32_FWD_WAVES
#define A32_FWD_WAVES 6
#endif
#ifndef A32_FWD_WAVES_S1
#define A32_FWD_WAVES_S1 6
#endif
__global__ void __launch_bounds__(A32_T, (DIGITS && ((S == 1 && !PAD) || S == 2)) ? A32_FWD_WAVES_S1 : A32_FWD_WAVES) ntt32_fwd_kernel3(      // (the digit loader of 2^15-point rows holds two digits per element; since the twiddles are stored in load order it fits 80 registers without a spill: A32_FWD_WAVES_S1 = 6, three workgroups per CU like every other forward variant)
    u32* __restrict__ rows, i64 count, int nslots, int a0, PR pr, const Tw32* __restrict__ tabs,
                                                              Dig32Src ds, Aux32Head hd) {
  static_assert(PB == 30 || (PB == 29 && !DIGITS && NEGW), "primes below 2^29: plain rows of the tensor half");
  __shared__ u32 lds[A32_HR * A32_P];
  __shared__ Tw32 tbl[A32_TBL];                    // the prime's phase-B twiddles (entries 32..1023): 16 threads share each, so they are staged once per row
  const u32 tid = threadIdx.x;
  i64 c = blockIdx.x;                             // grid (units, prime slots x sub-blocks): the order of a flat index without its division
  int ps = (int)blockIdx.y;                       // (prime slot, sub-block)
  if (DIGITS) {
    // The transforms of a digit polynomial (4 primes x 2^S sub-blocks) read the same source words: block ids 8 apart run on one XCD, so XCD x
    // takes unit x of every run of 8, primes inside -- the 4 x 2^S transforms of a unit are served from that XCD's L2 after the first.
    // (Whole polynomials per XCD -- all 22 digits share their word rows -- cut FETCH_SIZE 3.4x and ran 1.6 % SLOWER: the waves wait on line
    // requests of the twiddle loads, not on these bytes; profiles/r05_ab_digit_fwd.txt.  That order left the source in round 6.)
    const u32 bid = blockIdx.x;
    ps = (int)((bid >> 3) & ((4u << S) - 1));
    c = (i64)(bid >> (5 + S)) * 8 + (bid & 7);
    if (c >= count) return;
  }
  const int slot = ps >> S, h = ps & ((1 << S) - 1);
  const int a = a0 + slot;
  const u32 p = pr.p[a];
  const Tw32* __restrict__ tab = tabs + (((i64)a << S) + h) * A32_N;
  u32* __restrict__ g = rows + ((((c * nslots + slot)) << S) + h) * A32_N;
  a32_stage_tbl(tbl, tab, tid);                    // (visible to everyone after the first barrier of exchange 1)
  u32 r[32];
  if constexpr (DIGITS && S >= 3) {
    // rows of 2^17 and longer (the simple path): the digit polynomials arrive as PLAIN rows [unit][prime][2^S][2^14] with their head stages done
    // (dig32_headS_kernel), ds.parts points at them; this kernel runs the sub-transform and stores the tiled layout like every digit variant
    const u32* __restrict__ srow = reinterpret_cast<const u32*>(ds.parts) + ((((c * 4 + slot)) << S) + h) * (i64)A32_N;
#pragma unroll
    for (int k = 0; k < 32; ++k) r[k] = srow[k * A32_T + tid];
  } else if (DIGITS) {
    const i64 poly = div32((u32)c, (u32)ds.nd, ds.nd_inv);
    const u32 d = (u32)c - (u32)poly * (u32)ds.nd;
    const u32 bit = d * (u32)ds.digit_bits, g0 = bit >> 5, sh = bit & 31;
    // ByteDecomp digits are whole bytes at whole-byte offsets: one v_perm_b32 picks them out of the (up to) two words, zero-filled
    const u32 nbyt = (u32)ds.digit_bits >> 3, bo = sh >> 3;
    u32 sel = 0;
#pragma unroll
    for (u32 i = 0; i < 4; ++i) sel |= (i < nbyt ? bo + i : 0x0cu) << (8 * i);
    const u32* __restrict__ p32 = reinterpret_cast<const u32*>(ds.parts);
    // word g of polynomial `poly`: element e at byte offset ES * e
    constexpr u32 ES = WM ? 4 : 8;
    auto wrow = [&](u32 g) -> const u32* { return WM ? p32 + (poly * (2 * ds.nl) + g) * (i64)ds.n_src : p32 + (((poly * ds.nl + (g >> 1)) * (i64)ds.n_src) << 1) + (g & 1); };
    const u32* __restrict__ w0 = wrow(g0);
    const bool two = (sh + ds.digit_bits > 32) && (int)((g0 + 1) >> 1) < ds.nl;
    const u32 ns = ds.n_src;
    static_assert(!(DIGITS && S >= 2 && !PAD), "digit rows of 2^16 and longer exist for the padded linear-convolution rings only");
    if (S == 0 || (PAD && S == 1)) {       // (padded rows of 2^15, S = 1 with PAD: the upper half of the polynomial is zero, so the head stage leaves x in both sub-blocks)
      if (two) {
        const u32* __restrict__ w1 = wrow(g0 + 1);
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const u32 el = k * A32_T + tid, e = ES * (PAD ? (el < ns ? el : 0u) : el);        // (unconditional loads from a clamped index, then a select)
          const u32 v = __builtin_amdgcn_perm(ld32(w1, e), ld32(w0, e), sel);
          r[k] = (!PAD || el < ns) ? v : 0u;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const u32 el = k * A32_T + tid;
          const u32 v = __builtin_amdgcn_perm(0u, ld32(w0, ES * (PAD ? (el < ns ? el : 0u) : el)), sel);
          r[k] = (!PAD || el < ns) ? v : 0u;
        }
      }
    } else {
      // rows of 2^15 coefficients: the head stage pairs coefficient el with el + 2^14 (both below 2^digit_bits):
      //   sub-block 0: x + w y,  sub-block 1: x + 2p - w y   (below 4p), then the 2^14-point sub-transform with its twiddle slice.
      // The loads are written out in batches, the branch on `two` outside them (as in the S = 0 loader): with the digit behind a lambda and a
      // ternary the compiler emitted one load, one wait and one branch per digit -- 64 serialised L2 round trips per thread, which made
      // this kernel twice as slow per sub-row as the rows of 2^14 (profiles/r04_stress_digit_loader.txt).
      // Padded rows of 2^16 (S = 2, PAD: fewer than 2^15 coefficients): the first head stage pairs el with el + 2^15 = 0 and leaves x in both halves;
      // the second is this same x +- w y with the half's own twiddle -- sub-blocks 0, 1: psi^brv(2), sub-blocks 2, 3: psi^brv(3); coefficients from
      // n_src upwards are zero (clamped load, masked value).
      const Tw32 hw = S == 2 ? hd.head1[a][h >> 1] : hd.head[a];
      const u32* __restrict__ w1 = wrow(g0 + 1);
      auto body = [&](auto TWO) {
        constexpr bool two_c = decltype(TWO)::value;
        // batches of NB digits (one or two loads each) keep the loads in flight inside the 80-register budget of three workgroups per CU
        constexpr int NB = two_c ? 8 : 16;
        auto dig = [&](u32 el) -> u32 {
          const u32 e = ES * (PAD ? (el < ns ? el : 0u) : el);
          const u32 v = two_c ? __builtin_amdgcn_perm(ld32(w1, e), ld32(w0, e), sel) : __builtin_amdgcn_perm(0u, ld32(w0, e), sel);
          return (!PAD || el < ns) ? v : 0u;
        };
        // y = digit(el + 2^14) -> t = w y
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += NB) {
          u32 y[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) y[k] = dig((k0 + k) * A32_T + tid + A32_N);
#pragma unroll
          for (int k = 0; k < NB; ++k) r[k0 + k] = mul_lazy32(y[k], hw, p);
        }
        // x = digit(el)
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += NB) {
          u32 x[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) x[k] = dig((k0 + k) * A32_T + tid);
#pragma unroll
          for (int k = 0; k < NB; ++k) r[k0 + k] = (h & 1) == 0 ? x[k] + r[k0 + k] : x[k] + 2 * p - r[k0 + k];
        }
      };
      if (two) body(std::true_type{}); else body(std::false_type{});
    }
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k) r[k] = g[k * A32_T + tid];
  }
  // phase A: element e = k * 512 + tid; distances 16, 8, 4, 2, 1 in k; twiddles depend on the register index only
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int h = 16 >> s;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int k = a32_bfly_k(b, h);
      // (the first stage of a digit row sees the ByteDecomp digits themselves, below 2^24 < 2p: no range step)
      if (DIGITS && (S == 0 || (PAD && S == 1)) && NEGW && s == 0) a32_ct<NEGW, true, true>(r[k], r[k + h], tab[(1 << s) + (k >> (5 - s))], p);
      else a32_ct<NEGW, true>(r[k], r[k + h], tab[(1 << s) + (k >> (5 - s))], p, PB == 29 ? a32_fwd_step29(s) : 1);
    }
  }
  const u32 kq = tid >> 4, lo = tid & 15;          // sub-problem and position inside a group of 16 (after the first exchange)
  const bool upper = kq >= A32_HR;                 // waves 4..7
  // exchange 1, first pass: registers 0..15 -> rows 0..15, read by sub-problems 0..15
#pragma unroll
  for (int k = 0; k < 16; ++k) lds[k * A32_P + a32_f(tid)] = r[k];
  __syncthreads();
  u32 t[16];                                       // the upper half keeps its registers 16..31 aside while the lower half reads
#pragma unroll
  for (int k = 0; k < 16; ++k) t[k] = r[16 + k];
  if (!upper) {
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) r[k2] = lds[kq * A32_P + a32_f(k2 * 16 + lo)];
  }
  __syncthreads();
  // second pass: registers 16..31 (in t) -> the same rows, read by sub-problems 16..31
#pragma unroll
  for (int k = 0; k < 16; ++k) lds[k * A32_P + a32_f(tid)] = t[k];
  __syncthreads();
  if (upper) {
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) r[k2] = lds[(kq - A32_HR) * A32_P + a32_f(k2 * 16 + lo)];
  }
  // phase B: sub-problem kq (512 elements t = k2 * 16 + lo); distances 16 .. 1 in k2; the 2^u twiddles of stage u fetched at the stage
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int h = 16 >> u;
    Tw32 tb[16];
#pragma unroll
    for (int i = 0; i < (1 << u); ++i) tb[i] = tbl[a32_tbl_idx(u, kq, i)];
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int k2 = a32_bfly_k(b, h);
      a32_ct<NEGW>(r[k2], r[k2 + h], tb[k2 >> (5 - u)], p, PB == 29 ? a32_fwd_step29(5 + u) : 1);
    }
  }
  const u32 wv = __builtin_amdgcn_readfirstlane(tid >> 6), sub = kq & 3;      // (scalar: the store addresses below are wave-uniform up to the lane)
  __syncthreads();                                 // every read of exchange 1 is done: the rows change owner
  // exchange 2 inside the wave: rows 2w, 2w + 1; sub-problems (kq & 3) = 0, 1 first, then 2, 3
  u32* __restrict__ row = lds + (2 * wv + (sub & 1)) * A32_P;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    if ((int)(sub >> 1) == hh) {
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) row[a32_f(k2 * 16 + lo)] = r[k2];
    }
    __builtin_amdgcn_wave_barrier();
    if ((int)(sub >> 1) == hh) {
#pragma unroll
      for (int i = 0; i < 32; ++i) r[i] = row[lo * 36 + i];
    }
    __builtin_amdgcn_wave_barrier();
  }
  // phase C: this thread holds the groups k2 = 2 lo, 2 lo + 1 (32 consecutive elements); distances 8 .. 1 inside a group
  const u32 tcb = (tid & 63) * 16;                 // (the lane's 32-bit byte offset into a wave's 1 KB of twiddles: one register for all four stages)
  const __amdgpu_buffer_rsrc_t tabr = __builtin_amdgcn_make_buffer_rsrc(const_cast<Tw32*>(tab), 0, A32_N * 8, 0x00020000);
#define A32_TABC tabr
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int h = 8 >> v;
    Tw32 tc[2][8];
    A32_LOAD_TC(tc, A32_TABC, v, tid, wv, tcb);
#pragma unroll
    for (int gq = 0; gq < 2; ++gq) {
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int x = a32_bfly_k(b, h);
        a32_ct<NEGW>(r[gq * 16 + x], r[gq * 16 + x + h], tc[gq][x >> (4 - v)], p, PB == 29 ? a32_fwd_step29(10 + v) : 1);
      }
    }
  }
  // Store through the wave's two LDS rows so that every store instruction writes one whole 64-element slice (256 contiguous bytes):
  // a thread holds 32 consecutive elements, i.e. half a slice; the wave's 32 slices go out 16 at a time.  Slice t of the half sits at
  // [t * 72, t * 72 + 72): its two halves 36 words apart (the stride of exchange 2: conflict-free 16-byte writes, consecutive 4-byte reads).
  const u32 lane = tid & 63;
  u32* __restrict__ stage = lds + 2 * wv * A32_P;                  // 2 * 592 = 1184 words >= 16 * 72
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    __builtin_amdgcn_wave_barrier();
    if ((int)(sub >> 1) == hh) {
      u32* w = stage + ((sub & 1) * 8 + (lo >> 1)) * 72 + (lo & 1) * 36;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        u32 v = r[i];
        if (!DIGITS) {
          const u32 twop = 2 * p;
          if (PB == 29) v = min(v, v - 2 * twop);                  // (below 8p after the last stage)
          v = v >= twop ? v - twop : v; v = v >= p ? v - p : v;
        }
        w[i] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    const u32 pos = lane < 32 ? lane : lane + 4;                   // 36 + (lane - 32)
    // slice of the row: sub-problem kq' = 4 wv + 2 hh + (t >> 3), pair (t & 7), i.e. slices 32 wv + 16 hh + t: a running pointer with a
    // constant stride (one scalar add per store; the product form cost ten scalar instructions per store)
    // the tiled digit rows [sub-chunk][prime][slice][unit][64]: sub-chunks of ds.sub_units units keep the 256 slices a row is scattered
    // over within about a megabyte of each other however large the launch is (one tile of the whole launch measured 5 % slower at 1024
    // ciphertexts per launch: 17 MB between the slices of a row)
    i64 cnt_s = count, c_s = c, base_s = 0;
    if (DIGITS && ds.sub_units) {
      const i64 sub = div32((u32)c, ds.sub_units, ds.sub_inv), rest = count - sub * ds.sub_units;
      c_s = c - sub * ds.sub_units;
      cnt_s = rest < (i64)ds.sub_units ? rest : (i64)ds.sub_units;
      base_s = sub * ds.sub_units * (((i64)4 << (A32_LOGN - 6 + S)) * 64);
    }
    const i64 stride = DIGITS ? cnt_s * 64 : 64;
    // (the running pointer is wave-uniform -- scalar adds -- and the lane enters as a 32-bit offset: `global_store v_off, v, s[base]`; with
    // the lane inside the pointer every store cost a 64-bit vector add)
    u32* __restrict__ sp = (DIGITS ? rows + base_s + ((((i64)a << (A32_LOGN - 6 + S)) + ((i64)h << (A32_LOGN - 6)) + (32 * wv + 16 * hh)) * cnt_s + c_s) * 64 : g + (32 * wv + 16 * hh) * 64);
    const u32 lboff = lane * 4;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const u32 v = stage[t * 72 + pos];
      st32(sp, lboff, v);                      // non-temporal: rows of a large launch are read again long after they left the caches
      sp += stride;
    }
  }
}

// ---- third form of the inverse transform: the mirror of ntt32_fwd_kernel3 (half-size LDS buffer, phase-B twiddles staged in LDS,
// coalesced row loads through the wave's LDS rows); same input order, same output, same arithmetic as ntt32_inv_kernel.
// TENSOR: the rows are formed on the fly as the tensor product of two ciphertexts' evaluations (Ciphertext.cpp:179-186):
//   tsrc [nct][4][nslots][2^14] = the forward transforms of (a0, a1, b0, b1), values below p;  row c = ct * 3 + i of the output is the
//   inverse transform of  a0 b0 (i = 0),  a0 b1 + a1 b0 (i = 1),  a1 b1 (i = 2)  -- the element-wise products never touch memory.
template <bool MONT, bool TENSOR = false, class PR = Aux32Primes, int PB = 30>
__global__ void __launch_bounds__(A32_T, A32_INV_WAVES) ntt32_inv_kernel3(u32* __restrict__ rows, i64 count, int nslots, int a0, PR pr, const Tw32* __restrict__ tabs, int S,
                                                              const u32* __restrict__ tsrc) {
  static_assert(PB == 30 || (PB == 29 && !MONT), "primes below 2^29: the rows of the tensor half");
  __shared__ u32 lds[A32_HR * A32_P];
  __shared__ Tw32 tbl[A32_TBL];
  const u32 tid = threadIdx.x;
  i64 c = blockIdx.x;                             // grid (rows, prime slots x sub-blocks)
  const int ps = (int)blockIdx.y;
  if (TENSOR && count >= 24) {
    // the three rows of a ciphertext and prime read the same four source rows: same XCD (block ids 8 apart), consecutive in time
    // (grid x = groups of 8 ciphertexts x 3 rows).  Fewer than 8 ciphertexts take the plain order (grid x = rows): in the grouped one every
    // workgroup of a single ciphertext has a block id that is a multiple of 8 -- the whole launch ran on ONE XCD (47 us instead of 15)
    const u32 bid = blockIdx.x;
    const u32 grp = bid / 24, in = bid % 24;
    const i64 ct = (i64)grp * 8 + (in & 7);
    c = ct * 3 + (in >> 3);
    if (ct * 3 >= count) return;
  }
  const int slot = ps >> S, h = ps & ((1 << S) - 1), a = a0 + slot;
  const u32 p = pr.p[a];
  const Tw32* __restrict__ tab = tabs + (((i64)a << S) + h) * A32_N;
  u32* __restrict__ g = rows + (((c * nslots + slot) << S) + h) * A32_N;
  // (the wave index as a scalar makes the row addresses scalar arithmetic; in the TENSOR variant the register allocation spills with it)
  const u32 kq = tid >> 4, lo = tid & 15, wv = TENSOR ? tid >> 6 : __builtin_amdgcn_readfirstlane(tid >> 6), sub = kq & 3, lane = tid & 63;
  const bool upper = kq >= A32_HR;
  a32_stage_tbl(tbl, tab, tid);
  u32 r[32];
  // load: every instruction reads one whole 64-element slice; through the wave's two LDS rows each thread ends up with its 32
  // consecutive elements (the reverse of the forward kernel's store)
  u32* __restrict__ stage = lds + 2 * wv * A32_P;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const u32 pos = lane < 32 ? lane : lane + 4;
    u32 v[16];
    if constexpr (TENSOR) {
      const i64 ct = c / 3;
      const int comp = (int)(c - ct * 3);
      auto srow = [&](int jj) { return tsrc + (((((ct * 4 + jj) * nslots + slot)) << S) + h) * A32_N; };       // (sub-row h of a 2^15-point row)
      const u32* __restrict__ sa = srow(comp == 2 ? 1 : 0);      // a0 (rows 0, 1) or a1 (row 2)
      const u32* __restrict__ sb = srow(comp == 0 ? 2 : 3);      // b0 (row 0) or b1 (rows 1, 2)
      const u32 mu = pr.mu61[a], twop = 2 * p;
      // v < 2^61 (2^60: PB = 29, two products of values below p < 2^29) -> [0, 2p): quotient from the top 32 bits and floor(2^61 / p) (2^60), at most 2 below the true one
      auto red = [&](u64 x) -> u32 {
        const u32 q = __umulhi((u32)(x >> (PB == 29 ? 28 : 29)), mu);
        const u32 r = (u32)x - q * p;
        return r >= twop ? r - twop : r;
      };
      if (comp == 1) {
        const u32* __restrict__ sc = srow(1);      // a1
        const u32* __restrict__ sd = srow(2);      // b0
#pragma unroll
        for (int t0 = 0; t0 < 16; t0 += 8) {
          u32 x0[8], y1[8], x1[8], y0[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const u32 off = ((4 * wv + 2 * hh + ((t0 + t) >> 3)) * 8 + ((t0 + t) & 7)) * 64 + lane;
            x0[t] = sa[off]; y1[t] = sb[off]; x1[t] = sc[off]; y0[t] = sd[off];
          }
#pragma unroll
          for (int t = 0; t < 8; ++t) v[t0 + t] = red((u64)x0[t] * y1[t] + (u64)x1[t] * y0[t]);
        }
      } else {
        u32 x[16], y[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const u32 off = ((4 * wv + 2 * hh + (t >> 3)) * 8 + (t & 7)) * 64 + lane;
          x[t] = sa[off]; y[t] = sb[off];
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = red((u64)x[t] * y[t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) v[t] = g[((4 * wv + 2 * hh + (t >> 3)) * 8 + (t & 7)) * 64 + lane];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 16; ++t) stage[t * 72 + pos] = v[t];
    __builtin_amdgcn_wave_barrier();
    if ((int)(sub >> 1) == hh) {
      const u32* w = stage + ((sub & 1) * 8 + (lo >> 1)) * 72 + (lo & 1) * 36;
#pragma unroll
      for (int i = 0; i < 32; ++i) r[i] = w[i];
    }
  }
  // phase C (mirror): distances 1 .. 8 inside the two groups of 16; per-lane twiddles fetched stage by stage
  const u32 tcb = lane * 16, wvs = __builtin_amdgcn_readfirstlane(tid >> 6);
  const __amdgpu_buffer_rsrc_t tabr = __builtin_amdgcn_make_buffer_rsrc(const_cast<Tw32*>(tab), 0, A32_N * 8, 0x00020000);
#pragma unroll
  for (int v = 3; v >= 0; --v) {
    const int h = 8 >> v;
    Tw32 tc[2][8];
    A32_LOAD_TC(tc, A32_TABC, v, tid, wvs, tcb);
#pragma unroll
    for (int gq = 0; gq < 2; ++gq) {
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int x = a32_bfly_k(b, h);
        // (MONT rows come from dot32_kernel2 / dot32_kernel3, fully reduced: the first stage's sums stay below 2p by themselves)
        if (MONT && !TENSOR && v == 3) a32_gs<true>(r[gq * 16 + x], r[gq * 16 + x + h], tc[gq][x >> (4 - v)], p);
        else if (PB == 29) a32_gs29(r[gq * 16 + x], r[gq * 16 + x + h], tc[gq][x >> (4 - v)], p, v == 3 || (x & (h >> 1)) != 0);      // (the rows enter below 2p)
        else a32_gs(r[gq * 16 + x], r[gq * 16 + x + h], tc[gq][x >> (4 - v)], p);
      }
    }
  }
  // exchange 2 (mirror) inside the wave, two sub-problems at a time through the wave's two rows
  {
    u32* __restrict__ row = lds + (2 * wv + (sub & 1)) * A32_P;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      __builtin_amdgcn_wave_barrier();
      if ((int)(sub >> 1) == hh) {
#pragma unroll
        for (int i = 0; i < 32; ++i) row[lo * 36 + i] = r[i];
      }
      __builtin_amdgcn_wave_barrier();
      if ((int)(sub >> 1) == hh) {
#pragma unroll
        for (int k2 = 0; k2 < 32; ++k2) r[k2] = row[a32_f(k2 * 16 + lo)];
      }
    }
  }
  __syncthreads();                                 // the phase-B table is complete (and the rows change owner below)
  // phase B (mirror): twiddles from the LDS table
#pragma unroll
  for (int u = 4; u >= 0; --u) {
    const int h = 16 >> u;
    Tw32 tb[16];
#pragma unroll
    for (int i = 0; i < (1 << u); ++i) tb[i] = tbl[a32_tbl_idx(u, kq, i)];
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int k2 = a32_bfly_k(b, h);
      if (PB == 29) a32_gs29(r[k2], r[k2 + h], tb[k2 >> (5 - u)], p, u != 4 && (k2 & (h >> 1)) != 0);
      else a32_gs(r[k2], r[k2 + h], tb[k2 >> (5 - u)], p);
    }
  }
  // exchange 1 (mirror) in two passes: sub-problems 0..15 write their rows, everyone reads registers 0..15; then sub-problems 16..31
  u32 t[16];
  if (!upper) {
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) lds[kq * A32_P + a32_f(k2 * 16 + lo)] = r[k2];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) t[k] = lds[k * A32_P + a32_f(tid)];
  __syncthreads();
  if (upper) {
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) lds[(kq - A32_HR) * A32_P + a32_f(k2 * 16 + lo)] = r[k2];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) r[16 + k] = lds[k * A32_P + a32_f(tid)];
  // (registers 0..15 of phase A are the values read in the first pass: named through R() instead of copied back into r[])
#define R(k) ((k) < 16 ? t[(k)] : r[(k)])
  // phase A (mirror): distances 1 .. 16 in the register index, uniform twiddles.  The last stage (distance 16, ONE twiddle w) carries the final
  // scaling: X' = (X + Y) c, Y' = (X - Y) (w c) with c = 1/n (or 2^32 / n: MONT) -- two multiplications by constants per pair instead of
  // the butterfly's product followed by 32 scalings; c and w c sit in the table's entries 0 and 1 (no stage uses index 0), the MONT pair
  // with the primes.
#pragma unroll
  for (int s2 = 4; s2 >= 1; --s2) {
    const int h = 16 >> s2;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int k = a32_bfly_k(b, h);
      if (PB == 29) a32_gs29<true>(R(k), R(k + h), tab[(1 << s2) + (k >> (5 - s2))], p, s2 != 4 && (k & (h >> 1)) != 0);
      else a32_gs<false, true>(R(k), R(k + h), tab[(1 << s2) + (k >> (5 - s2))], p);
    }
  }
  Tw32 tn, tnw;
  if constexpr (MONT) { tn = Tw32{pr.ninv_m[a], pr.ninv_m_p[a]}; tnw = Tw32{pr.ninv_mw[a][h], pr.ninv_mw_p[a][h]}; }
  else if constexpr (std::is_same<PR, T32Primes>::value) {
    // the tensor half: the configuration's own pair (rows of 2^14: the CRT constant travels with 1/n), or the table's 1/n (longer rows)
    if (pr.closing) { tn = Tw32{pr.ninv[a], pr.ninv_p[a]}; tnw = Tw32{pr.ninv_w[a], pr.ninv_w_p[a]}; } else { tn = tab[0]; tnw = tab[1]; }
  }
  else { tn = tab[0]; tnw = tab[1]; }
  auto mulc = [&](u32 y, Tw32 t) -> u32 {            // y any 32-bit value -> [0, 2p): quotient estimate, then y w - Q p as two chained multiply-adds
    const u32 Q = __umulhi(y, t.wp);
    return (u32)mad64(Q, 0u - p, mul64_s(y, t.w));
  };
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    // both below 4p (PB = 29: below 8p -- registers k with bit 3 set are product outputs of the stage before, the others sums below 4p)
    const u32 sm = t[k] + r[k + 16], df = t[k] - r[k + 16] + ((PB == 29 && !(k & 8)) ? 4 * p : 2 * p);
    u32 v0 = mulc(sm, tn), v1 = mulc(df, tnw);
    v0 = min(v0, v0 - p); v1 = min(v1, v1 - p);
    g[k * A32_T + tid] = v0;
    g[(k + 16) * A32_T + tid] = v1;
  }
#undef R
}
