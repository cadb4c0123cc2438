// kernels_ct.hip -- coefficient-domain ciphertext algebra on batches that stay in HBM: the pieces of Ciphertext.cpp that
// Matrix<Ciphertext> (Matrix.cpp) and Regression::Regress (Regression.h:102-149) call between multiplications.
//
// Unscaled ciphertext parts are [count][nparts][phi(m)][nlimbs] two's complement coefficients (centred mod 2^logQ); scaled-up
// ciphertexts (tProd) are residue rows [count][3][L][phi(m)].  All kernels are streaming (HBM-bound) integer work.
#include "fhesi_internal.h"

// (the multi-limb steps -- sum with carry, multiply by a word, negation, the centred store of Reduce, Util.cpp:3-26 -- are ct_wide.h's)
// Ciphertext::operator+= for unscaled ciphertexts (Ciphertext.cpp:123-134): parts[i] += other.parts[i]; ReduceCoefficients
template <int MAXNL>
__global__ void __launch_bounds__(256) ct_add_kernel(u64* __restrict__ dst, const u64* __restrict__ src, i64 ncoeffs, int nl, int logQ) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncoeffs) return;
  u64 x[MAXNL];
  ctw_sum(x, nl, 0, [=](int i) { return dst[j * nl + i]; }, [=](int i) { return src[j * nl + i]; });
  ctw_store_centred(x, nl, logQ, dst + j * nl);
}

// CiphertextPart::operator*=(long) (Ciphertext.cpp:21-27): coefficient * l, Reduce.  Two's complement product mod 2^(64 nl)
// (exact modulo 2^logQ, which divides it), then the centred residue.
template <int MAXNL>
__global__ void __launch_bounds__(256) ct_mul_long_kernel(u64* __restrict__ ct, i64 ncoeffs, int nl, int logQ, u64 mag, int negate) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncoeffs) return;
  u64 x[MAXNL];
  ctw_muladd(x, nl, CtwNone{}, [=](int i) { return ct[j * nl + i]; }, mag);
  if (negate) ctw_neg(x, nl);
  ctw_store_centred(x, nl, logQ, ct + j * nl);
}

static int limbs_ok(const char* who, int nl) {
  if (nl > 32) FHESI_FAIL("%s of %d limbs exceed the supported 32", who, nl);
  return 0;
}
int launch_ct_add(fhesi_ctx* ctx, u64* d_dst, const u64* d_src, i64 ncoeffs, int nl, int logQ) {
  if (!ncoeffs) return 0;
  FHESI_TRY(limbs_ok("ciphertext coefficients", nl));
  const unsigned grid = (unsigned)((ncoeffs + 255) / 256);
  with_limb_class<2, 8, 16, 32>(nl, [&](auto C) { ct_add_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_dst, d_src, ncoeffs, nl, logQ); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- Ciphertext::operator>>= on the coefficients themselves.
// The reference takes X -> X^k in evaluation form (DoubleCRT::automorph, DoubleCRT.cpp:439-465, between DoubleCRT(poly) and toPoly:
// Ciphertext.cpp:54-59); its result is the INTEGER polynomial a(X^k) mod Phi_m (the coefficients, at most two input coefficients
// added, stay far below half the chain product).  On the rings below that polynomial is a signed gather:
//   m = 2n (power of two):  X^n = -1:              out_i = +-a_j,  j k = i or i + n (mod 2n)
//   m = 2Q, Q = q^k, q an odd prime (k = 1: the reference's safe-prime rings), s = q^(k-1), phi = Q - s:  X^Q = -1 modulo X^Q + 1,
//       R_e = +-a_j with j k = e (mod Q), sign - when j k mod 2Q >= Q;  out_i = R_i - (-1)^floor(i/s) R_(phi + i mod s)   (Phi_m = sum_{i<q} (-X^s)^i, monic)
//   m = Q odd, phi = m - s:   X^m = 1,  R_e = a_j with j k = e (mod m);  out_i = R_i - R_(phi + i mod s)   (Phi_m = sum_{i<q} X^(i s))
//   (a_j = 0 for j >= phi.  s = 1: the fixed top phi = q' - 1 or m - 1 and the sign (-1)^i.)  Each output is at most two signed source coefficients,
// so no row transform is needed at all: out = positive residue modulo 2^logQ, limb-major, as ByteDecompPart takes it (Ciphertext.cpp:94).
// mode: 0 power of two, 1 m = 2 q^k, 2 m = q^k; st = the stride s.  in [npolys][n][nl_in] two's complement;  out [npolys][nlq][n] (logQ > 0), or the
// integers themselves, sign-extended, coefficient-major [npolys][n][nlq] (logQ = 0: toPoly of Ciphertext >>= without a key switch).
// The sources of output coefficient i of a(X^k) mod Phi_m: term 1 is s1 a[j1], term 2 is s2 a[j2]  (s = 0: absent, its j = 0).  kk, kinv = k, k^-1 mod m.
__device__ __forceinline__ void automorph_sources(i64 i, i64 n, i64 m, i64 kk, i64 kinv, int mode, i64 st, i64& j1, int& s1, i64& j2, int& s2) {
  j1 = 0; j2 = 0;
  s1 = 0; s2 = 0;
  if (mode == 0) {
    const i64 j = (i64)(((u128)i * (u128)kinv) % (u128)m);          // j k = i (mod 2n)
    j1 = j < n ? j : j - n;
    s1 = j < n ? 1 : -1;
  } else if (mode == 1) {
    const i64 q = m / 2;
    const u32 b = st == 1 ? (u32)i : (u32)i / (u32)st;              // floor(i / s); i and s are below 2^20
    auto term = [&](i64 e, i64& j, int& sg) {                        // the a_j with j k = e (mod Q), and its sign
      j = (i64)(((u128)e * (u128)(kinv % q)) % (u128)q);
      if (j >= n) { sg = 0; j = 0; return; }
      sg = ((i64)(((u128)j * (u128)kk) % (u128)m) >= q) ? -1 : 1;
    };
    term(i, j1, s1);
    term(n + ((u32)i - b * (u32)st), j2, s2);
    s2 = (b & 1) ? s2 : -s2;                                        // - (-1)^floor(i/s) R_(phi + i mod s)
  } else {
    const u32 b = st == 1 ? (u32)i : (u32)i / (u32)st;
    auto term = [&](i64 e, i64& j, int& sg) {
      j = (i64)(((u128)e * (u128)kinv) % (u128)m);
      sg = j >= n ? 0 : 1;
      if (!sg) j = 0;
    };
    term(i, j1, s1);
    term(n + ((u32)i - b * (u32)st), j2, s2);
    s2 = -s2;
  }
}
__global__ void __launch_bounds__(256) ct_automorph_parts_kernel(const u64* __restrict__ in, i64 n, int nl_in, i64 m, i64 kk, i64 kinv, int mode, i64 st,
                                                                 int logQ, u64* __restrict__ out, int nlq) {
  const i64 poly = blockIdx.y;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  i64 j1, j2;
  int s1, s2;
  automorph_sources(i, n, m, kk, kinv, mode, st, j1, s1, j2, s2);
  const u64* __restrict__ a1 = in + (poly * n + j1) * nl_in;
  const u64* __restrict__ a2 = in + (poly * n + j2) * nl_in;
  const u64 ext1 = (a1[nl_in - 1] >> 63) ? ~0ull : 0ull, ext2 = (a2[nl_in - 1] >> 63) ? ~0ull : 0ull;
  u64 carry = ctw_neg_carry(s1, s2);
  u64* __restrict__ o = logQ ? out + poly * nlq * n + i : out + (poly * n + i) * nlq;
  for (int w = 0; w < nlq; ++w) {
    const u64 x1 = ctw_signed(w < nl_in ? a1[w] : ext1, s1), x2 = ctw_signed(w < nl_in ? a2[w] : ext2, s2);
    const u128 sum = (u128)x1 + x2 + carry;
    u64 v = (u64)sum;
    carry = (u64)(sum >> 64);
    if (logQ) {
      const int bits_left = logQ - 64 * w;
      if (bits_left < 64) v &= ((u64)1 << bits_left) - 1;      // (reduce_limb's rule, spelled out: through it the kernel timed above the parent, profiles/ct_wide_refactor_ab.txt)
      o[(i64)w * n] = v;
    } else o[w] = v;
  }
}
// which signed gather the ring has: mode 0 power of two, 1 m = 2 q^k, 2 m = q^k, st = the stride q^(k-1); false: none
static bool ring_gather(const fhesi_ctx* ctx, int* mode, i64* st) {
  const i64 m = ctx->m;
  *st = 1;
  if (ctx->pow2) { *mode = 0; return true; }
  const i64 qq = hm::prime_power_ring(m, nullptr);
  if (!qq) return false;
  *mode = (m & 1) ? 2 : 1;
  *st = ((m & 1) ? m : m / 2) / qq;
  return true;
}
// (k mod m, k^-1 mod m) of an automorphism, both in [0, m)
static int gather_key(const fhesi_ctx* ctx, i64 k, i64* kk, i64* kinv) {
  *kk = ((k % ctx->m) + ctx->m) % ctx->m;
  *kinv = hm::inv_mod(k, ctx->m);
  if (!*kinv) FHESI_FAIL("automorph: k=%lld is not in Zm*", (long long)k);
  return 0;
}
// 0 = launched; 2 = this ring / exponent is not covered (the caller keeps the evaluation-form path)
int launch_ct_automorph_parts(fhesi_ctx* ctx, const u64* d_in, int nl_in, i64 npolys, i64 kk, int logQ, u64* d_parts, int nlq) {
  const i64 m = ctx->m, n = ctx->phim;
  int mode;
  i64 st, kinv;
  if (!ring_gather(ctx, &mode, &st)) return 2;
  if (!npolys) return 0;
  FHESI_TRY(grid_y_ok("automorph", "polynomials per call", npolys));
  FHESI_TRY(gather_key(ctx, kk, &kk, &kinv));
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)npolys);
  ct_automorph_parts_kernel<<<grid, 256, 0, ctx->stream>>>(d_in, n, nl_in, m, kk, kinv, mode, st, logQ, d_parts, nlq);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- a sum of rotated ciphertexts, out = Reduce_logQ(base + sum_t sigma_{k_t}(pre_t)): the closing step of a baby-step/giant-step matrix-vector
// product (fhesi_ct_matvec_bsgs_dev).  Every term is the signed gather above, summed in registers in two's complement modulo 2^(64 nl)
// (exact modulo 2^logQ, which divides it), then ONE centred reduction as ct_add_kernel does it: one read per term and one write, where the composition
// (gather, reduction, addition per term) makes about seven passes.  The (k, k^-1) pairs travel in the argument segment: nothing is uploaded in front of
// the launch.  pre_t = pre + t * term_stride, [npolys][n][nl]; base (null: none) and out [npolys][n][nl].  A thread reads base and writes out at its own
// coefficient only, so out may be base (which is why neither is __restrict__); out must not overlap pre.
struct RotSumKeys { static constexpr int MAX = kRotSumMax; i64 k[MAX], kinv[MAX]; };
template <int MAXNL>
__global__ void __launch_bounds__(256) ct_rot_sum_kernel(const RotSumKeys keys, int nt, const u64* base, const u64* __restrict__ pre, i64 term_stride, i64 n, int nl,
                                                         i64 m, int mode, i64 st, int logQ, u64* out) {
  const i64 poly = blockIdx.y;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const i64 at = (poly * n + i) * nl;
  u64 x[MAXNL];
#pragma unroll
  for (int w = 0; w < MAXNL; ++w) x[w] = (base && w < nl) ? base[at + w] : 0;
  for (int t = 0; t < nt; ++t) {
    i64 j1, j2;
    int s1, s2;
    automorph_sources(i, n, m, keys.k[t], keys.kinv[t], mode, st, j1, s1, j2, s2);
    const u64* __restrict__ a1 = pre + t * term_stride + (poly * n + j1) * nl;
    const u64* __restrict__ a2 = pre + t * term_stride + (poly * n + j2) * nl;
    u64 carry = ctw_neg_carry(s1, s2);
#pragma unroll
    for (int w = 0; w < MAXNL; ++w)
      if (w < nl) {
        const u128 sum = (u128)x[w] + ctw_signed(a1[w], s1) + ctw_signed(a2[w], s2) + carry;
        x[w] = (u64)sum;
        carry = (u64)(sum >> 64);
      }
  }
  ctw_store_centred(x, nl, logQ, out + at);
}
// 0 = launched (nk > kRotSumMax terms: a chain of launches with base = out); 2 = this ring is not covered (the caller runs the composition).
// ks in Z_m^* and nl >= 1 holding logQ: checked by the caller.
int launch_ct_rot_sum(fhesi_ctx* ctx, const i64* ks, int nk, int logQ, const u64* d_base, const u64* d_pre, i64 term_stride, i64 npolys, int nl, u64* d_out) {
  const i64 m = ctx->m, n = ctx->phim;
  int mode;
  i64 st;
  if (!ring_gather(ctx, &mode, &st)) return 2;
  if (!npolys || nk < 1) return 0;
  if (nl < 1 || nl > 32) FHESI_FAIL("ciphertext coefficients of %d limbs exceed the supported 32", nl);
  FHESI_TRY(grid_y_ok("ct_rot_sum", "polynomials per call", npolys));
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)npolys);
  for (int t0 = 0; t0 < nk; t0 += kRotSumMax) {
    const int nt = nk - t0 < kRotSumMax ? nk - t0 : kRotSumMax;
    RotSumKeys keys{};
    for (int t = 0; t < nt; ++t) FHESI_TRY(gather_key(ctx, ks[t0 + t], &keys.k[t], &keys.kinv[t]));
    const u64* base = t0 ? d_out : d_base;
    const u64* pre = d_pre + (i64)t0 * term_stride;
    with_limb_class<2, 8, 16, 32>(nl, [&](auto C) {
      ct_rot_sum_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(keys, nt, base, pre, term_stride, n, nl, m, mode, st, logQ, d_out);
    });
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int launch_ct_mul_long(fhesi_ctx* ctx, u64* d_ct, i64 ncoeffs, int nl, int logQ, i64 l) {
  if (!ncoeffs) return 0;
  FHESI_TRY(limbs_ok("ciphertext coefficients", nl));
  const u64 mag = l < 0 ? (u64)(-(l + 1)) + 1 : (u64)l;
  const int neg = l < 0;
  const unsigned grid = (unsigned)((ncoeffs + 255) / 256);
  with_limb_class<2, 8, 16, 32>(nl, [&](auto C) { ct_mul_long_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_ct, ncoeffs, nl, logQ, mag, neg); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- Ciphertext::operator+=(const ZZX&) on unscaled ciphertexts (Ciphertext.cpp:147-156): scaledConstant_j = (other_j << logQ) / p
// with NTL's floor division (ctw_floor_quotient), parts[0] += scaledConstant, ReduceCoefficients.  poly: [npoly][n] machine-word coefficients (npoly = 1:
// one constant for the whole batch).  Only the quotient modulo 2^logQ matters.
template <int MAXNL>
__global__ void __launch_bounds__(256) ct_add_const_kernel(u64* __restrict__ ct, const i64* __restrict__ poly, int npoly, i64 n, int nparts, int nl, int logQ,
                                                           u64 p) {
  const i64 c = blockIdx.y;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  u64 q[MAXNL];
  ctw_floor_quotient(q, poly[(npoly == 1 ? 0 : c) * n + j], logQ, p);
  u64* x0 = ct + ((c * nparts) * n + j) * nl;                     // part 0 of ciphertext c
  u64 x[MAXNL];
  ctw_sum(x, nl, 0, [=](int i) { return x0[i]; }, [&](int i) { return q[i]; });
  ctw_store_centred(x, nl, logQ, x0);
}
int launch_ct_add_const(fhesi_ctx* ctx, u64* d_ct, const i64* d_poly, int npoly, int nparts, int nl, int logQ, u64 p, i64 count) {
  if (!count) return 0;
  FHESI_TRY(limbs_ok("ciphertext coefficients", nl));
  FHESI_TRY(grid_y_ok("Ciphertext += ZZX", "ciphertexts per call", count));
  const dim3 grid((unsigned)((ctx->phim + 255) / 256), (unsigned)count);
  // (the quotient needs limbs 0 .. logQ / 64 + 1 <= nl + 1: the class of nl + 2 holds them)
  with_limb_class<4, 8, 16, 34>(nl + 2, [&](auto C) {
    ct_add_const_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_ct, d_poly, npoly, ctx->phim, nparts, nl, logQ, p);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- scalar linear combinations with a constant, out[g] = Reduce_logQ(sum_t coef[t] pool[idx[t]] + konst[g]) (fhesi_ct_lin_comb_dev, include/fhesi_hip.h): what
// the composition -- a copy, Ciphertext *= long and Ciphertext += per term, Ciphertext += ZZX -- makes in three passes per term, in one read per term and one
// write.  A thread owns one coefficient of one polynomial of one group and sums in registers (ctw_lin_comb).  The lists are the host's (lin_comb_lists,
// poly_plan.h), in device memory and read at block-uniform addresses: idx, mag per term, the negative coefficients of a group first; bounds[3 g ..] = first
// term, first positive term, end; konst [ngroups] or null.  The constant goes to coefficient 0 of part 0.  poly0: the first polynomial (2 g + part) of this launch.
template <int MAXNL>
__global__ void __launch_bounds__(256) ct_lin_comb_kernel(const u64* __restrict__ pool, const int* __restrict__ idx, const u64* __restrict__ mag,
                                                          const int* __restrict__ bounds, const i64* __restrict__ konst, i64 poly0, i64 n, int nl, int logQ, u64 p,
                                                          u64* __restrict__ out) {
  const i64 poly = poly0 + blockIdx.y, g = poly >> 1, part = poly & 1;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int t0 = bounds[3 * g], ts = bounds[3 * g + 1], t1 = bounds[3 * g + 2];
  const i64 cv = konst ? konst[g] : 0;
  u64 x[MAXNL];
  ctw_lin_comb(x, nl, mag, t0, ts, t1, [=](int t) {
    const u64* __restrict__ a = pool + (((i64)idx[t] * 2 + part) * n + j) * nl;
    return [=](int i) { return a[i]; };
  }, cv != 0 && part == 0 && j == 0, cv, logQ, p);
  ctw_store_centred(x, nl, logQ, out + (poly * n + j) * nl);
}
// idx < the pool's size, nl in 1..32 holding logQ, out apart from pool: checked by the caller
int launch_ct_lin_comb(fhesi_ctx* ctx, const u64* d_pool, const int* d_idx, const u64* d_mag, const int* d_bounds, const i64* d_konst, i64 ngroups, int nl, int logQ,
                       u64 p, u64* d_out) {
  if (!ngroups) return 0;
  FHESI_TRY(limbs_ok("ciphertext coefficients", nl));
  const unsigned gx = (unsigned)((ctx->phim + 255) / 256);
  grid_chunks(ngroups * 2, [&](i64 done, i64 cnt) {
    with_limb_class<2, 8, 16, 32>(nl, [&](auto C) {
      ct_lin_comb_kernel<decltype(C)::value><<<dim3(gx, (unsigned)cnt), 256, 0, ctx->stream>>>(d_pool, d_idx, d_mag, d_bounds, d_konst, done, ctx->phim, nl, logQ, p, d_out);
    });
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- gather: out[i] = pool[idx[i]], `words` u64 per element (operands of one wave of Matrix products)
__global__ void __launch_bounds__(256) gather_kernel(const u64* __restrict__ pool, const int* __restrict__ idx, u64* __restrict__ out, i64 words) {
  const u64* __restrict__ s = pool + (i64)idx[blockIdx.y] * words;
  u64* __restrict__ d = out + (i64)blockIdx.y * words;
  for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (i64)gridDim.x * blockDim.x) d[w] = s[w];
}
int launch_gather(fhesi_ctx* ctx, const u64* d_pool, const int* d_idx, i64 count, i64 words, u64* d_out) {
  if (!count || !words) return 0;
  unsigned gx = (unsigned)((words + 255) / 256);
  if (gx > 256) gx = 256;
  grid_chunks(count, [&](i64 done, i64 cnt) { gather_kernel<<<dim3(gx, (unsigned)cnt), 256, 0, ctx->stream>>>(d_pool, d_idx + done, d_out + done * words, words); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- segmented sum of scaled-up ciphertexts: out[g] = sum_{t in [seg[g], seg[g+1])} in[t]  (the `newMatrix(i,j) += tmp` loops of
// Matrix.cpp:62-72,157-167 and `det += tmp` of :243; Ciphertext::operator+= on tProd, Ciphertext.cpp:135-142 -> DoubleCRT +=)
__global__ void __launch_bounds__(256) segment_sum_kernel(const u64* __restrict__ in, const int* __restrict__ seg, u64* __restrict__ out, int ncomp_L,
                                                          i64 n, const PrimeConst* __restrict__ pcs, int L) {
  const int g = blockIdx.z, r = blockIdx.y;       // r = comp * L + prime
  const u64 q = pcs[r % L].q;
  const i64 ct_words = (i64)ncomp_L * n;
  const int t0 = seg[g], t1 = seg[g + 1];
  for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) {
    u64 acc = 0;
    for (int t = t0; t < t1; ++t) {
      acc += in[(i64)t * ct_words + (i64)r * n + j];
      if (acc >= q) acc -= q;
    }
    out[(i64)g * ct_words + (i64)r * n + j] = acc;
  }
}
int launch_segment_sum(fhesi_ctx* ctx, const u64* d_in, const int* d_seg, i64 ngroups, int ncomp, u64* d_out) {
  if (!ngroups) return 0;
  unsigned gx = (unsigned)((ctx->phim + 255) / 256);
  if (gx > 64) gx = 64;
  grid_chunks(ngroups, [&](i64 done, i64 cnt) {
    segment_sum_kernel<<<dim3(gx, (unsigned)(ncomp * ctx->L), (unsigned)cnt), 256, 0, ctx->stream>>>(
        d_in, d_seg + done, d_out + done * ncomp * ctx->L * ctx->phim, ncomp * ctx->L, ctx->phim, ctx->d_pc, ctx->L);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- FHESIPubKey::Encrypt (FHE-SI.cpp:26-27): ct[i] = pk[i] * r + e[i]  for i = 0,1, all in evaluation form.
// rows: [count][3][L][n] = (r, e0*p, e1*p); pk: [2][L][n]; out: [count][2][L][n]
__global__ void __launch_bounds__(256) encrypt_combine_kernel(const u64* __restrict__ rows, const u64* __restrict__ pk, u64* __restrict__ out, int L, i64 n,
                                                              const PrimeConst* __restrict__ pcs) {
  const i64 c = blockIdx.z;
  const int l = blockIdx.y;
  const PrimeConst pc = pcs[l];
  const u64* r = rows + ((c * 3 + 0) * L + l) * n;
  for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) {
    const u64 rv = r[j];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const u64 e = rows[((c * 3 + 1 + i) * L + l) * n + j];
      out[((c * 2 + i) * L + l) * n + j] = d_addmod(d_mulmod(pk[((i64)i * L + l) * n + j], rv, pc), e, pc.q);
    }
  }
}
int launch_encrypt_combine(fhesi_ctx* ctx, const u64* d_rows, const u64* d_pk, i64 count, u64* d_out) {
  if (!count) return 0;
  unsigned gx = (unsigned)((ctx->phim + 255) / 256);
  if (gx > 64) gx = 64;
  grid_chunks(count, [&](i64 done, i64 cnt) {
    encrypt_combine_kernel<<<dim3(gx, (unsigned)ctx->L, (unsigned)cnt), 256, 0, ctx->stream>>>(d_rows + done * 3 * ctx->L * ctx->phim, d_pk,
                                                                                               d_out + done * 2 * ctx->L * ctx->phim, ctx->L, ctx->phim, ctx->d_pc);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- ctxt[0] += delta * msg; ReduceCoefficients (FHE-SI.cpp:31-35).  ct: [count][2][n][nl]; msg: [count][n] small non-negative;
// delta = floor(2^logQ / p) as nl limbs.  The product is taken modulo 2^(64 nl), exact modulo 2^logQ.
template <int MAXNL>
__global__ void __launch_bounds__(256) add_scaled_msg_kernel(u64* __restrict__ ct, const i64* __restrict__ msg, const u64* __restrict__ delta, i64 n, int nl,
                                                             int logQ) {
  const i64 c = blockIdx.y;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  u64* x = ct + ((c * 2) * n + j) * nl;
  u64 v[MAXNL];
  ctw_muladd(v, nl, [=](int i) { return x[i]; }, [=](int i) { return delta[i]; }, (u64)msg[c * n + j]);
  ctw_store_centred(v, nl, logQ, x);
}
int launch_add_scaled_msg(fhesi_ctx* ctx, u64* d_ct, const i64* d_msg, const u64* d_delta, i64 count, int nl, int logQ) {
  if (!count) return 0;
  FHESI_TRY(limbs_ok("ciphertext coefficients", nl));
  FHESI_TRY(grid_y_ok("Encrypt", "plaintexts per call", count));
  const dim3 grid((unsigned)((ctx->phim + 255) / 256), (unsigned)count);
  with_limb_class<2, 8, 16, 32>(nl, [&](auto C) { add_scaled_msg_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_ct, d_msg, d_delta, ctx->phim, nl, logQ); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- FHESISecKey::Decrypt (FHE-SI.cpp:105-107): z = c0 + c1 * t in evaluation form.  rows: [count][2][L][n]; t: [L][n]; out [count][L][n]
__global__ void __launch_bounds__(256) decrypt_dot_kernel(const u64* __restrict__ rows, const u64* __restrict__ t, u64* __restrict__ out, int L, i64 n,
                                                          const PrimeConst* __restrict__ pcs) {
  const i64 c = blockIdx.z;
  const int l = blockIdx.y;
  const PrimeConst pc = pcs[l];
  for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x)
    out[(c * L + l) * n + j] = d_addmod(rows[((c * 2) * L + l) * n + j], d_mulmod(rows[((c * 2 + 1) * L + l) * n + j], t[(i64)l * n + j], pc), pc.q);
}
int launch_decrypt_dot(fhesi_ctx* ctx, const u64* d_rows, const u64* d_t, i64 count, u64* d_out) {
  if (!count) return 0;
  unsigned gx = (unsigned)((ctx->phim + 255) / 256);
  if (gx > 64) gx = 64;
  grid_chunks(count, [&](i64 done, i64 cnt) {
    decrypt_dot_kernel<<<dim3(gx, (unsigned)ctx->L, (unsigned)cnt), 256, 0, ctx->stream>>>(d_rows + done * 2 * ctx->L * ctx->phim, d_t,
                                                                                           d_out + done * ctx->L * ctx->phim, ctx->L, ctx->phim, ctx->d_pc);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the rounding of Decrypt (FHE-SI.cpp:110-116): m = floor((2 p z + q) / (2 q)) mod p, q = 2^logQ (round_product, round_quotient: ct_wide.h).
// z: [npolys][n][nw] two's complement truncated to nw = ceil((logQ+1)/64) limbs; out: [npolys][n]
template <int MAXNL>
__global__ void __launch_bounds__(256) decrypt_round_kernel(const u64* __restrict__ z, i64 total, int nw, int logQ, u64 p, i64* __restrict__ out) {
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  u64 P[MAXNL];
  u64 carry;
  round_product(z, j, nw, logQ, p, P, carry);
  out[j] = (i64)(round_quotient(P, carry, nw, logQ) % p);
}
int launch_decrypt_round(fhesi_ctx* ctx, const u64* d_z, i64 total, int nw, int logQ, u64 p, i64* d_out) {
  if (!total) return 0;
  if (nw > 32) FHESI_FAIL("Decrypt: logQ=%d exceeds the supported 2047 bits", logQ);
  const unsigned grid = (unsigned)((total + 255) / 256);
  with_limb_class<2, 9, 17, 32>(nw, [&](auto C) { decrypt_round_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_z, total, nw, logQ, p, d_out); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the noise of a ciphertext, from the same product: the maximum over the coefficients of |r|, r = (2 p z + q) mod 2q - q (round_residual, ct_wide.h).
// Exact maximum of the block's nw-limb values without a multi-limb shuffle: the limbs are walked from the top, each round takes the 64-bit
// maximum over the threads still level with the maximum so far (wave64 shuffles, then LDS across the waves), and the threads below it drop out.
// Ties are harmless: tied threads hold the same limbs.  Thread 0 writes the nw limbs to `out`; every thread returns the maximum's bit length.
template <int MAXNL, int NWAVES>
__device__ __forceinline__ int block_limb_max(const u64 (&a)[MAXNL], int nw, u64* __restrict__ out) {
  __shared__ u64 s[MAXNL][NWAVES];
  bool level = true;
  int bitlen = 0;
#pragma unroll
  for (int i = MAXNL - 1; i >= 0; --i)
    if (i < nw) {
      u64 v = level ? a[i] : 0;
#pragma unroll
      for (int o = 32; o; o >>= 1) { const u64 w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
      if (NWAVES > 1) {
        if ((threadIdx.x & 63) == 0) s[i][threadIdx.x >> 6] = v;
        __syncthreads();                                            // (round i has its own row of s: one barrier per round)
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { const u64 o = s[i][w]; v = o > v ? o : v; }
      }
      level = level && a[i] == v;
      if (!bitlen && v) bitlen = 64 * i + 64 - __clzll((long long)v);
      if (threadIdx.x == 0) out[i] = v;
    }
  return bitlen;
}
// z: [gridDim.y][n][nw] as decrypt_round_kernel takes it; msg: [gridDim.y][n] the same message bits, or null; part: [gridDim.y][gridDim.x][nw]
// the maximum of |r| over the coefficients of each block
template <int MAXNL>
__global__ void __launch_bounds__(256) decrypt_noise_kernel(const u64* __restrict__ z, i64 n, int nw, int logQ, u64 p, i64* __restrict__ msg,
                                                            u64* __restrict__ part) {
  const i64 c = blockIdx.y;
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
  u64 a[MAXNL];
  ctw_zero(a);
  if (j < n) {
    u64 P[MAXNL];
    u64 carry;
    round_product(z, c * n + j, nw, logQ, p, P, carry);
    if (msg) msg[c * n + j] = (i64)(round_quotient(P, carry, nw, logQ) % p);
    round_residual(P, nw, logQ, a);
  }
  block_limb_max<MAXNL, 4>(a, nw, part + (c * gridDim.x + blockIdx.x) * nw);
}
// part: [count][np][nw] -> maxres [count][nw], budget [count] = max(0, logQ - bitlen(maxres)); one wave per ciphertext, each lane keeping
// the lexicographic maximum of the partials it strides over.  A launch boundary separates it from the kernel above: no atomics, no hand-off.
template <int MAXNL>
__global__ void __launch_bounds__(64) noise_budget_kernel(const u64* __restrict__ part, int np, int nw, int logQ, u64* __restrict__ maxres,
                                                          int* __restrict__ budget) {
  const i64 c = blockIdx.x;
  u64 a[MAXNL];
  ctw_zero(a);
  for (int g = threadIdx.x; g < np; g += 64) {
    const u64* x = part + (c * np + g) * nw;
    u64 v[MAXNL];
    bool decided = false, greater = false;
#pragma unroll
    for (int i = MAXNL - 1; i >= 0; --i) {
      v[i] = 0;
      if (i < nw) {
        v[i] = x[i];
        if (!decided && v[i] != a[i]) { decided = true; greater = v[i] > a[i]; }
      }
    }
#pragma unroll
    for (int i = 0; i < MAXNL; ++i) a[i] = greater ? v[i] : a[i];
  }
  const int bitlen = block_limb_max<MAXNL, 1>(a, nw, maxres + c * nw);
  if (threadIdx.x == 0) budget[c] = logQ > bitlen ? logQ - bitlen : 0;
}
int launch_decrypt_noise(fhesi_ctx* ctx, const u64* d_z, i64 count, int nw, int logQ, u64 p, i64* d_msg, u64* d_part, u64* d_maxres, int* d_budget) {
  if (!count) return 0;
  if (nw > 32) FHESI_FAIL("Decrypt: logQ=%d exceeds the supported 2047 bits", logQ);
  FHESI_TRY(grid_y_ok("Decrypt", "ciphertexts per launch", count));
  const i64 n = ctx->phim, np = noise_blocks(ctx);
  with_limb_class<2, 9, 17, 32>(nw, [&](auto C) {
    constexpr int N = decltype(C)::value;
    decrypt_noise_kernel<N><<<dim3((unsigned)np, (unsigned)count), 256, 0, ctx->stream>>>(d_z, n, nw, logQ, p, d_msg, d_part);
    noise_budget_kernel<N><<<(unsigned)count, 64, 0, ctx->stream>>>(d_part, (int)np, nw, logQ, d_maxres, d_budget);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- KeySwitchSI::Init in batches (FHE-SI.cpp:153-209) -------------------------------------------------------------------------------
// b = A * t for every column: dst[col][l][j] = a[col][l][j] * t[l][j] mod q_l   (`b[ind] = A[ind]; b[ind] *= t`, :180-184)
__global__ void __launch_bounds__(256) rows_mul_bcast_kernel(u64* __restrict__ dst, const u64* __restrict__ a, const u64* __restrict__ t, int L, i64 n,
                                                              const PrimeConst* __restrict__ pcs) {
  const i64 col = blockIdx.z;
  const int l = blockIdx.y;
  const PrimeConst pc = pcs[l];
  const u64* ar = a + (col * L + l) * n;
  const u64* tr = t + (i64)l * n;
  u64* dr = dst + (col * L + l) * n;
  for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) dr[j] = d_mulmod(ar[j], tr[j], pc);
}
int launch_rows_mul_bcast(fhesi_ctx* ctx, u64* d_dst, const u64* d_a, const u64* d_t, i64 ncols) {
  if (!ncols) return 0;
  FHESI_TRY(grid_y_ok("KeySwitchSI::Init", "columns", ncols));
  unsigned gx = (unsigned)((ctx->phim + 255) / 256);
  if (gx > 64) gx = 64;
  rows_mul_bcast_kernel<<<dim3(gx, (unsigned)ctx->L, (unsigned)ncols), 256, 0, ctx->stream>>>(d_dst, d_a, d_t, ctx->L, ctx->phim, ctx->d_pc);
  HIP_TRY(hipGetLastError());
  return 0;
}
// bCoeff += err; bCoeff += sCoeff[i] (already shifted left by digit_bits * j); ReduceCoefficients(bCoeff, logQ)   (:192-203)
//   bcoef: [ncol][n][wb] two's complement (toPoly of b), scoef: [nsrc][n][ws] (toPoly of the source key components), err: [ncol][n];
//   out: [ncol][n][nl] centred modulo 2^logQ.  Only the bits below logQ of every term matter, so all arithmetic is modulo 2^(64 nl).
template <int MAXNL>
__global__ void __launch_bounds__(256) keygen_combine_kernel(const u64* __restrict__ bcoef, int wb, const u64* __restrict__ scoef, int ws,
                                                             const i64* __restrict__ err, i64 n, int nd, int digit_bits, int nl, int logQ,
                                                             u64* __restrict__ out) {
  const i64 col = blockIdx.y;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const i64 comp = col / nd;
  const int sh = (int)(col % nd) * digit_bits, wsh = sh >> 6, bsh = sh & 63;
  const u64* bx = bcoef + (col * n + j) * wb;
  const u64* sx = scoef + (comp * n + j) * ws;
  const i64 e = err[col * n + j];
  const u64 bsign = (bx[wb - 1] >> 63) ? ~0ull : 0, ssign = (sx[ws - 1] >> 63) ? ~0ull : 0, esign = e < 0 ? ~0ull : 0;
  // limb k of the sign-extended s; limb i of (s << sh) is made of its limbs i - wsh and i - wsh - 1
  auto slimb = [=](int k) -> u64 { return k < 0 ? 0 : (k < ws ? sx[k] : ssign); };
  u64 v[MAXNL];
  ctw_sum(v, nl, 0, [=](int i) { return i < wb ? bx[i] : bsign; }, [=](int i) { return i == 0 ? (u64)e : esign; }, [=](int i) {
    const u64 hi = slimb(i - wsh), lo = slimb(i - wsh - 1);
    return bsh ? ((hi << bsh) | (lo >> (64 - bsh))) : hi;
  });
  ctw_store_centred(v, nl, logQ, out + (col * n + j) * nl);
}
int launch_keygen_combine(fhesi_ctx* ctx, const u64* d_bcoef, int wb, const u64* d_scoef, int ws, const i64* d_err, i64 ncols, int nd, int digit_bits, int nl,
                          int logQ, u64* d_out) {
  if (!ncols) return 0;
  FHESI_TRY(limbs_ok("KeySwitchSI::Init: coefficients", nl));
  const dim3 grid((unsigned)((ctx->phim + 255) / 256), (unsigned)ncols);
  with_limb_class<2, 8, 16, 32>(nl, [&](auto C) {
    keygen_combine_kernel<decltype(C)::value><<<grid, 256, 0, ctx->stream>>>(d_bcoef, wb, d_scoef, ws, d_err, ctx->phim, nd, digit_bits, nl, logQ, d_out);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
