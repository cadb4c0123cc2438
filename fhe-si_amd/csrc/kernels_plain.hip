// kernels_plain.hip -- sums of ciphertext x prepared-plaintext products in the evaluation domain (fhesi_ct_plain_sum_dev, capi_ct.hip)
//   plain_sum    sum_t parts[i] *= w_t (CiphertextPart::operator*=(ZZX), Ciphertext.cpp:29-36) under Ciphertext::operator+= (:123-134), before toPoly
#include "fhesi_internal.h"

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// out[g][i] = sum_{t in [seg[g], seg[g+1])} ca[slot_a[t]][i] * w[slot_w[t]]   (i = 0, 1: the two ciphertext parts), per prime and evaluation point.
// ca: [nu][2][L][n] evaluation form of the distinct ciphertexts of the pass, w: [nw][L][n] the prepared plaintexts (fhesi_plain), out: [ng][2][L][n].
// Grid (tiles of j, prime, group); the index lists are read uniformly per block, a lane owns two adjacent evaluation points (16 B per access,
// coalesced along j).  Every plaintext word is loaded once and feeds both parts: 3 T rows read and 2 written per (group, prime).
// Exact 128-bit accumulation.  The launcher admits residues of at most 61 bits (bar_k <= 61): a product is at most (2^61 - 1)^2 = 2^122 - 2^62 + 1
// and an accumulator starts from a folded value (or, accumulating, a stored residue) below 2^61, so after F = 64 terms it holds at most
// 64 (2^61 - 1)^2 + 2^61 - 1 = 2^128 - 2^68 + 2^61 + 63 < 2^128; a 65th term could wrap.  Folded every F = kPlainSumFold = 64 terms.
__global__ void __launch_bounds__(256) plain_sum_kernel(const u64* __restrict__ ca, const u64* __restrict__ w, const int* __restrict__ slot_a, const int* __restrict__ slot_w,
                                                        const int* __restrict__ seg, int accumulate, u64* __restrict__ out, i64 n, int L, const PrimeConst* __restrict__ pcs) {
  const int g = blockIdx.z, l = blockIdx.y;
  const PrimeConst pc = pcs[l];
  const i64 rs = (i64)L * n, n2 = n >> 1;
  u64x2* o0 = (u64x2*)(out + (((i64)g * 2) * L + l) * n);
  u64x2* o1 = (u64x2*)(out + (((i64)g * 2 + 1) * L + l) * n);
  const int t0 = seg[g], t1 = seg[g + 1];
  for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += (i64)gridDim.x * blockDim.x) {
    Acc128 r0x{0, 0}, r0y{0, 0}, r1x{0, 0}, r1y{0, 0};
    if (accumulate) { const u64x2 p0 = o0[j], p1 = o1[j]; r0x.lo = p0.x; r0y.lo = p0.y; r1x.lo = p1.x; r1y.lo = p1.y; }
    for (int t = t0; t < t1;) {
      const int te = t1 - t < kPlainSumFold ? t1 : t + kPlainSumFold;
      for (; t < te; ++t) {
        const u64* a = ca + (((i64)slot_a[t] * 2) * L + l) * n;
        const u64x2 a0 = ((const u64x2*)a)[j], a1 = ((const u64x2*)(a + rs))[j];
        const u64x2 b = ((const u64x2*)(w + ((i64)slot_w[t] * L + l) * n))[j];
        acc_mad(r0x, a0.x, b.x);
        acc_mad(r0y, a0.y, b.y);
        acc_mad(r1x, a1.x, b.x);
        acc_mad(r1y, a1.y, b.y);
      }
      if (t < t1) { r0x = Acc128{acc_reduce(r0x, pc), 0}; r0y = Acc128{acc_reduce(r0y, pc), 0}; r1x = Acc128{acc_reduce(r1x, pc), 0}; r1y = Acc128{acc_reduce(r1y, pc), 0}; }
    }
    u64x2 s0, s1;
    s0.x = acc_reduce(r0x, pc); s0.y = acc_reduce(r0y, pc);
    s1.x = acc_reduce(r1x, pc); s1.y = acc_reduce(r1y, pc);
    o0[j] = s0;
    o1[j] = s1;
  }
}
int launch_plain_sum(fhesi_ctx* ctx, const u64* d_ca, const u64* d_w, const int* d_slot_a, const int* d_slot_w, const int* d_seg, i64 ngroups, bool accumulate, u64* d_out,
                     double nterms) {
  if (!ngroups) return 0;
  if (ctx->phim & 1) FHESI_FAIL("plain_sum: odd phi(m) not supported (two evaluation points per lane)");
  for (int l = 0; l < ctx->L; ++l) if (ctx->pc[l].bar_k > 61) FHESI_FAIL("plain_sum: %u-bit residues overflow the 128-bit accumulator", ctx->pc[l].bar_k);
  ProfScope prof(ctx, PROF_PLAIN_SUM, nterms);
  PROF_KERNEL(ctx, PROF_PLAIN_SUM, plain_sum_kernel);
  const i64 b = (ctx->phim / 2 + 255) / 256;
  const unsigned gx = (unsigned)(b < 1 ? 1 : (b > 64 ? 64 : b));
  grid_chunks(ngroups, [&](i64 done, i64 cnt) {
    plain_sum_kernel<<<dim3(gx, (unsigned)ctx->L, (unsigned)cnt), 256, 0, ctx->stream>>>(d_ca, d_w, d_slot_a, d_slot_w, d_seg + done, accumulate ? 1 : 0,
                                                                                        d_out + done * 2 * ctx->L * ctx->phim, ctx->phim, ctx->L, ctx->d_pc);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
