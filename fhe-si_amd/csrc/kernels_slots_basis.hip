// kernels_slots_basis.hip -- integer slots over a basis of plaintext primes on a two-row ring.
//
// A slot basis is k distinct primes p_c = 1 mod m on ONE ring m = 2^3 .. 2^16 (hm::slot_basis), P = prod p_c.  A slot holds an integer modulo P,
// given and returned as a signed value in (-P/2, P/2) of L two's complement 64-bit limbs; channel c is the ordinary two-row space of
// (m, p_c, g) (kernels_slots_pow2.hip: same rho0 rule, same slot order), so every operation of the scheme applies channel by channel with that
// channel's p, on one context and one key set.  This file is the layer that makes k channels one value:
//   embed     vals [count][nvals][L_in] -> msg [k][count][n]     the loader reduces the slot's limbs modulo p_c, then the inverse transform
//   decode    msg [k][count][n] -> res [k][count][nvals]         the forward transform, 32-bit residues
//   garner    res -> vals [count][nvals][L]                      mixed-radix digits, P-adic Horner, centred lift
// embed and decode run one workgroup per (plaintext, channel), grid (count, k), over the transform of slots_pow2_core.inc with the channel's
// record taken from an array indexed by blockIdx.y; garner runs one thread per (plaintext, slot).
#include "../../include/fhesi_hip.h"
#include "fhesi_internal.h"

#include <algorithm>

#include "slots_pow2_core.inc"

using hm::SlotBasis;

struct BasisChan {
  Pow2Dev D;
  SpTw one, r32;                        // 1 and 2^32 mod p with their quotients floor(w 2^32 / p): the Horner step of the loader
  u32 top[SlotBasis::MAXL + 1];         // 2^(64 l) mod p: what a negative value of l limbs read as unsigned is too large by
};

// The slot's L two's complement limbs -> [0, p).  Horner over the 32-bit halves from the top: acc <- acc 2^32 + half, every term brought
// into [0, 2p) by a Shoup product; a negative value was read 2^(64 L) too large.
__device__ __forceinline__ u32 sb_red(const u64* __restrict__ limbs, int L, const BasisChan& C, u32 p) {
  const u32 twop = 2 * p;
  const SpTw one = C.one, r32 = C.r32;
  u32 acc = 0;
  u64 w = 0;
  for (int l = L - 1; l >= 0; --l) {
    w = limbs[l];
    acc = sp2_add(sp2_mul(acc, r32, p), sp2_mul((u32)(w >> 32), one, p), twop);
    acc = sp2_add(sp2_mul(acc, r32, p), sp2_mul((u32)w, one, p), twop);
  }
  if (limbs[L - 1] >> 63) acc = sp2_sub(acc, C.top[L], twop);
  return acc >= p ? acc - p : acc;
}

// One workgroup per (plaintext, channel); dynamic LDS: n + n / 32 words.
// embed: vals [count][nvals][L] -> msg [k][count][n] in [0, p_c); slots nvals .. n-1 are zero.
__global__ void __launch_bounds__(SP2_T) slots_basis_embed(const u64* __restrict__ vals, i64* __restrict__ msg, i64 nvals, int L, i64 count, const BasisChan* __restrict__ chans) {
  extern __shared__ __attribute__((aligned(16))) u32 sb_lds[];
  const BasisChan& C = chans[blockIdx.y];
  const Pow2Dev D = C.D;
  const i64 row = blockIdx.x;
  const u64* in = vals + row * nvals * L;
  if (nvals < (i64)D.n) {               // (uniform) the spectrum positions of the slots not given
    for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) sb_lds[sp2_pad(i)] = 0;
    __syncthreads();
  }
  for (i64 j = threadIdx.x; j < nvals; j += blockDim.x) sb_lds[sp2_pad(D.pos[j])] = sb_red(in + j * L, L, C, D.p);
  __syncthreads();
  sp2_transform<false>(sb_lds, D);
  i64* out = msg + ((i64)blockIdx.y * count + row) * D.n;
  for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) { const u32 x = sb_lds[sp2_pad(i)]; out[i] = (i64)(x >= D.p ? x - D.p : x); }
}
// decode: msg [k][count][n] (any int64) -> res [k][count][nvals], residues in [0, p_c)
__global__ void __launch_bounds__(SP2_T) slots_basis_decode(const i64* __restrict__ msg, u32* __restrict__ res, i64 nvals, i64 count, const BasisChan* __restrict__ chans) {
  extern __shared__ __attribute__((aligned(16))) u32 sb_lds[];
  const Pow2Dev D = chans[blockIdx.y].D;
  const i64 at = (i64)blockIdx.y * count + blockIdx.x;
  const i64* in = msg + at * D.n;
  for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) sb_lds[sp2_pad(i)] = sp2_red(in[i], D.p64, D.one_sh);
  __syncthreads();
  sp2_transform<true>(sb_lds, D);
  u32* out = res + at * nvals;
  for (i64 j = threadIdx.x; j < nvals; j += blockDim.x) { const u32 x = sb_lds[sp2_pad(D.pos[j])]; out[j] = x >= D.p ? x - D.p : x; }
}

// Recombination, one thread per (plaintext, slot): res [k][total] -> vals [total][L].
//   digits   x_c = (..((r_c - x_0) p_0^-1 - x_1) p_1^-1 .. - x_(c-1)) p_(c-1)^-1 mod p_c          (value = x_0 + p_0 (x_1 + p_1 (x_2 + ..)))
//   value    Horner from the top digit over W = 2 L words of 32 bits, a 64-bit multiply-add with carry per word
//   lift     value > floor(P / 2): one subtraction of P, two's complement
// The digits and the words live in LDS, [index][thread]: their indices are run-time values (k, L), and consecutive threads hit consecutive banks.
static constexpr int SB_GT = 128;
__global__ void __launch_bounds__(SB_GT) slots_basis_garner(const u32* __restrict__ res, u64* __restrict__ vals, i64 total, int k, int L, const u32* __restrict__ primes,
                                                            const Shoup2* __restrict__ inv /* [k][k] */, const u32* __restrict__ Pw /* [2][2 L]: P, floor(P / 2) */) {
  __shared__ u32 x[SlotBasis::MAXK][SB_GT];
  __shared__ u32 a[2 * SlotBasis::MAXL][SB_GT];
  const int tid = threadIdx.x;
  const i64 t = (i64)blockIdx.x * SB_GT + tid;
  if (t >= total) return;               // (no barrier below: a thread touches its own column only)
  for (int c = 0; c < k; ++c) {
    const u64 p = primes[c];
    u64 v = res[(i64)c * total + t];
    for (int j = 0; j < c; ++j) {
      const Shoup2 w = inv[c * k + j];
      v = d_shoup(v + (p << 32) - x[j][tid], w.w, w.wp, p);             // p 2^32 = 0 mod p keeps the difference non-negative
    }
    x[c][tid] = (u32)v;
  }
  const int W = 2 * L;
  for (int w = 0; w < W; ++w) a[w][tid] = 0;
  for (int c = k - 1; c >= 0; --c) {
    const u64 p = primes[c];
    u64 carry = x[c][tid];
    for (int w = 0; w < W; ++w) {
      const u64 s = (u64)a[w][tid] * p + carry;
      a[w][tid] = (u32)s;
      carry = s >> 32;
    }
  }
  bool above = false;
  for (int w = W - 1; w >= 0; --w) {
    const u32 aw = a[w][tid], hw = Pw[W + w];
    if (aw != hw) { above = aw > hw; break; }
  }
  u64 borrow = 0;
  u64* out = vals + t * L;
  for (int l = 0; l < L; ++l) {
    u32 lo = a[2 * l][tid], hi = a[2 * l + 1][tid];
    if (above) {
      const u64 d0 = (u64)lo - Pw[2 * l] - borrow;
      const u64 d1 = (u64)hi - Pw[2 * l + 1] - (d0 >> 63);
      lo = (u32)d0; hi = (u32)d1; borrow = d1 >> 63;
    }
    out[l] = (u64)lo | (u64)hi << 32;
  }
}

// ------------------------------------------------------------------------------------------------ setup and launch
static void basis_release(fhesi_slots_basis* b) {
  for (fhesi_slots* s : b->ch)
    if (s) slots_unmake(s);
  hipFree(b->d_chan); hipFree(b->d_garner); hipFree(b->d_words);
  delete b;
}
static int basis_build(fhesi_slots_basis* b) {
  const SlotBasis& B = b->B;
  fhesi_ctx* c = b->ctx;
  const int k = B.k;
  std::vector<BasisChan> chans(k);
  for (int i = 0; i < k; ++i) {
    FHESI_TRY(slots_make(c, B.ch[i], &b->ch[i]));          // (direct path: hm::slot_basis admits no other)
    const u64 p = B.primes[i];
    BasisChan& C = chans[i];
    C.D = sp2_dev(b->ch[i]);
    C.one = {1u, (u32)((1ull << 32) / p)};
    const u64 r = (1ull << 32) % p;
    C.r32 = {(u32)r, (u32)((r << 32) / p)};
    u64 t = 1;
    for (int l = 0; l <= SlotBasis::MAXL; ++l) { C.top[l] = (u32)t; t = hm::mulmod(t, hm::mulmod(r, r, p), p); }
  }
  std::vector<Shoup2> inv((size_t)k * k, Shoup2{0, 0});
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < i; ++j) { const u64 w = B.garner[(size_t)i * k + j]; inv[(size_t)i * k + j] = {w, hm::shoup(w, B.primes[i])}; }
  const int W = 2 * B.limbs;
  std::vector<u32> words((size_t)2 * W + k);             // P, floor(P / 2) as 32-bit words, then the primes
  for (int w = 0; w < W; ++w) {
    words[w] = (u32)(B.P[w / 2] >> (32 * (w & 1)));
    words[W + w] = (u32)(B.halfP[w / 2] >> (32 * (w & 1)));
  }
  for (int i = 0; i < k; ++i) words[2 * W + i] = (u32)B.primes[i];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMalloc(&b->d_chan, chans.size() * sizeof(BasisChan)));
  HIP_TRY(hipMemcpy(b->d_chan, chans.data(), chans.size() * sizeof(BasisChan), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&b->d_garner, inv.size() * sizeof(Shoup2)));
  HIP_TRY(hipMemcpy(b->d_garner, inv.data(), inv.size() * sizeof(Shoup2), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&b->d_words, words.size() * sizeof(u32)));
  HIP_TRY(hipMemcpy(b->d_words, words.data(), words.size() * sizeof(u32), hipMemcpyHostToDevice));
  const int shmem = (int)sp2_shmem((u32)(B.m / 2));
  if (shmem > 64 * 1024) {
    HIP_TRY(hipFuncSetAttribute((const void*)slots_basis_decode, hipFuncAttributeMaxDynamicSharedMemorySize, shmem));
    HIP_TRY(hipFuncSetAttribute((const void*)slots_basis_embed, hipFuncAttributeMaxDynamicSharedMemorySize, shmem));
  }
  return 0;
}
static int basis_shape(const fhesi_slots_basis* b, const char* what, i64 nvals, i64 count) {
  if (!b) FHESI_FAIL("null slot basis");
  FHESI_TRY(slots_check_shape(what, nvals, count, b->B.m / 2));
  if (count > (1ll << 30)) FHESI_FAIL("%s: more than 2^30 plaintexts in one call", what);
  return 0;
}
int slots_basis_embed_rows(fhesi_slots_basis* b, const i64* d_vals, int L_in, i64 nvals, i64 count, i64* d_msg) {
  FHESI_TRY(basis_shape(b, "EmbedInSlots", nvals, count));
  if (L_in < 1 || L_in > SlotBasis::MAXL) FHESI_FAIL("EmbedInSlots: %d limbs per value, 1 .. %d are taken", L_in, SlotBasis::MAXL);
  if (!count) return 0;
  HIP_TRY(hipSetDevice(b->ctx->device));
  const u32 n = (u32)(b->B.m / 2);
  slots_basis_embed<<<dim3((unsigned)count, (unsigned)b->B.k), sp2_threads(n), sp2_shmem(n), b->ctx->stream>>>((const u64*)d_vals, d_msg, nvals, L_in, count, (const BasisChan*)b->d_chan);
  if (hipGetLastError() != hipSuccess) FHESI_FAIL("slot basis: kernel launch failed");
  return 0;
}
int slots_basis_decode_rows(fhesi_slots_basis* b, const i64* d_msg, i64 count, i64 nvals, i64* d_vals) {
  FHESI_TRY(basis_shape(b, "DecodeSlots", nvals, count));
  if (!count) return 0;
  fhesi_ctx* c = b->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const SlotBasis& B = b->B;
  const i64 total = count * nvals;
  const u32 n = (u32)(B.m / 2);
  const int W = 2 * B.limbs;
  void* d_res;
  FHESI_TRY(ws_reserve(c, 8, (size_t)B.k * total * sizeof(u32), &d_res));
  slots_basis_decode<<<dim3((unsigned)count, (unsigned)B.k), sp2_threads(n), sp2_shmem(n), c->stream>>>(d_msg, (u32*)d_res, nvals, count, (const BasisChan*)b->d_chan);
  slots_basis_garner<<<(unsigned)((total + SB_GT - 1) / SB_GT), SB_GT, 0, c->stream>>>((const u32*)d_res, (u64*)d_vals, total, B.k, B.limbs, b->d_words + 2 * W, b->d_garner, b->d_words);
  if (hipGetLastError() != hipSuccess) FHESI_FAIL("slot basis: kernel launch failed");
  return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/fhesi_hip.h)
extern "C" int fhesi_slots_basis_plan(int64_t m, int32_t bits, int32_t prime_bits, int64_t generator, int32_t* k, uint64_t* primes_out, int32_t* limbs) {
  std::vector<u64> primes;
  int L = 0;
  if (const char* why = hm::slot_basis_plan(m, bits, prime_bits, generator, &primes, &L))
    FHESI_FAIL("SlotBasis plan (m=%lld, bits=%d, prime_bits=%d, g=%lld) refused: %s", (long long)m, bits, prime_bits, (long long)generator, why);
  if (k) *k = (int32_t)primes.size();
  if (primes_out) std::copy(primes.begin(), primes.end(), primes_out);
  if (limbs) *limbs = L;
  return 0;
}
extern "C" int fhesi_slots_basis_check(int64_t m, const uint64_t* primes, int32_t k, int64_t generator, int32_t* limbs, uint64_t* modulus_out) {
  SlotBasis B;
  if (const char* why = hm::slot_basis(m, (const u64*)primes, k, generator, &B)) FHESI_FAIL("SlotBasis(m=%lld, k=%d, g=%lld) refused: %s", (long long)m, k, (long long)generator, why);
  if (limbs) *limbs = B.limbs;
  if (modulus_out) std::copy(B.P.begin(), B.P.end(), modulus_out);
  return 0;
}
extern "C" int fhesi_slots_basis_create(fhesi_ctx* c, const uint64_t* primes, int32_t k, int64_t generator, fhesi_slots_basis** out) {
  if (!out) FHESI_FAIL("null output pointer");
  *out = nullptr;
  if (!c) FHESI_FAIL("null context");
  SlotBasis B;                                             // the argument checks come first: a refused basis launches nothing
  if (const char* why = hm::slot_basis(c->m, (const u64*)primes, k, generator, &B)) FHESI_FAIL("SlotBasis(m=%lld, k=%d, g=%lld) refused: %s", (long long)c->m, k, (long long)generator, why);
  if (B.m / 2 != c->phim) FHESI_FAIL("SlotBasis: phi(m) mismatch");
  HIP_TRY(hipSetDevice(c->device));
  fhesi_slots_basis* b = new fhesi_slots_basis();
  b->ctx = c;
  b->B = B;
  b->ch.assign(B.k, nullptr);
  if (const int rc = basis_build(b)) { basis_release(b); return rc; }
  c->live_handles++;
  *out = b;
  return 0;
}
extern "C" int fhesi_slots_basis_free(fhesi_slots_basis* b) {
  if (!b) return 0;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->ctx->live_handles--;
  basis_release(b);
  return 0;
}
extern "C" int fhesi_slots_basis_info(const fhesi_slots_basis* b, int32_t* k, uint64_t* primes, int32_t* limbs, int64_t* total, int64_t* rows, int64_t* cols) {
  if (!b) FHESI_FAIL("null slot basis");
  if (k) *k = b->B.k;
  if (primes) std::copy(b->B.primes.begin(), b->B.primes.end(), primes);
  if (limbs) *limbs = b->B.limbs;
  if (total) *total = b->B.m / 2;
  if (rows) *rows = 2;
  if (cols) *cols = b->B.m / 4;
  return 0;
}
extern "C" int fhesi_slots_basis_channel(fhesi_slots_basis* b, int32_t c, fhesi_slots** slots) {
  if (!b || !slots) FHESI_FAIL("null argument");
  if (c < 0 || c >= b->B.k) FHESI_FAIL("SlotBasis: channel %d of %d", c, b->B.k);
  *slots = b->ch[c];
  return 0;
}
extern "C" int fhesi_slots_basis_embed_dev(fhesi_slots_basis* b, const int64_t* vals_dev, int32_t L_in, int64_t nvals, int64_t count, int64_t* msg_dev) {
  return slots_basis_embed_rows(b, vals_dev, L_in, nvals, count, msg_dev);
}
extern "C" int fhesi_slots_basis_decode_dev(fhesi_slots_basis* b, const int64_t* msg_dev, int64_t count, int64_t nvals, int64_t* vals_dev) {
  return slots_basis_decode_rows(b, msg_dev, count, nvals, vals_dev);
}
extern "C" int fhesi_slots_basis_embed(fhesi_slots_basis* b, const int64_t* vals_host, int32_t L_in, int64_t nvals, int64_t count, int64_t* msg_host) {
  FHESI_TRY(basis_shape(b, "EmbedInSlots", nvals, count));
  if (L_in < 1 || L_in > SlotBasis::MAXL) FHESI_FAIL("EmbedInSlots: %d limbs per value, 1 .. %d are taken", L_in, SlotBasis::MAXL);
  return slots_stage_host(b->ctx, true, vals_host, msg_host, (size_t)count * nvals * L_in * 8, (size_t)b->B.k * count * (b->B.m / 2) * 8,
                          [&](i64* d_vals, i64* d_msg) { return slots_basis_embed_rows(b, d_vals, L_in, nvals, count, d_msg); });
}
extern "C" int fhesi_slots_basis_decode(fhesi_slots_basis* b, const int64_t* msg_host, int64_t count, int64_t nvals, int64_t* vals_host) {
  FHESI_TRY(basis_shape(b, "DecodeSlots", nvals, count));
  return slots_stage_host(b->ctx, false, msg_host, vals_host, (size_t)count * nvals * b->B.limbs * 8, (size_t)b->B.k * count * (b->B.m / 2) * 8,
                          [&](i64* d_vals, i64* d_msg) { return slots_basis_decode_rows(b, d_msg, count, nvals, d_vals); });
}
