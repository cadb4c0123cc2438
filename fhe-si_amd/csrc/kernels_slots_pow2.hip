// kernels_slots_pow2.hip -- plaintext slots on the power-of-two rings: m = 2^k (k >= 3), n = m/2, p prime, p = 1 mod m.
//
// Phi_m = X^n + 1 splits into n linear factors modulo p, but (Z/m)^* = <-1> x <g> (g = 3 or 5 mod 8) is not cyclic: the slots form 2 rows
// of h = n/2 columns, slot r h + j on the root rho0^(e), e = (-1)^r g^j mod m (hm::slot_space_pow2).  X -> X^(g^t) rotates both rows left
// by t, X -> X^(m-1) swaps them.  What the reference's single-generator walk cannot express; every BFV-style library calls it batching.
//
// No chirp is needed here: p = 1 mod 2n has a primitive 2n-th root (rho0 itself), so
//   DecodeSlots(a)[s] = a(rho0^(e_s))   is ONE negacyclic transform of length n modulo p with psi = rho0, gathered through a table, and
//   EmbedInSlots(v)                      is the scatter through the same table and the inverse transform; the transform is already modulo
//                                        X^n + 1, so nothing is folded.
// Direct path (n <= 2^15, p < 2^31): one workgroup per plaintext, the whole row of n 32-bit words in LDS (one pad word per 32: 132 KiB of
// the 160 KiB at n = 2^15, two workgroups per CU from n = 2^14 down).  Harvey butterflies on lazy values in [0, 2p) (2p < 2^32) with Shoup
// constants floor(w 2^32 / p); three stages per pass over LDS in registers (a pass of one or two stages first when log2 n is not a multiple of
// three), one barrier per pass.  The forward transform takes natural order to bit-reversed order: the evaluation at rho0^(2u + 1) lands on
// position brv(u), so slot s reads position brv((e_s - 1) / 2) (d_p2pos); the inverse runs the passes backwards with the inverse twiddles
// and n^-1 folded into its last stage.  The primes of ntt32_core.inc are compile-time chain primes below 2^30 with lazy values up to 4p;
// p here is a run-time value up to 2^31, hence butterflies of its own.
// Everything else (n > 2^15 or p >= 2^31) runs the chirp machinery of kernels_slots.hip on the two-row exponent table: the length-m DFT at
// rho0 with the fold out[i] = f[i] - f[i + n] (its case q = 2, s = n), one or two auxiliary primes by the same m p^2 < 2^59 rule.
#include "../../include/fhesi_hip.h"
#include "fhesi_internal.h"

#include <algorithm>

using hm::SlotSpace;
#include "slots_pow2_core.inc"

// One workgroup per plaintext; dynamic LDS: n + n / 32 words.
// decode: msg [count][n] -> vals [count][nvals]; slots take .. nvals-1 are written as zero.
__global__ void __launch_bounds__(SP2_T) slots_pow2_decode(const i64* __restrict__ msg, i64* __restrict__ vals, i64 nvals, i64 take, Pow2Dev D) {
  extern __shared__ __attribute__((aligned(16))) u32 sp2_lds[];
  const i64 row = blockIdx.x;
  const i64* in = msg + row * D.n;
  for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) sp2_lds[sp2_pad(i)] = sp2_red(in[i], D.p64, D.one_sh);
  __syncthreads();
  sp2_transform<true>(sp2_lds, D);
  i64* out = vals + row * nvals;
  for (i64 j = threadIdx.x; j < nvals; j += blockDim.x) {
    i64 v = 0;
    if (j < take) { const u32 x = sp2_lds[sp2_pad(D.pos[j])]; v = x >= D.p ? x - D.p : x; }
    out[j] = v;
  }
}
// embed: vals [count][nvals] -> msg [count][n]; slots take .. n-1 are zero.
__global__ void __launch_bounds__(SP2_T) slots_pow2_embed(const i64* __restrict__ vals, i64* __restrict__ msg, i64 nvals, i64 take, Pow2Dev D) {
  extern __shared__ __attribute__((aligned(16))) u32 sp2_lds[];
  const i64 row = blockIdx.x;
  const i64* in = vals + row * nvals;
  if (take < (i64)D.n) {                // (uniform) the spectrum positions of the slots not given
    for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) sp2_lds[sp2_pad(i)] = 0;
    __syncthreads();
  }
  for (i64 j = threadIdx.x; j < take; j += blockDim.x) sp2_lds[sp2_pad(D.pos[j])] = sp2_red(in[j], D.p64, D.one_sh);
  __syncthreads();
  sp2_transform<false>(sp2_lds, D);
  i64* out = msg + row * D.n;
  for (u32 i = threadIdx.x; i < D.n; i += blockDim.x) { const u32 x = sp2_lds[sp2_pad(i)]; out[i] = (i64)(x >= D.p ? x - D.p : x); }
}

// ------------------------------------------------------------------------------------------------ setup and launch
static u32 sp2_brv(u32 x, int bits) {
  u32 r = 0;
  for (int b = 0; b < bits; ++b) r |= ((x >> b) & 1u) << (bits - 1 - b);
  return r;
}
static SpTw sp2_tw(u64 w, u64 p) { return {(u32)w, (u32)(((u128)w << 32) / p)}; }
int slots_pow2_build(fhesi_slots* s) {
  if (s->d_p2tw) return 0;
  const SlotSpace& S = s->S;
  const u64 p = S.p;
  const u32 n = (u32)S.phim;
  int logn = 0;
  while ((1u << logn) < n) ++logn;
  std::vector<u64> pw(n), pwi(n);       // psi^i, psi^-i
  const u64 psi_inv = hm::invmod(S.rho0, p);
  pw[0] = pwi[0] = 1;
  for (u32 i = 1; i < n; ++i) { pw[i] = hm::mulmod(pw[i - 1], S.rho0, p); pwi[i] = hm::mulmod(pwi[i - 1], psi_inv, p); }
  std::vector<SpTw> tw((size_t)2 * n);
  for (u32 i = 0; i < n; ++i) { const u32 b = sp2_brv(i, logn); tw[i] = sp2_tw(pw[b], p); tw[n + i] = sp2_tw(pwi[b], p); }
  std::vector<u32> pos(n);
  for (u32 j = 0; j < n; ++j) pos[j] = sp2_brv(((u32)S.exps[j] - 1) / 2, logn);
  const u64 ninv = hm::invmod((u64)n % p, p);
  s->p2ninv = sp2_tw(ninv, p);
  s->p2ninv_w1 = sp2_tw(hm::mulmod(ninv, pwi[sp2_brv(1, logn)], p), p);
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipMalloc(&s->d_p2pos, pos.size() * sizeof(u32)));
  HIP_TRY(hipMemcpy(s->d_p2pos, pos.data(), pos.size() * sizeof(u32), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&s->d_p2tw, tw.size() * sizeof(SpTw)));
  HIP_TRY(hipMemcpy(s->d_p2tw, tw.data(), tw.size() * sizeof(SpTw), hipMemcpyHostToDevice));
  const int shmem = (int)sp2_shmem(n);
  if (shmem > 64 * 1024) {
    HIP_TRY(hipFuncSetAttribute((const void*)slots_pow2_decode, hipFuncAttributeMaxDynamicSharedMemorySize, shmem));
    HIP_TRY(hipFuncSetAttribute((const void*)slots_pow2_embed, hipFuncAttributeMaxDynamicSharedMemorySize, shmem));
  }
  return 0;
}
int slots_pow2_run(fhesi_slots* s, bool embed, const i64* d_in, i64* d_out, i64 nvals, i64 take, i64 count) {
  const SlotSpace& S = s->S;
  if (!S.direct || !s->d_p2tw) FHESI_FAIL("slot transform: the direct tables of this space were not built");
  const u32 n = (u32)S.phim;
  const Pow2Dev D = sp2_dev(s);
  const unsigned threads = sp2_threads(n);
  const size_t shmem = sp2_shmem(n);
  hipStream_t st = s->ctx->stream;
  const i64 step = 1ll << 30;           // grid.x stays below 2^31
  for (i64 done = 0; done < count; done += step) {
    const unsigned R = (unsigned)std::min(step, count - done);
    if (embed) slots_pow2_embed<<<R, threads, shmem, st>>>(d_in + done * nvals, d_out + done * (i64)n, nvals, take, D);
    else slots_pow2_decode<<<R, threads, shmem, st>>>(d_in + done * (i64)n, d_out + done * nvals, nvals, take, D);
    if (hipGetLastError() != hipSuccess) FHESI_FAIL("slot transform: kernel launch failed");
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/fhesi_hip.h)
extern "C" int fhesi_slots_plan_pow2(int64_t m, uint64_t p, int64_t generator, int64_t* total, int64_t* rows, int64_t* cols, uint64_t* rho0, int32_t* path, int32_t* e_out) {
  SlotSpace S;
  if (const char* why = hm::slot_space_pow2(m, p, generator, &S)) FHESI_FAIL("PlaintextSpace(m=%lld, p=%llu, g=%lld), two rows, refused: %s", (long long)m, (unsigned long long)p, (long long)generator, why);
  slots_describe(S, total, nullptr, rows, cols, rho0, nullptr, path, e_out);
  return 0;
}
extern "C" int fhesi_slots_create_pow2(fhesi_ctx* c, uint64_t p, int64_t generator, fhesi_slots** out) {
  if (!out) FHESI_FAIL("null output pointer");
  *out = nullptr;
  if (!c) FHESI_FAIL("null context");
  SlotSpace S;                                             // the argument checks come first: a refused ring launches nothing
  if (const char* why = hm::slot_space_pow2(c->m, p, generator, &S)) FHESI_FAIL("PlaintextSpace(m=%lld, p=%llu, g=%lld), two rows, refused: %s", (long long)c->m, (unsigned long long)p, (long long)generator, why);
  return slots_make(c, S, out);
}
extern "C" int fhesi_slots_shape(const fhesi_slots* s, int64_t* rows, int64_t* cols, int32_t* path) {
  if (!s) FHESI_FAIL("null slot space");
  slots_describe(s->S, nullptr, nullptr, rows, cols, nullptr, nullptr, path, nullptr);
  return 0;
}
// Which transform a two-row space runs: 0 the direct one (where the plan admits it), anything else the chirp.  Result-neutral: both compute
// the same words; the tables of the other path are built on first request and kept.  For measurements and for the test that compares the two.
extern "C" int fhesi_slots_set_path(fhesi_slots* s, int32_t path) {
  if (!s) FHESI_FAIL("null slot space");
  if (s->S.rows != 2) FHESI_FAIL("fhesi_slots_set_path: not a two-row space");
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  if (path == 0) {
    if (s->S.phim > (1 << 15) || s->S.p >= (1ull << 31)) FHESI_FAIL("fhesi_slots_set_path: the direct transform needs n <= 2^15 and p < 2^31");
    FHESI_TRY(slots_pow2_build(s));
    s->S.direct = true;
  } else {
    if (!s->aux) FHESI_TRY(slots_build(s));
    s->S.direct = false;
  }
  return 0;
}
