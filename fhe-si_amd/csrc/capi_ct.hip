// capi_ct.hip -- ciphertext algebra between multiplications, Encrypt / Decrypt batches, prepared plaintext operands, key generation (include/fhesi_hip.h)
#include "capi_common.h"
#include "wave_plan.h"
#include "poly_plan.h"
#include "conv_plan.h"

// ---- coefficient-domain ciphertext algebra on device batches (kernels_ct.hip)
extern "C" int fhesi_ct_add_dev(fhesi_ctx* c, int32_t logQ, uint64_t* dst, const uint64_t* src, int32_t nparts, int32_t nlimbs, int64_t count) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Ciphertext += : coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  return launch_ct_add(c, (u64*)dst, (const u64*)src, count * nparts * c->phim, nlimbs, logQ);
}
extern "C" int fhesi_ct_mul_long_dev(fhesi_ctx* c, int32_t logQ, uint64_t* ct, int64_t l, int32_t nparts, int32_t nlimbs, int64_t count) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Ciphertext *= long: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  return launch_ct_mul_long(c, (u64*)ct, count * nparts * c->phim, nlimbs, logQ, l);
}
// Ciphertext::operator+=(const ZZX&) / (const ZZ_pX&) on unscaled ciphertexts (Ciphertext.cpp:147-161)
extern "C" int fhesi_ct_add_const_dev(fhesi_ctx* c, int32_t logQ, uint64_t p, uint64_t* ct, int32_t nparts, int32_t nlimbs, int64_t count, const int64_t* poly_host, int32_t npoly) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Ciphertext += ZZX: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (p < 2) FHESI_FAIL("Ciphertext += ZZX: plaintext modulus %llu", (unsigned long long)p);
  if (npoly != 1 && npoly != count) FHESI_FAIL("Ciphertext += ZZX: %d constants for %lld ciphertexts (one for all, or one each)", npoly, (long long)count);
  if (!count) return 0;
  void* d_poly;
  FHESI_TRY(ws_reserve(c, 9, (size_t)npoly * c->phim * 8, &d_poly));
  HIP_TRY(hipMemcpyAsync(d_poly, poly_host, (size_t)npoly * c->phim * 8, hipMemcpyHostToDevice, c->stream));
  const int rc = launch_ct_add_const(c, (u64*)ct, (const i64*)d_poly, npoly, nparts, nlimbs, logQ, p, count);
  HIP_TRY(hipStreamSynchronize(c->stream));        // poly_host may be released on return
  return rc;
}
// Ciphertext::operator*=(const ZZX&) / (const ZZ_pX&) on unscaled ciphertexts (Ciphertext.cpp:245-252 -> CiphertextPart::operator*=(ZZX) :29-36):
// parts[i].poly *= other as INTEGER polynomials, rem Phi_m, Reduce.  The integer product modulo Phi_m is formed in the chain (DoubleCRT of
// both factors, product, toPoly): exact because its coefficients stay below half the chain product, which is checked here.
extern "C" int fhesi_ct_mul_poly_dev(fhesi_ctx* c, int32_t logQ, uint64_t* ct, int32_t nparts, int32_t nlimbs, int64_t count, const int64_t* poly_host, int32_t npoly) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Ciphertext *= ZZX: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (npoly != 1 && npoly != count) FHESI_FAIL("Ciphertext *= ZZX: %d polynomials for %lld ciphertexts (one for all, or one each)", npoly, (long long)count);
  if (!count) return 0;
  const i64 n = c->phim;
  const int L = c->L;
  // |coefficient of the product modulo Phi_m| <= growth * n * 2^(logQ-1) * max|other_j|, growth = 1 (X^n + 1), 2 (the two-term folds of the rings
  // m = q^k and 2 q^k, q an odd prime) or, conservatively, n for a general Phi_m
  u64 maxc = 0;
  for (i64 i = 0; i < (i64)npoly * n; ++i) { const i64 v = poly_host[i]; const u64 a = v < 0 ? (u64)(-(v + 1)) + 1 : (u64)v; if (a > maxc) maxc = a; }
  double bits = (logQ - 1) + std::log2((double)n) + (maxc ? std::log2((double)maxc) + 1e-9 : 0.0) + 1.0;
  bits += c->pow2 ? 0.0 : (c->phi_two_term ? 1.0 : std::log2((double)n));
  const double chain = chain_bits(c);
  if (bits + 1.0 >= chain) FHESI_FAIL("Ciphertext *= ZZX: the product needs %.0f bits, the chain holds %.0f", bits + 1.0, chain);
  const std::vector<int> all = full_set(c);
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  void *d_rows, *d_prow, *d_pl;
  FHESI_TRY(ws_reserve(c, 0, (size_t)count * nparts * L * n * 8, &d_rows));
  FHESI_TRY(ws_reserve(c, 3, (size_t)npoly * L * n * 8, &d_prow));
  FHESI_TRY(ws_reserve(c, 9, (size_t)npoly * n * 8, &d_pl));
  HIP_TRY(hipMemcpyAsync(d_pl, poly_host, (size_t)npoly * n * 8, hipMemcpyHostToDevice, c->stream));      // one signed limb per coefficient
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_pl, 1, n, npoly, 1, nullptr, (u64*)d_prow, L, nullptr));
  FHESI_TRY(row_fwd(c, (u64*)d_prow, npoly, L, nullptr, all.data()));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)ct, nlimbs, n, count, nparts, nullptr, (u64*)d_rows, L, nullptr));
  FHESI_TRY(row_fwd(c, (u64*)d_rows, count * nparts, L, nullptr, all.data()));
  if (npoly == 1) {
    FHESI_TRY(grid_chunks(count * nparts, [&](i64 done, i64 cnt) { return launch_rows_mul_bcast(c, (u64*)d_rows + (size_t)done * L * n, (const u64*)d_rows + (size_t)done * L * n, (const u64*)d_prow, cnt); }));
  } else {
    for (i64 ci = 0; ci < count; ++ci) FHESI_TRY(launch_rows_mul_bcast(c, (u64*)d_rows + (size_t)ci * nparts * L * n, (const u64*)d_rows + (size_t)ci * nparts * L * n, (const u64*)d_prow + (size_t)ci * L * n, nparts));
  }
  FHESI_TRY(row_inv(c, (u64*)d_rows, count * nparts, L, nullptr, all.data()));
  FHESI_TRY(launch_crt(c, t, (const u64*)d_rows, L, nullptr, count * nparts, 2, 0, logQ, (u64*)ct, nlimbs));
  HIP_TRY(hipStreamSynchronize(c->stream));        // poly_host may be released on return
  return 0;
}
extern "C" int fhesi_rows_mul_long_dev(fhesi_ctx* c, uint64_t* rows, int64_t l, int64_t count) {
  CHECK_CTX(c);
  if (!count) return 0;
  std::vector<u64> sc(c->L);
  for (int i = 0; i < c->L; ++i) { const u64 q = c->q[i]; sc[i] = l >= 0 ? (u64)l % q : (q - ((u64)(-(l + 1)) + 1) % q) % q; }
  void* d_sc;
  FHESI_TRY(ws_reserve(c, 9, sizeof(u64) * 64, &d_sc));
  HIP_TRY(hipMemcpyAsync(d_sc, sc.data(), sizeof(u64) * c->L, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));        // sc lives on this stack frame
  return launch_ew_scalar(c, (u64*)rows, (const u64*)d_sc, count, c->L, nullptr, FHESI_OP_MUL);
}
extern "C" int fhesi_ct_gather_dev(fhesi_ctx* c, const uint64_t* pool, const int32_t* idx_host, int64_t count, int64_t words, uint64_t* out) {
  CHECK_CTX(c);
  if (!count) return 0;
  void* d_idx;
  FHESI_TRY(ws_reserve(c, 8, sizeof(int) * (size_t)count, &d_idx));
  HIP_TRY(hipMemcpyAsync(d_idx, idx_host, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));        // the caller's index array may be reused as soon as we return
  return launch_gather(c, (const u64*)pool, (const int*)d_idx, count, words, (u64*)out);
}

// --------------------------------------------------------------------------------------------- Encrypt / Decrypt batches
// FHESIPubKey::Encrypt (FHE-SI.cpp:10-36) for `count` plaintexts whose message polynomials d_msg [count][phi(m)] are already in HBM: the one
// core behind every Encrypt entry point.  The randomness is the caller's (the reference draws it from NTL's PRNG): rand_host =
// [count][3][phi(m)] int64 = (r binary, e0, e1 Gaussian samples before the multiplication by p); or, seeded, drawn in HBM from (seed, first).
// Ends in a synchronise: delta lives on this frame, and rand_host and the array the stage in front uploaded from are the caller's, free to go
// when the entry point returns.  (A slot basis therefore synchronises once per channel.)
static int encrypt_rows_dev(fhesi_ctx* c, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t p, const int64_t* rand_host, bool seeded, u64 seed, u64 first,
                            const i64* d_msg, int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  if (!pk0 || !pk1 || pk0->ctx != c || pk1->ctx != c) FHESI_FAIL("Encrypt: public key belongs to another context");
  if ((int)pk0->idx.size() != c->L || (int)pk1->idx.size() != c->L) FHESI_FAIL("Encrypt: public key must be defined over all primes");
  if (logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Encrypt: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (p < 2) FHESI_FAIL("Encrypt: plaintext modulus must be at least 2");
  if (!count) return 0;
  const i64 n = c->phim;
  const int L = c->L;
  const std::vector<int> all = full_set(c);
  void *d_small, *d_rows, *d_ct, *d_pk, *d_delta;
  FHESI_TRY(ws_reserve(c, 2, (size_t)count * 3 * n * 8, &d_small));
  FHESI_TRY(ws_reserve(c, 0, (size_t)count * 3 * L * n * 8, &d_rows));
  FHESI_TRY(ws_reserve(c, 1, (size_t)count * 2 * L * n * 8, &d_ct));
  FHESI_TRY(ws_reserve(c, 3, (size_t)2 * L * n * 8, &d_pk));
  FHESI_TRY(ws_reserve(c, 4, (size_t)(nlimbs + 1) * 8, &d_delta));
  // delta = floor(2^logQ / p) (FHE-SI.cpp:31), nlimbs limbs
  std::vector<u64> delta(nlimbs, 0);
  { u128 rem = 0; for (int i = nlimbs - 1; i >= 0; --i) { const u64 limb = (i == logQ / 64) ? (1ull << (logQ % 64)) : 0; const u128 cur = (rem << 64) | limb; delta[i] = (u64)(cur / p); rem = cur % p; }
    if (logQ == 64 * nlimbs) { /* 2^logQ needs limb nlimbs: redo with the extra limb */ rem = 1; for (int i = nlimbs - 1; i >= 0; --i) { const u128 cur = rem << 64; delta[i] = (u64)(cur / p); rem = cur % p; } } }
  if (seeded) FHESI_TRY(launch_sample_encrypt(c, (i64*)d_small, count, seed, first));      // r, e0, e1 drawn in HBM (kernels_sample.hip)
  else HIP_TRY(hipMemcpyAsync(d_small, rand_host, (size_t)count * 3 * n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_delta, delta.data(), (size_t)nlimbs * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_pk, pk0->d_rows, (size_t)L * n * 8, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync((u64*)d_pk + (size_t)L * n, pk1->d_rows, (size_t)L * n * 8, hipMemcpyDeviceToDevice, c->stream));
  // DoubleCRT(r), DoubleCRT(e_i) * p: one-limb signed coefficients, the noise lifted by p (FHE-SI.cpp:19-25)
  const u64 lift[3] = {0, p, p};
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_small, 1, n, count, 3, lift, (u64*)d_rows, L, nullptr));
  FHESI_TRY(row_fwd(c, (u64*)d_rows, count * 3, L, nullptr, all.data()));
  FHESI_TRY(launch_encrypt_combine(c, (const u64*)d_rows, (const u64*)d_pk, count, (u64*)d_ct));          // ct[i] = pk[i]*r + e_i (:26-27)
  FHESI_TRY(row_inv(c, (u64*)d_ct, count * 2, L, nullptr, all.data()));                                    // toPoly (:28)
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  FHESI_TRY(launch_crt(c, t, (const u64*)d_ct, L, nullptr, count * 2, 2, 0, logQ, (u64*)out_dev, nlimbs));
  FHESI_TRY(launch_add_scaled_msg(c, (u64*)out_dev, d_msg, (const u64*)d_delta, count, nlimbs, logQ));     // += delta*msg, Reduce (:31-35)
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the stages in front of the core.  Each checks its own arguments and leaves the message polynomials [rows][phi(m)] in workspace slot 5
// (slot values pass through slot 9: dead before the transforms of the encryption start); nothing here synchronises -- the core does.
static int ws_i64(fhesi_ctx* c, int slot, size_t bytes, i64** out) { void* d; FHESI_TRY(ws_reserve(c, slot, bytes, &d)); *out = (i64*)d; return 0; }
static int msg_staging(fhesi_ctx* c, i64 rows, i64** d_msg) { return ws_i64(c, 5, (size_t)rows * c->phim * 8, d_msg); }
static int upload_vals(fhesi_ctx* c, const int64_t* vals_host, size_t bytes, i64** d_vals) {
  FHESI_TRY(ws_i64(c, 9, bytes, d_vals));
  HIP_TRY(hipMemcpyAsync(*d_vals, vals_host, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
static int stage_msg_host(fhesi_ctx* c, const int64_t* msg_host, i64 count, i64** d_msg) {      // [count][phi(m)] coefficient form
  if (count <= 0) return 0;
  FHESI_TRY(msg_staging(c, count, d_msg));
  HIP_TRY(hipMemcpyAsync(*d_msg, msg_host, (size_t)count * c->phim * 8, hipMemcpyHostToDevice, c->stream));
  return 0;
}
static int stage_msg_slots(fhesi_ctx* c, fhesi_slots* s, const int64_t* vals_host, i64 nvals, bool only_usable, i64 count, i64** d_msg, const char* what = "Encrypt") {      // [count][nvals] slot values
  if (!s) FHESI_FAIL("%s: null plaintext space", what);
  if (s->ctx != c) FHESI_FAIL("%s: the plaintext space belongs to another context", what);
  if (!vals_host) FHESI_FAIL("%s: null slot values", what);
  FHESI_TRY(slots_check_shape(what, nvals, count, s->S.phim));
  if (!count) return 0;
  i64* d_vals;
  FHESI_TRY(msg_staging(c, count, d_msg));
  FHESI_TRY(upload_vals(c, vals_host, (size_t)count * nvals * 8, &d_vals));
  return slots_embed_rows(s, d_vals, nvals, only_usable, count, *d_msg);
}
// Regression::GenerateNoise masks: slot 0 zero, the others uniform from (seed, first + i) (Regression.h:181-185); all phi(m) slots embedded (:188)
static int stage_msg_noise(fhesi_ctx* c, fhesi_slots* s, u64 seed, u64 first, i64 count, i64** d_msg) {
  if (!s) FHESI_FAIL("GenerateNoise: null plaintext space");
  if (s->ctx != c) FHESI_FAIL("Encrypt: the plaintext space belongs to another context");
  if (count <= 0) return 0;
  i64* d_vals;
  FHESI_TRY(msg_staging(c, count, d_msg));
  FHESI_TRY(ws_i64(c, 9, (size_t)count * c->phim * 8, &d_vals));
  FHESI_TRY(slots_noise_rows(s, seed, first, count, d_vals));
  return slots_embed_rows(s, d_vals, c->phim, false, count, *d_msg);
}
// a slot basis (kernels_slots_basis.hip): one embedding launch for all k channels, [k][count][phi(m)]
static int basis_check(fhesi_ctx* c, const fhesi_slots_basis* b, const char* what, i64 nvals, i64 count) {
  if (!b) FHESI_FAIL("%s: null slot basis", what);
  if (b->ctx != c) FHESI_FAIL("%s: the slot basis belongs to another context", what);
  return slots_check_shape(what, nvals, count, c->phim);
}
static int stage_msg_basis(fhesi_ctx* c, fhesi_slots_basis* b, const int64_t* vals_host, int L_in, i64 nvals, i64 count, i64** d_msg) {      // [count][nvals][L_in] limbs
  FHESI_TRY(basis_check(c, b, "Encrypt", nvals, count));
  if (!vals_host) FHESI_FAIL("Encrypt: null slot values");
  if (L_in < 1 || L_in > hm::SlotBasis::MAXL) FHESI_FAIL("Encrypt: %d limbs per value, 1 .. %d are taken", L_in, hm::SlotBasis::MAXL);
  if (!count) return 0;
  i64* d_vals;
  FHESI_TRY(msg_staging(c, b->B.k * count, d_msg));
  FHESI_TRY(upload_vals(c, vals_host, (size_t)count * nvals * L_in * 8, &d_vals));
  return slots_basis_embed_rows(b, d_vals, L_in, nvals, count, *d_msg);
}

extern "C" int fhesi_encrypt_batch(fhesi_ctx* c, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t p, const int64_t* rand_host,
                                   const int64_t* msg_host, int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  if (!rand_host) FHESI_FAIL("Encrypt: null randomness (fhesi_encrypt_batch_seeded draws it on the device)");
  CHECK_CTX(c);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_host(c, msg_host, count, &d_msg));
  return encrypt_rows_dev(c, pk0, pk1, logQ, p, rand_host, false, 0, 0, d_msg, count, out_dev, nlimbs);
}
// ... with the randomness drawn on the device: plaintext i takes the streams of object index first_index + i (philox.h)
extern "C" int fhesi_encrypt_batch_seeded(fhesi_ctx* c, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t p, uint64_t seed, uint64_t first_index,
                                          const int64_t* msg_host, int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_host(c, msg_host, count, &d_msg));
  return encrypt_rows_dev(c, pk0, pk1, logQ, p, nullptr, true, seed, first_index, d_msg, count, out_dev, nlimbs);
}
// ... of plaintexts given as slot values (Plaintext(context, vector) + Encrypt): the message polynomials are embedded on the device and never
// leave HBM.  Bit for bit fhesi_encrypt_batch_seeded(fhesi_slots_embed(vals)) under the same (seed, index).
extern "C" int fhesi_encrypt_slots_batch_seeded(fhesi_ctx* c, fhesi_slots* s, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                                const int64_t* vals_host, int64_t nvals, int32_t only_usable, int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_slots(c, s, vals_host, nvals, only_usable != 0, count, &d_msg));
  return encrypt_rows_dev(c, pk0, pk1, logQ, s->S.p, nullptr, true, seed, first_index, d_msg, count, out_dev, nlimbs);
}
// Regression::GenerateNoise (Regression.h:180-191) for `count` masks: slot 0 is 0, slots 1 .. phi(m)-1 are uniform on [0, p), drawn on the device
// from (seed, first_index + i, slot, purpose 7) (philox.h); all phi(m) slots embedded, then an ordinary encryption under the same (seed, index)
extern "C" int fhesi_encrypt_noise_batch_seeded(fhesi_ctx* c, fhesi_slots* s, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                                int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_noise(c, s, seed, first_index, count, &d_msg));
  return encrypt_rows_dev(c, pk0, pk1, logQ, s->S.p, nullptr, true, seed, first_index, d_msg, count, out_dev, nlimbs);
}
// ... over a slot basis: k channels on one key set, channel ch with p = p_ch reading its part of the staging; object index of channel ch,
// plaintext i: first_index + ch count + i
extern "C" int fhesi_encrypt_int_slots_batch_seeded(fhesi_ctx* c, fhesi_slots_basis* b, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                                    const int64_t* vals_host, int32_t L_in, int64_t nvals, int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_basis(c, b, vals_host, L_in, nvals, count, &d_msg));
  const size_t n = (size_t)c->phim;
  for (int ch = 0; ch < b->B.k; ++ch)
    FHESI_TRY(encrypt_rows_dev(c, pk0, pk1, logQ, b->B.primes[ch], nullptr, true, seed, first_index + (u64)ch * (u64)count, d_msg + ch * count * n, count,
                               out_dev + ch * count * 2 * n * nlimbs, nlimbs));
  return 0;
}
extern "C" int fhesi_encrypt_noise_int_batch_seeded(fhesi_ctx* c, fhesi_slots_basis* b, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                                    int64_t count, uint64_t* out_dev, int32_t nlimbs) {
  CHECK_CTX(c);
  FHESI_TRY(basis_check(c, b, "GenerateNoise", 1, count));
  for (int ch = 0; ch < b->B.k; ++ch)
    FHESI_TRY(fhesi_encrypt_noise_batch_seeded(c, b->ch[ch], pk0, pk1, logQ, seed, first_index + (u64)ch * (u64)count, count, out_dev + (size_t)ch * count * 2 * c->phim * nlimbs, nlimbs));
  return 0;
}

// FHESISecKey::Decrypt (FHE-SI.cpp:93-119) of `count` unscaled 2-part ciphertexts [count][2][phi(m)][nlimbs] in HBM, up to the rounding: leaves
// z = c0 + c1 t (toPoly, the low logQ+1 bits kept) in workspace slot 2 as [count][phi(m)][nw] words.  The checks of every Decrypt entry point.
static int decrypt_z_dev(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count, u64** d_zw, int* nw_out) {
  CHECK_CTX(c);
  if (!sk1 || sk1->ctx != c) FHESI_FAIL("Decrypt: secret key belongs to another context");
  if ((int)sk1->idx.size() != c->L) FHESI_FAIL("Decrypt: secret key must be defined over all primes");
  if (logQ < 1 || nlimbs < 1) FHESI_FAIL("Decrypt: bad shape");
  if (p < 2 || p >= (1ull << 62)) FHESI_FAIL("Decrypt: plaintext modulus out of range");
  const i64 n = c->phim;
  const int L = c->L, nw = (logQ + 1 + 63) / 64;
  *nw_out = nw;
  *d_zw = nullptr;
  if (!count) return 0;
  const std::vector<int> all = full_set(c);
  void *d_rows, *d_z, *d_big;
  FHESI_TRY(ws_reserve(c, 0, (size_t)count * 2 * L * n * 8, &d_rows));
  FHESI_TRY(ws_reserve(c, 1, (size_t)count * L * n * 8, &d_z));
  FHESI_TRY(ws_reserve(c, 2, (size_t)count * n * nw * 8, &d_big));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)ct_dev, nlimbs, n, count, 2, nullptr, (u64*)d_rows, L, nullptr));     // DoubleCRT(parts[i]) (:98-101)
  FHESI_TRY(row_fwd(c, (u64*)d_rows, count * 2, L, nullptr, all.data()));
  FHESI_TRY(launch_decrypt_dot(c, (const u64*)d_rows, sk1->d_rows, count, (u64*)d_z));                              // DotProduct with (1, t) (:105-107)
  FHESI_TRY(row_inv(c, (u64*)d_z, count, L, nullptr, all.data()));
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  FHESI_TRY(launch_crt(c, t, (const u64*)d_z, L, nullptr, count, 0, 0, 0, (u64*)d_big, nw));                         // toPoly, low logQ+1 bits kept
  *d_zw = (u64*)d_big;
  return 0;
}
// ... and the rounding: the one core behind every Decrypt entry point.  Leaves round(p z / q) mod p in d_msg [count][phi(m)] (HBM) and returns;
// only enqueues, and reads no host array.
static int decrypt_rows_dev(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count, i64* d_msg) {
  u64* d_zw;
  int nw;
  FHESI_TRY(decrypt_z_dev(c, sk1, logQ, p, ct_dev, nlimbs, count, &d_zw, &nw));
  if (!count) return 0;
  return launch_decrypt_round(c, d_zw, count * c->phim, nw, logQ, p, d_msg);                                         // round(p z / q) mod p (:110-116)
}
// ---- behind the core: the message staging in slot 5 for the core to fill; slot values, once the transforms of the decryption are enqueued,
// in slot 9; the host copy and the synchronise every Decrypt entry point ends in
static int copy_out(fhesi_ctx* c, int64_t* out_host, const i64* d, size_t bytes) {
  if (bytes) HIP_TRY(hipMemcpyAsync(out_host, d, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int fhesi_decrypt_batch(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                   int64_t* msg_host) {
  CHECK_CTX(c);
  i64* d_msg;
  FHESI_TRY(msg_staging(c, count, &d_msg));
  FHESI_TRY(decrypt_rows_dev(c, sk1, logQ, p, ct_dev, nlimbs, count, d_msg));
  return copy_out(c, msg_host, d_msg, (size_t)count * c->phim * 8);
}
// ... followed by Plaintext::DecodeSlots (Test_Regression.cpp:47-58: Decrypt, DecodeSlots, msgs[0]) on the message polynomials where they
// are: vals_host [count][nvals]
extern "C" int fhesi_decrypt_slots_batch(fhesi_ctx* c, fhesi_slots* s, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                         int64_t nvals, int32_t only_usable, int64_t* vals_host) {
  CHECK_CTX(c);
  if (!s) FHESI_FAIL("Decrypt: null plaintext space");
  if (s->ctx != c) FHESI_FAIL("Decrypt: the plaintext space belongs to another context");
  FHESI_TRY(slots_check_shape("Decrypt", nvals, count, s->S.phim));
  const size_t bv = (size_t)count * nvals * 8;
  i64 *d_msg, *d_vals;
  FHESI_TRY(msg_staging(c, count, &d_msg));
  FHESI_TRY(decrypt_rows_dev(c, sk1, logQ, s->S.p, ct_dev, nlimbs, count, d_msg));
  FHESI_TRY(ws_i64(c, 9, bv, &d_vals));
  FHESI_TRY(slots_decode_rows(s, d_msg, count, nvals, only_usable != 0, d_vals));
  return copy_out(c, vals_host, d_vals, bv);
}
// ... over a slot basis: k decryptions leave their message polynomials in the staging [k][count][phi(m)]; one decoding launch and one
// recombination follow
extern "C" int fhesi_decrypt_int_slots_batch(fhesi_ctx* c, fhesi_slots_basis* b, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                             int64_t nvals, int64_t* vals_host) {
  CHECK_CTX(c);
  FHESI_TRY(basis_check(c, b, "Decrypt", nvals, count));
  if (!vals_host) FHESI_FAIL("Decrypt: null output");
  const size_t n = (size_t)c->phim, bv = (size_t)count * nvals * b->B.limbs * 8;
  i64 *d_msg, *d_vals;
  FHESI_TRY(msg_staging(c, b->B.k * count, &d_msg));
  for (int ch = 0; ch < b->B.k; ++ch)
    FHESI_TRY(decrypt_rows_dev(c, sk1, logQ, b->B.primes[ch], ct_dev + ch * count * 2 * n * nlimbs, nlimbs, count, d_msg + ch * count * n));
  FHESI_TRY(ws_i64(c, 9, bv, &d_vals));
  FHESI_TRY(slots_basis_decode_rows(b, d_msg, count, nvals, d_vals));
  return copy_out(c, vals_host, d_vals, bv);
}

// ---- the noise budget (include/fhesi_hip.h): the same z, the rounding that keeps its remainder (launch_decrypt_noise).  Workspace slot 4 holds
// [rows][nw] maxima, [rows] budgets, then the per-block maxima of one chunk of at most `count` ciphertexts; rows = count, or k count for a slot basis.
struct NoiseWs { u64 *maxres, *part; int* budget; };
// the rows in front of the rounding put two polynomials per ciphertext on grid.y: batches of at most kNoiseChunk ciphertexts, one after the other
static const i64 kNoiseChunk = 32767;
static int noise_ws(fhesi_ctx* c, int32_t logQ, i64 rows, i64 count, NoiseWs* w) {
  if (logQ < 1) FHESI_FAIL("Decrypt: bad shape");
  const size_t nw = (size_t)(logQ + 1 + 63) / 64, head = (size_t)rows * nw * 8 + (((size_t)rows * 4 + 7) & ~(size_t)7);
  void* d;
  FHESI_TRY(ws_reserve(c, 4, head + (size_t)std::min<i64>(count, kNoiseChunk) * noise_blocks(c) * nw * 8, &d));
  w->maxres = (u64*)d;
  w->budget = (int*)(w->maxres + (size_t)rows * nw);
  w->part = (u64*)((char*)d + head);
  return 0;
}
static int noise_rows_dev(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count, i64* d_msg, const NoiseWs& w, i64 row0) {
  const i64 n = c->phim;
  for (i64 done = 0; done < count || !done; done += kNoiseChunk) {              // (count = 0 still runs the checks)
    const i64 cnt = std::min<i64>(kNoiseChunk, count - done);
    u64* d_zw;
    int nw;
    FHESI_TRY(decrypt_z_dev(c, sk1, logQ, p, ct_dev + (size_t)done * 2 * n * nlimbs, nlimbs, cnt, &d_zw, &nw));
    FHESI_TRY(launch_decrypt_noise(c, d_zw, cnt, nw, logQ, p, d_msg ? d_msg + done * n : nullptr, w.part, w.maxres + (row0 + done) * nw, w.budget + row0 + done));
  }
  return 0;
}
static int noise_copy_out(fhesi_ctx* c, int32_t logQ, const NoiseWs& w, i64 rows, int32_t* budget_host, uint64_t* maxres_host) {
  const size_t nw = (size_t)(logQ + 1 + 63) / 64;
  if (rows) HIP_TRY(hipMemcpyAsync(budget_host, w.budget, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && maxres_host) HIP_TRY(hipMemcpyAsync(maxres_host, w.maxres, (size_t)rows * nw * 8, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
extern "C" int fhesi_ct_noise_batch(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                    int32_t* budget_host, uint64_t* maxres_host) {
  CHECK_CTX(c);
  if (count < 0) FHESI_FAIL("noise budget: negative count");
  if (!budget_host) FHESI_FAIL("noise budget: null output");
  NoiseWs w;
  FHESI_TRY(noise_ws(c, logQ, count, count, &w));
  FHESI_TRY(noise_rows_dev(c, sk1, logQ, p, ct_dev, nlimbs, count, nullptr, w, 0));
  FHESI_TRY(noise_copy_out(c, logQ, w, count, budget_host, maxres_host));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int fhesi_decrypt_noise_batch(fhesi_ctx* c, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                         int64_t* msg_host, int32_t* budget_host, uint64_t* maxres_host) {
  CHECK_CTX(c);
  if (count < 0) FHESI_FAIL("noise budget: negative count");
  if (!msg_host || !budget_host) FHESI_FAIL("noise budget: null output");
  NoiseWs w;
  i64* d_msg;
  FHESI_TRY(noise_ws(c, logQ, count, count, &w));
  FHESI_TRY(msg_staging(c, count, &d_msg));
  FHESI_TRY(noise_rows_dev(c, sk1, logQ, p, ct_dev, nlimbs, count, d_msg, w, 0));
  FHESI_TRY(noise_copy_out(c, logQ, w, count, budget_host, maxres_host));
  return copy_out(c, msg_host, d_msg, (size_t)count * c->phim * 8);
}
// ... over a slot basis: channel ch with p = p_ch on its part of ct_dev, the layout of fhesi_decrypt_int_slots_batch; budget_host [k][count]
extern "C" int fhesi_ct_noise_int_batch(fhesi_ctx* c, fhesi_slots_basis* b, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                                        int32_t* budget_host) {
  CHECK_CTX(c);
  FHESI_TRY(basis_check(c, b, "noise budget", 1, count));
  if (!budget_host) FHESI_FAIL("noise budget: null output");
  NoiseWs w;
  FHESI_TRY(noise_ws(c, logQ, b->B.k * count, count, &w));
  for (int ch = 0; ch < b->B.k; ++ch)
    FHESI_TRY(noise_rows_dev(c, sk1, logQ, b->B.primes[ch], ct_dev + (size_t)ch * count * 2 * c->phim * nlimbs, nlimbs, count, nullptr, w, ch * count));
  FHESI_TRY(noise_copy_out(c, logQ, w, b->B.k * count, budget_host, nullptr));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// --------------------------------------------------------------------------------------------- prepared plaintext operands
// fhesi_plain (include/fhesi_hip.h): the one core behind both constructors.  d_msg [nw][phi(m)] int64 message polynomials in HBM (a stage above
// left them in workspace slot 5) -> DoubleCRT rows over all primes, owned by the handle.  Synchronises: the array the stage uploaded from is the
// caller's again on return.
// In two halves, for a stage that makes its message polynomials in chunks (a grid of linear blocks): the handle with its rows allocated and nothing in
// them -- not yet a live handle of the context --, and the rows [row0, row0 + nrows) from d_msg [nrows][phi(m)], enqueued.
static int plain_alloc(fhesi_ctx* c, i64 nw, u64 maxabs, u64 p, fhesi_plain** out) {
  fhesi_plain* w = new fhesi_plain();
  w->ctx = c; w->nw = nw; w->maxabs = maxabs; w->p = p;
  const size_t bytes = (size_t)nw * c->L * c->phim * 8;
  if (hipMalloc(&w->d_rows, bytes) != hipSuccess) { (void)hipGetLastError(); delete w; FHESI_FAIL("prepared plaintext: hipMalloc of %zu bytes failed", bytes); }
  *out = w;
  return 0;
}
static int plain_rows_fill(fhesi_ctx* c, fhesi_plain* w, i64 row0, const i64* d_msg, i64 nrows) {
  const std::vector<int> all = full_set(c);
  u64* rows = w->d_rows + (size_t)row0 * c->L * c->phim;
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_msg, 1, c->phim, nrows, 1, nullptr, rows, c->L, nullptr));      // one signed limb per coefficient
  return row_fwd(c, rows, nrows, c->L, nullptr, all.data());
}
// closes what the two halves began: waits for the transforms and counts the handle, or releases it (rc: how the fills went)
static int plain_rows_close(fhesi_ctx* c, fhesi_plain* w, int rc, fhesi_plain** out) {
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { fhesi_set_error("prepared plaintext: the transforms failed"); rc = 1; }
  if (rc) { hipStreamSynchronize(c->stream); hipFree(w->d_rows); delete w; return rc; }
  ++c->live_handles;
  *out = w;
  return 0;
}
static int plain_rows_dev(fhesi_ctx* c, const i64* d_msg, i64 nw, u64 maxabs, u64 p, fhesi_plain** out) {
  fhesi_plain* w;
  FHESI_TRY(plain_alloc(c, nw, maxabs, p, &w));
  return plain_rows_close(c, w, plain_rows_fill(c, w, 0, d_msg, nw), out);
}
extern "C" int fhesi_plain_create_slots(fhesi_slots* s, const int64_t* vals_host, int64_t nvals, int32_t only_usable, int64_t nw, fhesi_plain** out) {
  if (!out) FHESI_FAIL("prepared plaintext: null output pointer");
  *out = nullptr;
  if (!s) FHESI_FAIL("prepared plaintext: null plaintext space");
  fhesi_ctx* c = s->ctx;
  CHECK_CTX(c);
  if (nw < 1 || nw > 65535) FHESI_FAIL("prepared plaintext: %lld plaintexts per handle, 1 .. 65535 are taken", (long long)nw);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_slots(c, s, vals_host, nvals, only_usable != 0, nw, &d_msg, "prepared plaintext"));
  return plain_rows_dev(c, d_msg, nw, s->S.p - 1, s->S.p, out);      // the embedding leaves coefficients in [0, p)
}
extern "C" int fhesi_plain_create_poly(fhesi_ctx* c, const int64_t* poly_host, int64_t nw, fhesi_plain** out) {
  if (!out) FHESI_FAIL("prepared plaintext: null output pointer");
  *out = nullptr;
  CHECK_CTX(c);
  if (!poly_host) FHESI_FAIL("prepared plaintext: null polynomial");
  if (nw < 1 || nw > 65535) FHESI_FAIL("prepared plaintext: %lld plaintexts per handle, 1 .. 65535 are taken", (long long)nw);
  u64 maxc = 0;
  for (i64 i = 0; i < nw * c->phim; ++i) { const i64 v = poly_host[i]; const u64 a = v < 0 ? (u64)(-(v + 1)) + 1 : (u64)v; if (a > maxc) maxc = a; }
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_host(c, poly_host, nw, &d_msg));
  return plain_rows_dev(c, d_msg, nw, maxc, 0, out);
}
extern "C" int fhesi_plain_free(fhesi_plain* w) {
  if (!w) return 0;
  hipSetDevice(w->ctx->device);
  hipStreamSynchronize(w->ctx->stream);
  --w->ctx->live_handles;
  hipFree(w->d_rows);
  delete w;
  return 0;
}
extern "C" int fhesi_plain_info(const fhesi_plain* w, int64_t* nw, uint64_t* maxabs, uint64_t* p) {
  if (!w) FHESI_FAIL("null prepared plaintext");
  if (nw) *nw = w->nw;
  if (maxabs) *maxabs = w->maxabs;
  if (p) *p = w->p;
  return 0;
}
// host only: no device, no context
extern "C" int fhesi_plain_sum_bits(int64_t m, int32_t logQ, uint64_t maxabs, int64_t terms, double* bits) {
  if (!bits) FHESI_FAIL("plain_sum_bits: null output");
  if (m < 2 || m > ((i64)1 << 20)) FHESI_FAIL("plain_sum_bits: m=%lld outside [2, 2^20]", (long long)m);
  if (logQ < 1) FHESI_FAIL("plain_sum_bits: logQ=%d", logQ);
  if (terms < 0) FHESI_FAIL("plain_sum_bits: %lld terms", (long long)terms);
  i64 n = 0;
  hm::zms_idx(m, &n);
  const bool pow2 = (m & (m - 1)) == 0 && m >= 4;      // the classes fhesi_ctx_create records (pow2, phi_two_term)
  *bits = plain_sum_bits(n, pow2, !pow2 && hm::prime_power_ring(m, nullptr) != 0, logQ, maxabs, terms);
  return 0;
}

// out[g] = sum_{t in [seg[g], seg[g+1])} pool[a_idx[t]] (*) w[b_idx[t]] on unscaled two-part ciphertexts (include/fhesi_hip.h).  The host plans
// passes: groups [g, g2) whose distinct ciphertexts and whose sums both fit the rows one pass may hold; a single group with more distinct
// ciphertexts than that is summed piecewise into the same rows.  The index lists of ALL passes are uploaded once, in front of the first launch.
extern "C" int fhesi_ct_plain_sum_dev(fhesi_ctx* c, const fhesi_plain* w, int32_t logQ, const uint64_t* pool, int64_t npool, int32_t nlimbs,
                                      const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, uint64_t* out) {
  CHECK_CTX(c);
  if (!w) FHESI_FAIL("ct_plain_sum: null prepared plaintext");
  if (w->ctx != c) FHESI_FAIL("ct_plain_sum: the prepared plaintext belongs to another context");
  if (nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("ct_plain_sum: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (ngroups < 0 || npool < 0) FHESI_FAIL("ct_plain_sum: negative count");
  if (!ngroups) return 0;
  if (!seg || !out) FHESI_FAIL("ct_plain_sum: null argument");
  if (seg[0] != 0) FHESI_FAIL("ct_plain_sum: seg must start at 0, got %d", seg[0]);
  i64 tmax = 0;
  for (i64 g = 0; g < ngroups; ++g) {
    if (seg[g + 1] < seg[g]) FHESI_FAIL("ct_plain_sum: seg is not non-decreasing at group %lld (%d after %d)", (long long)g, seg[g + 1], seg[g]);
    tmax = std::max<i64>(tmax, seg[g + 1] - seg[g]);
  }
  const i64 nterms = seg[ngroups];
  if (nterms && (!a_idx || !b_idx || !pool)) FHESI_FAIL("ct_plain_sum: null argument");
  for (i64 t = 0; t < nterms; ++t) {
    if (a_idx[t] < 0 || a_idx[t] >= npool) FHESI_FAIL("ct_plain_sum: ciphertext index %d of term %lld out of range (pool of %lld)", a_idx[t], (long long)t, (long long)npool);
    if (b_idx[t] < 0 || b_idx[t] >= w->nw) FHESI_FAIL("ct_plain_sum: plaintext index %d of term %lld out of range (%lld prepared)", b_idx[t], (long long)t, (long long)w->nw);
  }
  const i64 n = c->phim;
  const int L = c->L;
  const i64 ct_words = (i64)2 * n * nlimbs, row_words = (i64)2 * L * n;
  {
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)ngroups * ct_words * 8, p0 = (uintptr_t)pool, p1 = p0 + (size_t)npool * ct_words * 8;
    if (npool && o0 < p1 && p0 < o1) FHESI_FAIL("ct_plain_sum: out overlaps pool");
  }
  const double chain = chain_bits(c);
  const double bits = plain_sum_bits(n, c->pow2, c->phi_two_term, logQ, w->maxabs, tmax);
  if (bits >= chain) FHESI_FAIL("ct_plain_sum: a sum of %lld products needs %.0f bits, the chain holds %.0f", (long long)tmax, std::ceil(bits), std::floor(chain));
  const std::vector<int> all = full_set(c);
  CrtTables* t_all;
  FHESI_TRY(get_crt_tables(c, all, &t_all));
  // rows of one pass: the distinct ciphertexts' and the sums', about 4 GiB each (option "wave_operands": at most that many of either, for tests)
  i64 cap = (i64)(4.0 * 1024 * 1024 * 1024 / ((double)row_words * 8));
  if (cap > 32767) cap = 32767;                             // (the reduction and the CRT put two polynomials per ciphertext on grid.y)
  if (c->opt.wave_operands > 0 && c->opt.wave_operands < cap) cap = c->opt.wave_operands;
  if (cap < 1) cap = 1;
  // ---- plan (wave_plan.h): the passes and, in one index array, per pass [distinct pool entries][local ciphertext slot per term][plaintext index per term][segment bounds]
  const WavePlan plan = wave_plan(a_idx, b_idx, seg, ngroups, cap, cap, false);
  const std::vector<int>& ix = plan.ix;
  void* d_ix;
  FHESI_TRY(ws_reserve(c, 5, sizeof(int) * ix.size(), &d_ix));
  HIP_TRY(hipMemcpyAsync(d_ix, ix.data(), sizeof(int) * ix.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                 // the one synchronisation: ix lives on this frame, a_idx / b_idx / seg are read no more
  i64 max_nu = 0, max_ng = 0;
  for (const WavePass& P : plan.passes) { max_nu = std::max<i64>(max_nu, P.nua); max_ng = std::max<i64>(max_ng, P.ng); }
  void *d_ops, *d_rows, *d_sum;
  FHESI_TRY(ws_reserve(c, 7, (size_t)max_nu * ct_words * 8, &d_ops));
  FHESI_TRY(ws_reserve(c, 0, (size_t)max_nu * row_words * 8, &d_rows));
  FHESI_TRY(ws_reserve(c, 4, (size_t)max_ng * row_words * 8, &d_sum));
  for (const WavePass& P : plan.passes) {
    const int* dix = (const int*)d_ix + P.off;
    if (P.nua) {
      FHESI_TRY(launch_gather(c, (const u64*)pool, dix, P.nua, ct_words, (u64*)d_ops));
      FHESI_TRY(launch_rns_reduce(c, (const u64*)d_ops, nlimbs, n, P.nua, 2, nullptr, (u64*)d_rows, L, nullptr));
      FHESI_TRY(row_fwd(c, (u64*)d_rows, P.nua * 2, L, nullptr, all.data()));
    }
    FHESI_TRY(launch_plain_sum(c, (const u64*)d_rows, w->d_rows, dix + P.nua, dix + P.nua + P.nt, dix + P.nua + 2 * P.nt, P.ng, P.accumulate, (u64*)d_sum, (double)P.nt));
    if (!P.close) continue;
    FHESI_TRY(row_inv(c, (u64*)d_sum, P.ng * 2, L, nullptr, all.data()));
    FHESI_TRY(launch_crt(c, t_all, (const u64*)d_sum, L, nullptr, P.ng * 2, 2, 0, logQ, (u64*)out + (size_t)P.g * ct_words, nlimbs));
  }
  return 0;
}
// out[g] = Reduce_logQ(sum_{t in [seg[g], seg[g+1])} coef[t] pool[a_idx[t]] + konst[g]) on unscaled two-part ciphertexts (include/fhesi_hip.h): one launch of
// ct_lin_comb_kernel per 65535 polynomials, whatever the number of terms.  The lists (lin_comb_lists, poly_plan.h) are uploaded once, in front of the first
// launch, into workspace slot 5: [magnitudes][constants][pool indices][bounds].
extern "C" int fhesi_ct_lin_comb_dev(fhesi_ctx* c, int32_t logQ, uint64_t p, const uint64_t* pool, int64_t npool, int32_t nlimbs, const int32_t* a_idx,
                                     const int64_t* coef, const int32_t* seg, const int64_t* konst, int64_t ngroups, uint64_t* out) {
  CHECK_CTX(c);
  if (nlimbs < 1 || nlimbs > 32) FHESI_FAIL("ct_lin_comb: ciphertext coefficients of %d limbs are outside the supported 1..32", nlimbs);
  if (logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("ct_lin_comb: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (p < 2) FHESI_FAIL("ct_lin_comb: plaintext modulus %llu", (unsigned long long)p);
  if (ngroups < 0 || npool < 0) FHESI_FAIL("ct_lin_comb: negative count");
  if (!ngroups) return 0;
  if (!seg || !out) FHESI_FAIL("ct_lin_comb: null argument");
  if (seg[0] != 0) FHESI_FAIL("ct_lin_comb: seg must start at 0, got %d", seg[0]);
  for (i64 g = 0; g < ngroups; ++g)
    if (seg[g + 1] < seg[g]) FHESI_FAIL("ct_lin_comb: seg is not non-decreasing at group %lld (%d after %d)", (long long)g, seg[g + 1], seg[g]);
  const i64 nterms = seg[ngroups];
  if (nterms && (!a_idx || !coef || !pool)) FHESI_FAIL("ct_lin_comb: null argument");
  for (i64 t = 0; t < nterms; ++t)
    if (a_idx[t] < 0 || a_idx[t] >= npool) FHESI_FAIL("ct_lin_comb: ciphertext index %d of term %lld out of range (pool of %lld)", a_idx[t], (long long)t, (long long)npool);
  const size_t ct_bytes = (size_t)2 * c->phim * nlimbs * 8;
  {
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)ngroups * ct_bytes, p0 = (uintptr_t)pool, p1 = p0 + (size_t)npool * ct_bytes;
    if (pool && npool && o0 < p1 && p0 < o1) FHESI_FAIL("ct_lin_comb: out overlaps pool");
  }
  const LinCombLists L = lin_comb_lists(a_idx, coef, seg, ngroups);
  const size_t nt = L.idx.size(), ng = (size_t)ngroups, nk = konst ? ng : 0;
  void* d;
  FHESI_TRY(ws_reserve(c, 5, (nt + nk) * 8 + (nt + 3 * ng) * 4, &d));
  u64* d_mag = (u64*)d;
  i64* d_konst = (i64*)(d_mag + nt);
  int* d_idx = (int*)(d_konst + nk);
  int* d_bounds = d_idx + nt;
  if (nt) HIP_TRY(hipMemcpyAsync(d_mag, L.mag.data(), nt * 8, hipMemcpyHostToDevice, c->stream));
  if (nk) HIP_TRY(hipMemcpyAsync(d_konst, konst, nk * 8, hipMemcpyHostToDevice, c->stream));
  if (nt) HIP_TRY(hipMemcpyAsync(d_idx, L.idx.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_bounds, L.bounds.data(), 3 * ng * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                 // the one synchronisation: the lists live on this frame, konst is the caller's again on return
  return launch_ct_lin_comb(c, (const u64*)pool, d_idx, d_mag, d_bounds, nk ? d_konst : nullptr, ngroups, nlimbs, logQ, p, (u64*)out);
}
// Ciphertext::operator+=(const ZZX&) unscaled (Ciphertext.cpp:147-156) with the constant given as slot values: the embed stage, then the kernel
// behind fhesi_ct_add_const_dev on the message polynomials where they are
extern "C" int fhesi_ct_add_slots_dev(fhesi_ctx* c, fhesi_slots* s, int32_t logQ, uint64_t* ct, int32_t nparts, int32_t nlimbs, int64_t count,
                                      const int64_t* vals_host, int64_t nvals, int32_t only_usable, int64_t nv) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs < 1 || logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("Ciphertext += slots: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (count < 0) FHESI_FAIL("Ciphertext += slots: negative count");
  if (nv != 1 && nv != count) FHESI_FAIL("Ciphertext += slots: %lld constants for %lld ciphertexts (one for all, or one each)", (long long)nv, (long long)count);
  i64* d_msg = nullptr;
  FHESI_TRY(stage_msg_slots(c, s, vals_host, nvals, only_usable != 0, nv, &d_msg, "Ciphertext += slots"));
  const size_t n = (size_t)c->phim;
  FHESI_TRY(grid_chunks(count, [&](i64 done, i64 cnt) {
    return launch_ct_add_const(c, (u64*)ct + (size_t)done * nparts * n * nlimbs, d_msg + (nv == 1 ? 0 : (size_t)done * n), nv == 1 ? 1 : (int)cnt, nparts, nlimbs, logQ, s->S.p, cnt);
  }));
  HIP_TRY(hipStreamSynchronize(c->stream));        // vals_host may be released on return
  return 0;
}

// --------------------------------------------------------------------------------------------- layers on packed slots: the stage and the constructor
// fhesi_linear, fhesi_linear_grid, fhesi_conv2d (include/fhesi_hip.h; GridLayer, fhesi_internal.h).  The stage next to stage_msg_slots.  A layer is nI nJ
// units (blocks, channel pairs) of nk slot vectors each, written by a kernel from a tensor where it lies: chunks of whole units in the values slot
// (workspace 9) -- at most cap_bytes of them, a single unit may take more --, a host tensor of src_words uploaded into the same slot, behind them.  The
// workspace holds a chunk and never the layer; opening the stage synchronises nothing.
struct ValueStage {
  i64 per = 0;                 // units per chunk
  i64* d_vals = nullptr;       // [per][unit_vals] in workspace slot 9, a host tensor behind them
  const i64* d_src = nullptr;  // the tensor in HBM
};
static int value_stage_open(fhesi_ctx* c, i64 nunits, size_t unit_vals, size_t cap_bytes, const int64_t* src, bool on_dev, size_t src_words, ValueStage* st) {
  st->per = std::max<i64>(1, std::min<i64>(nunits, (i64)(cap_bytes / (unit_vals * 8))));
  const size_t nvals = (size_t)st->per * unit_vals;
  FHESI_TRY(ws_i64(c, 9, (nvals + (on_dev ? 0 : src_words)) * 8, &st->d_vals));
  st->d_src = src;
  if (!on_dev) {
    HIP_TRY(hipMemcpyAsync(st->d_vals + nvals, src, src_words * 8, hipMemcpyHostToDevice, c->stream));
    st->d_src = st->d_vals + nvals;
  }
  return 0;
}
// the prepared plaintext of the layer, T rows per unit: write(first, nb) fills d_vals with the slot vectors of the units [first, first + nb), nb <= per, which
// are embedded and transformed into their rows chunk by chunk.  Synchronises (plain_rows_close): a host tensor is the caller's again on return.
template <class F> static int value_stage_plain(fhesi_slots* s, i64 nunits, i64 T, i64 per, const i64* d_vals, F write, fhesi_plain** made) {
  fhesi_ctx* c = s->ctx;
  i64* d_msg = nullptr;
  fhesi_plain* w = nullptr;
  int rc = msg_staging(c, per * T, &d_msg);
  if (!rc) rc = plain_alloc(c, nunits * T, s->S.p - 1, s->S.p, &w);      // the embedding leaves coefficients in [0, p)
  if (rc) { hipStreamSynchronize(c->stream); return rc; }
  for (i64 first = 0; first < nunits && !rc; first += per) {
    const i64 nb = std::min(per, nunits - first);
    rc = write(first, nb);
    if (!rc) rc = slots_embed_rows(s, d_vals, s->S.phim, false, nb * T, d_msg);
    if (!rc) rc = plain_rows_fill(c, w, first * T, d_msg, nb * T);
  }
  return plain_rows_close(c, w, rc, made);
}
// the same chunks downloaded instead: vals_host [nunits][unit_vals]
template <class F> static int value_stage_download(fhesi_ctx* c, i64 nunits, size_t unit_vals, i64 per, const i64* d_vals, F write, int64_t* vals_host) {
  for (i64 first = 0; first < nunits; first += per) {
    const i64 nb = std::min(per, nunits - first);
    FHESI_TRY(write(first, nb));
    HIP_TRY(hipMemcpyAsync(vals_host + (size_t)first * unit_vals, d_vals, (size_t)nb * unit_vals * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
constexpr size_t kLayerChunkBytes = (size_t)256 << 20;      // slot values of one chunk of units (a single unit may take more)

// A layer's entry E (LinearEntry, ConvEntry below) holds the space `s`, the shape, `what` -- the entry point, for its refusals -- and says
//   tensor, src_words(), bias_words(), cap_bytes()     what the tensor is called, its words and the bias's, the cap of a chunk
//   plan(h)                                             refuses the shape, or fills h's plan (GridLayer and the layer's own fields); launches nothing
//   bias_vals(h, d_b, d_bias)                           the nI bias rows from the bias in HBM
//   write(h, st, first, nb)                             the slot vectors of the units [first, first + nb) into st.d_vals
// The checks every entry starts with, once, and the ONE planner call: the shape, before anything is launched
template <class E> static int layer_plan(const E& e, const int64_t* src, typename E::Handle* h) {
  if (!e.s) FHESI_FAIL("%s: null plaintext space", e.what);
  CHECK_CTX(e.s->ctx);
  if (!src) FHESI_FAIL("%s: null %s", e.what, E::tensor);
  FHESI_TRY(e.plan(h));
  h->ctx = e.s->ctx; h->slots = e.s;
  return 0;
}
template <class E> static int layer_stage_open(const E& e, const typename E::Handle& h, const int64_t* src, bool on_dev, ValueStage* st) {
  return value_stage_open(h.ctx, (i64)h.nI * h.nJ, (size_t)h.nk * e.s->S.phim, e.cap_bytes(), src, on_dev, e.src_words(), st);
}
// The ONE constructor.  In order: the checks and the plan; the bias, allocated and written first -- a host bias goes through the values slot, which the stage
// takes over behind it --; the stage; the prepared plaintext (synchronises); the handle.  A failure behind the first launch synchronises before it returns
// and frees the bias.
template <class E, class H> static int layer_create(const E& e, const int64_t* src, const int64_t* bias, bool on_dev, H** out) {
  if (!out) FHESI_FAIL("%s: null output pointer", e.what);
  *out = nullptr;
  H h;
  FHESI_TRY(layer_plan(e, src, &h));
  fhesi_ctx* c = h.ctx;
  if (bias) {
    const size_t bytes = (size_t)h.nI * e.s->S.phim * 8;
    if (hipMalloc(&h.d_bias, bytes) != hipSuccess) { (void)hipGetLastError(); FHESI_FAIL("%s: hipMalloc of %zu bytes failed", e.what, bytes); }
    i64* d_b = const_cast<i64*>(bias);
    int rc = on_dev ? 0 : upload_vals(c, bias, e.bias_words() * 8, &d_b);
    if (!rc) rc = e.bias_vals(h, d_b, h.d_bias);
    if (rc) { hipStreamSynchronize(c->stream); hipFree(h.d_bias); return rc; }
  }
  ValueStage st;
  int rc = layer_stage_open(e, h, src, on_dev, &st);
  if (rc) hipStreamSynchronize(c->stream);
  else rc = value_stage_plain(e.s, (i64)h.nI * h.nJ, h.nk, st.per, st.d_vals, [&](i64 first, i64 nb) { return e.write(h, st, first, nb); }, &h.w);
  if (rc) { hipFree(h.d_bias); return rc; }
  *out = new H(h);
  return 0;
}
// the same stage without a handle: vals_host [nI][nJ][nk][phi(m)], chunk by chunk
template <class E> static int layer_download(const E& e, const int64_t* src_host, int64_t* vals_host) {
  if (!vals_host) FHESI_FAIL("%s: null output", e.what);
  typename E::Handle h;
  ValueStage st;
  FHESI_TRY(layer_plan(e, src_host, &h));
  FHESI_TRY(layer_stage_open(e, h, src_host, false, &st));
  return value_stage_download(h.ctx, (i64)h.nI * h.nJ, (size_t)h.nk * e.s->S.phim, st.per, st.d_vals, [&](i64 first, i64 nb) { return e.write(h, st, first, nb); }, vals_host);
}
template <class H> static int layer_free(H* h) {
  if (!h) return 0;
  fhesi_plain_free(h->w);      // (synchronises; the one live handle the layer counts as)
  hipFree(h->d_bias);
  delete h;
  return 0;
}
// what the info entries share
template <class T, class V> static void put(T* out, V v) { if (out) *out = (T)v; }
static int layer_info(const GridLayer& L, int32_t* has_bias, int64_t* amounts) {
  put(has_bias, L.d_bias ? 1 : 0);
  if (amounts) std::copy(L.amounts.begin(), L.amounts.end(), amounts);
  return 0;
}

// --------------------------------------------------------------------------------------------- dense linear layers
// The units are the nI nJ blocks, T prepared slot vectors w_t [T][phi(m)] each, written by linear_diag_kernel from the matrix where it is.  A layer is the
// grid of one block (Rb = R, Cb = C): everything here is written for the grid.
namespace {
struct LinearEntry {
  typedef fhesi_linear_grid Handle;
  static constexpr const char* tensor = "matrix";
  fhesi_slots* s;
  i64 R, C, Rb, Cb;
  int32_t baby;
  const char* what;
  size_t src_words() const { return (size_t)R * C; }
  size_t bias_words() const { return (size_t)R; }
  size_t cap_bytes() const { return kLayerChunkBytes; }
  int plan(Handle* lin) const {
    const i64 cols = s->S.phim / s->S.rows;
    int32_t nI = 0, nJ = 0, T = 0, B = 0, G = 0, nfold = 0;
    FHESI_TRY(linear_grid_plan(cols, R, C, Rb, Cb, baby, &nI, &nJ, &T, &B, &G, &nfold, &lin->amounts));
    lin->R = R; lin->C = C; lin->Rb = Rb; lin->Cb = Cb;
    lin->nI = nI; lin->nJ = nJ; lin->nk = T; lin->B = B; lin->G = G; lin->nfold = nfold;
    lin->terms = (i64)nJ * std::min(B, T);
    for (int t = 0; t < (int)lin->amounts.size(); ++t) lin->place.push_back(t + (t < B - 1 ? 1 : 2));      // the identity in front of the babies and of the giants
    return 0;
  }
  // b[I Rb + i mod Rb] in every row, I < nI: per output block the diagonal of the Rb x 1 block whose only column is its part of the bias -- a grid of nI x 1
  // such blocks with leading dimension 1
  int bias_vals(const Handle& lin, const i64* d_b, i64* d_bias) const { return launch_linear_diag(lin.ctx, s->S, d_b, 1, 1, 0, lin.nI, Rb, 1, 1, 1, d_bias); }
  int write(const Handle& lin, const ValueStage& st, i64 first, i64 nb) const {
    return launch_linear_diag(lin.ctx, s->S, st.d_src, C, lin.nJ, (int)first, (int)nb, Rb, Cb, lin.nk, lin.B, st.d_vals);
  }
};
}  // namespace
extern "C" int fhesi_linear_create(fhesi_slots* s, const int64_t* M_host, int64_t R, int64_t C, const int64_t* bias_host, int32_t baby, fhesi_linear** out) {
  return layer_create(LinearEntry{s, R, C, R, C, baby, "linear_create"}, M_host, bias_host, false, out);
}
extern "C" int fhesi_linear_create_dev(fhesi_slots* s, const int64_t* M_dev, int64_t R, int64_t C, const int64_t* bias_dev, int32_t baby, fhesi_linear** out) {
  return layer_create(LinearEntry{s, R, C, R, C, baby, "linear_create"}, M_dev, bias_dev, true, out);
}
extern "C" int fhesi_linear_free(fhesi_linear* lin) { return layer_free(lin); }
extern "C" int fhesi_linear_grid_info(const fhesi_linear_grid* lin, int64_t* R, int64_t* C, int64_t* Rb, int64_t* Cb, int32_t* nI, int32_t* nJ, int32_t* T, int32_t* B, int32_t* G,
                                      int32_t* nfold, int32_t* has_bias, int64_t* amounts) {
  if (!lin) FHESI_FAIL("null linear grid");
  put(R, lin->R); put(C, lin->C); put(Rb, lin->Rb); put(Cb, lin->Cb); put(nI, lin->nI); put(nJ, lin->nJ);
  put(T, lin->nk); put(B, lin->B); put(G, lin->G); put(nfold, lin->nfold);
  return layer_info(*lin, has_bias, amounts);
}
extern "C" int fhesi_linear_info(const fhesi_linear* lin, int64_t* R, int64_t* C, int32_t* T, int32_t* B, int32_t* G, int32_t* nfold, int32_t* has_bias, int64_t* amounts) {
  if (!lin) FHESI_FAIL("null linear layer");
  return fhesi_linear_grid_info(lin, R, C, nullptr, nullptr, nullptr, nullptr, T, B, G, nfold, has_bias, amounts);
}
extern "C" int fhesi_linear_diagonals(fhesi_slots* s, const int64_t* M_host, int64_t R, int64_t C, int32_t baby, int64_t* vals_host) {
  return layer_download(LinearEntry{s, R, C, R, C, baby, "linear_diagonals"}, M_host, vals_host);
}
extern "C" int fhesi_linear_grid_create(fhesi_slots* s, const int64_t* M_host, int64_t R, int64_t C, int64_t Rb, int64_t Cb, const int64_t* bias_host, int32_t baby,
                                        fhesi_linear_grid** out) {
  return layer_create(LinearEntry{s, R, C, Rb, Cb, baby, "linear_grid_create"}, M_host, bias_host, false, out);
}
extern "C" int fhesi_linear_grid_create_dev(fhesi_slots* s, const int64_t* M_dev, int64_t R, int64_t C, int64_t Rb, int64_t Cb, const int64_t* bias_dev, int32_t baby,
                                            fhesi_linear_grid** out) {
  return layer_create(LinearEntry{s, R, C, Rb, Cb, baby, "linear_grid_create"}, M_dev, bias_dev, true, out);
}
extern "C" int fhesi_linear_grid_free(fhesi_linear_grid* lin) { return layer_free(lin); }
extern "C" int fhesi_linear_grid_diagonals(fhesi_slots* s, const int64_t* M_host, int64_t R, int64_t C, int64_t Rb, int64_t Cb, int32_t baby, int64_t* vals_host) {
  return layer_download(LinearEntry{s, R, C, Rb, Cb, baby, "linear_grid_diagonals"}, M_host, vals_host);
}

// --------------------------------------------------------------------------------------------- convolution layers
// The plan and its refusals: conv_plan.h.  The units are the Cout Cin channel pairs, kh kw masked weight plaintexts [kh kw][phi(m)] each, written by
// conv_lattice_mask_kernel from the weight tensor where it is (option "stage_chunk_bytes" lowers the cap of a chunk, for tests).  The geometry -- step,
// stride, dilation -- is in the mask and in the bias; fhesi_conv2d_plan, _create[_dev] and _masks are the entries of the unit geometry, fhesi_conv2d_lattice_*
// take one, the handle records it, and the run call is fhesi_ct_conv2d_dev whatever it is.
static int conv_geom_plan(const char* what, const ConvShape& sh, const LatticeGeom& g, int32_t form, LatticeConvPlan* plan) {
  char why[256];
  if (lattice_refused(LatticeShape{sh, g}, form, why, sizeof why)) FHESI_FAIL("%s: %s", what, why);
  *plan = lattice_conv_plan(LatticeShape{sh, g}, form);
  return 0;
}
namespace {
struct ConvEntry {
  typedef fhesi_conv2d Handle;
  static constexpr const char* tensor = "kernel";
  fhesi_slots* s;
  i64 Cout, Cin, kh, kw, H, W, ah, aw;
  LatticeGeom g;
  int32_t form;
  const char* what;
  size_t src_words() const { return (size_t)(Cout * Cin * kh * kw); }
  size_t bias_words() const { return (size_t)Cout; }
  size_t cap_bytes() const { return s->ctx->opt.stage_chunk_bytes > 0 ? (size_t)s->ctx->opt.stage_chunk_bytes : kLayerChunkBytes; }
  int plan(Handle* cv) const {
    LatticeConvPlan lp;
    FHESI_TRY(conv_geom_plan(what, ConvShape{s->S.phim / s->S.rows, H, W, Cin, Cout, kh, kw, ah, aw}, g, form, &lp));
    cv->Cout = Cout; cv->Cin = Cin; cv->kh = kh; cv->kw = kw; cv->H = H; cv->W = W; cv->ah = ah; cv->aw = aw;
    cv->sy = g.sy; cv->sx = g.sx; cv->ty = g.ty; cv->tx = g.tx; cv->ey = g.ey; cv->ex = g.ex;
    cv->form = lp.p.form; cv->nh = lp.p.nh; cv->key_switches = lp.p.key_switches; cv->terms = lp.p.terms;
    cv->nI = (int)Cout; cv->nJ = (int)Cin; cv->nk = (int)(kh * kw);
    cv->flat = cv->form == 1; cv->anchored = true;
    cv->B = cv->flat ? cv->nk : (int)kw; cv->G = cv->flat ? 1 : (int)kh;
    cv->amounts.assign(lp.p.amounts.begin(), lp.p.amounts.end());
    for (int t = 0; t < cv->nh; ++t) cv->place.push_back(t);      // the babies, then the giants, the anchor among them
    return 0;
  }
  // b[I] on the output lattice, 0 off it: the plaintexts of the 1 x 1 kernel [Cout][1] whose only weight is the bias
  int bias_vals(const Handle& cv, const i64* d_b, i64* d_bias) const {
    return launch_conv_lattice_mask(cv.ctx, s->S, d_b, 0, (int)Cout, 1, 1, 0, 0, H, W, 1, 1, g.sy * g.ty, g.sx * g.tx, false, d_bias);
  }
  int write(const Handle& cv, const ValueStage& st, i64 first, i64 nb) const {
    return launch_conv_lattice_mask(cv.ctx, s->S, st.d_src, (int)first, (int)nb, (int)kh, (int)kw, (int)ah, (int)aw, H, W, g.ey * g.sy, g.ex * g.sx, g.sy * g.ty, g.sx * g.tx,
                                    cv.form == 2, st.d_vals);
  }
};
}  // namespace
extern "C" int fhesi_conv2d_lattice_plan(int64_t cols, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kh, int64_t kw, int64_t ah, int64_t aw, int64_t sy, int64_t sx,
                                         int64_t ty, int64_t tx, int64_t ey, int64_t ex, int32_t form, int32_t* form_out, int32_t* nh, int64_t* key_switches, int64_t* terms,
                                         int64_t* out_sy, int64_t* out_sx, int64_t* amounts) {
  LatticeConvPlan plan;
  FHESI_TRY(conv_geom_plan("conv2d_lattice_plan", ConvShape{cols, H, W, Cin, Cout, kh, kw, ah, aw}, LatticeGeom{sy, sx, ty, tx, ey, ex}, form, &plan));
  put(form_out, plan.p.form); put(nh, plan.p.nh); put(key_switches, plan.p.key_switches); put(terms, plan.p.terms); put(out_sy, plan.oy); put(out_sx, plan.ox);
  if (amounts) std::copy(plan.p.amounts.begin(), plan.p.amounts.end(), amounts);
  return 0;
}
extern "C" int fhesi_conv2d_plan(int64_t cols, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kh, int64_t kw, int64_t ah, int64_t aw, int32_t form, int32_t* form_out,
                                 int32_t* nh, int64_t* key_switches, int64_t* terms, int64_t* amounts) {
  LatticeConvPlan plan;
  FHESI_TRY(conv_geom_plan("conv2d_plan", ConvShape{cols, H, W, Cin, Cout, kh, kw, ah, aw}, LatticeGeom{}, form, &plan));
  put(form_out, plan.p.form); put(nh, plan.p.nh); put(key_switches, plan.p.key_switches); put(terms, plan.p.terms);
  if (amounts) std::copy(plan.p.amounts.begin(), plan.p.amounts.end(), amounts);
  return 0;
}
extern "C" int fhesi_conv2d_create(fhesi_slots* s, const int64_t* K_host, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                   const int64_t* bias_host, int32_t form, fhesi_conv2d** out) {
  return layer_create(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{}, form, "conv2d_create"}, K_host, bias_host, false, out);
}
extern "C" int fhesi_conv2d_create_dev(fhesi_slots* s, const int64_t* K_dev, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                       const int64_t* bias_dev, int32_t form, fhesi_conv2d** out) {
  return layer_create(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{}, form, "conv2d_create"}, K_dev, bias_dev, true, out);
}
extern "C" int fhesi_conv2d_lattice_create(fhesi_slots* s, const int64_t* K_host, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                           int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex, const int64_t* bias_host, int32_t form, fhesi_conv2d** out) {
  return layer_create(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{sy, sx, ty, tx, ey, ex}, form, "conv2d_lattice_create"}, K_host, bias_host, false, out);
}
extern "C" int fhesi_conv2d_lattice_create_dev(fhesi_slots* s, const int64_t* K_dev, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                               int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex, const int64_t* bias_dev, int32_t form, fhesi_conv2d** out) {
  return layer_create(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{sy, sx, ty, tx, ey, ex}, form, "conv2d_lattice_create"}, K_dev, bias_dev, true, out);
}
extern "C" int fhesi_conv2d_free(fhesi_conv2d* cv) { return layer_free(cv); }
extern "C" int fhesi_conv2d_info(const fhesi_conv2d* cv, int64_t* Cout, int64_t* Cin, int64_t* kh, int64_t* kw, int64_t* H, int64_t* W, int64_t* ah, int64_t* aw, int32_t* form,
                                 int32_t* nh, int64_t* key_switches, int64_t* terms, int32_t* has_bias, int64_t* amounts) {
  if (!cv) FHESI_FAIL("null convolution layer");
  put(Cout, cv->Cout); put(Cin, cv->Cin); put(kh, cv->kh); put(kw, cv->kw); put(H, cv->H); put(W, cv->W); put(ah, cv->ah); put(aw, cv->aw);
  put(form, cv->form); put(nh, cv->nh); put(key_switches, cv->key_switches); put(terms, cv->terms);
  return layer_info(*cv, has_bias, amounts);
}
extern "C" int fhesi_conv2d_lattice_info(const fhesi_conv2d* cv, int64_t* sy, int64_t* sx, int64_t* ty, int64_t* tx, int64_t* ey, int64_t* ex, int64_t* out_sy, int64_t* out_sx) {
  if (!cv) FHESI_FAIL("null convolution layer");
  put(sy, cv->sy); put(sx, cv->sx); put(ty, cv->ty); put(tx, cv->tx); put(ey, cv->ey); put(ex, cv->ex); put(out_sy, cv->sy * cv->ty); put(out_sx, cv->sx * cv->tx);
  return 0;
}
// vals_host [Cout][Cin][kh kw][phi(m)]
extern "C" int fhesi_conv2d_masks(fhesi_slots* s, const int64_t* K_host, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                  int32_t form, int64_t* vals_host) {
  return layer_download(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{}, form, "conv2d_masks"}, K_host, vals_host);
}
extern "C" int fhesi_conv2d_lattice_masks(fhesi_slots* s, const int64_t* K_host, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W, int64_t ah, int64_t aw,
                                          int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex, int32_t form, int64_t* vals_host) {
  return layer_download(ConvEntry{s, Cout, Cin, kh, kw, H, W, ah, aw, LatticeGeom{sy, sx, ty, tx, ey, ex}, form, "conv2d_lattice_masks"}, K_host, vals_host);
}

// --------------------------------------------------------------------------------------------- the dense bridge on a lattice of the plane
// M [R][nch Hl Wl] over logical pixels -> M' [R][nch H W] over the slots of the planes, zero columns off the lattice (lattice_columns_kernel): what
// fhesi_linear_grid_create[_dev] with Cb = H W takes as it is
static int lattice_columns_args(fhesi_slots* s, const char* what, const void* M, const void* out, i64 R, i64 nch, i64 H, i64 W, i64 sy, i64 sx) {
  if (!s) FHESI_FAIL("%s: null plaintext space", what);
  CHECK_CTX(s->ctx);
  if (!M || !out) FHESI_FAIL("%s: null argument", what);
  const long long cols = s->S.phim / s->S.rows;
  if (R < 1 || nch < 1 || H < 1 || W < 1 || sy < 1 || sx < 1)
    FHESI_FAIL("%s: %lld rows, %lld planes of %lld x %lld pixels, a step (%lld, %lld) (every size at least 1)", what, (long long)R, (long long)nch, (long long)H, (long long)W, (long long)sy, (long long)sx);
  if (H > cols || W > cols || H * W > cols || cols % (H * W)) FHESI_FAIL("%s: the plane of %lld x %lld pixels does not divide the row of %lld slots", what, (long long)H, (long long)W, cols);
  if (H % sy || W % sx) FHESI_FAIL("%s: the step (%lld, %lld) does not divide the %lld x %lld plane", what, (long long)sy, (long long)sx, (long long)H, (long long)W);
  if (nch > 65535 || R > ((i64)1 << 31) / (nch * H * W)) FHESI_FAIL("%s: %lld rows of %lld planes, at most 2^31 entries and 65535 planes are taken", what, (long long)R, (long long)nch);
  return 0;
}
extern "C" int fhesi_slots_lattice_columns_dev(fhesi_slots* s, const int64_t* M_dev, int64_t R, int64_t nch, int64_t H, int64_t W, int64_t sy, int64_t sx, int64_t* out_dev) {
  const char* what = "lattice_columns";
  FHESI_TRY(lattice_columns_args(s, what, M_dev, out_dev, R, nch, H, W, sy, sx));
  const size_t in_bytes = (size_t)R * nch * (H / sy) * (W / sx) * 8, out_bytes = (size_t)R * nch * H * W * 8;
  const uintptr_t a = (uintptr_t)M_dev, b = (uintptr_t)out_dev;
  if (a < b + out_bytes && b < a + in_bytes) FHESI_FAIL("%s: out overlaps the matrix", what);
  return launch_lattice_columns(s->ctx, M_dev, R, nch, H, W, sy, sx, out_dev);
}
extern "C" int fhesi_slots_lattice_columns(fhesi_slots* s, const int64_t* M_host, int64_t R, int64_t nch, int64_t H, int64_t W, int64_t sy, int64_t sx, int64_t* out_host) {
  const char* what = "lattice_columns";
  FHESI_TRY(lattice_columns_args(s, what, M_host, out_host, R, nch, H, W, sy, sx));
  fhesi_ctx* c = s->ctx;
  const size_t in_words = (size_t)R * nch * (H / sy) * (W / sx), out_words = (size_t)R * nch * H * W;
  i64* d_buf;      // the result, the uploaded matrix behind it (the values slot)
  FHESI_TRY(ws_i64(c, 9, (out_words + in_words) * 8, &d_buf));
  HIP_TRY(hipMemcpyAsync(d_buf + out_words, M_host, in_words * 8, hipMemcpyHostToDevice, c->stream));
  FHESI_TRY(launch_lattice_columns(c, d_buf + out_words, R, nch, H, W, sy, sx, d_buf));
  HIP_TRY(hipMemcpyAsync(out_host, d_buf, out_words * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// KeySwitchSI::Init (FHE-SI.cpp:153-209) for all columns of a matrix at once; the randomness is the caller's, in the reference's draw order
static int keyswitch_init_impl(fhesi_ksk* k, const fhesi_dcrt* const* src, int32_t nsrc, const fhesi_dcrt* dst_t, int32_t logQ, int32_t decomp_bytes,
                               const uint64_t* a_host, int32_t nlimbs, const int64_t* err_host, bool seeded, u64 seed, u64 pub_seed, u64 first) {
  if (!k) FHESI_FAIL("null key-switch matrix");
  fhesi_ctx* c = k->ctx;
  CHECK_CTX(c);
  if (nsrc != k->ncomp) FHESI_FAIL("KeySwitchSI::Init: the source key has %d components, the matrix was created for %d", nsrc, k->ncomp);
  if (decomp_bytes < 1 || decomp_bytes > 7) FHESI_FAIL("decompSize %d not supported", decomp_bytes);
  const int nd = (logQ + 8 * decomp_bytes - 1) / (8 * decomp_bytes);
  if (nd != k->ndigits) FHESI_FAIL("KeySwitchSI::Init: matrix has %d digits per component, context needs %d", k->ndigits, nd);
  if (nlimbs < 1 || nlimbs * 64 < logQ) FHESI_FAIL("KeySwitchSI::Init: random coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  const int L = c->L;
  if (!dst_t || dst_t->ctx != c || dst_t->coeff_form || (int)dst_t->idx.size() != L) FHESI_FAIL("KeySwitchSI::Init: the target key must be a DoubleCRT over all primes of this context");
  for (int i = 0; i < nsrc; ++i)
    if (!src[i] || src[i]->ctx != c || src[i]->coeff_form || (int)src[i]->idx.size() != L) FHESI_FAIL("KeySwitchSI::Init: source key component %d must be a DoubleCRT over all primes of this context", i);
  const i64 n = c->phim, ncol = (i64)nsrc * nd;
  const int nlq = (logQ + 63) / 64;
  const std::vector<int> all = full_set(c);
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  const int W = t->W;
  u64* d_b = k->d_rows;                                  // keySwitchMatrix[0] = b
  u64* d_A = k->d_rows + (size_t)ncol * L * n;           // keySwitchMatrix[1] = A
  // one-off call: its scratch is allocated here and released on return (the transforms below own the context's workspace slots)
  struct Scratch { std::vector<void*> p; ~Scratch() { hipDeviceSynchronize(); for (void* q : p) hipFree(q); } int get(size_t bytes, void** out) { if (hipMalloc(out, bytes ? bytes : 8) != hipSuccess) return 1; p.push_back(*out); return 0; } } scratch;
  void *d_s, *d_scoef, *d_in, *d_err, *d_bcoef, *d_comb;
  if (scratch.get((size_t)nsrc * L * n * 8, &d_s) || scratch.get((size_t)nsrc * n * W * 8, &d_scoef) || scratch.get((size_t)ncol * n * std::max(nlimbs, W) * 8, &d_in) ||
      scratch.get((size_t)ncol * n * 8, &d_err) || scratch.get((size_t)ncol * n * nlq * 8, &d_comb)) FHESI_FAIL("KeySwitchSI::Init: out of device memory");
  // sCoeff[i] = toPoly(s[i])   (:163-166)
  for (int i = 0; i < nsrc; ++i) HIP_TRY(hipMemcpyAsync((u64*)d_s + (size_t)i * L * n, src[i]->d_rows, (size_t)L * n * 8, hipMemcpyDeviceToDevice, c->stream));
  FHESI_TRY(row_inv(c, (u64*)d_s, nsrc, L, nullptr, all.data()));
  FHESI_TRY(launch_crt(c, t, (const u64*)d_s, L, nullptr, nsrc, 0, 0, 0, (u64*)d_scoef, W));
  // A[ind] = DoubleCRT(poly)   (:176-179)
  if (seeded) FHESI_TRY(launch_sample_keygen(c, (u64*)d_in, (i64*)d_err, ncol, nlimbs, logQ, seed, pub_seed, first));      // polynomials and errors drawn in HBM
  else {
    HIP_TRY(hipMemcpyAsync(d_in, a_host, (size_t)ncol * n * nlimbs * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_err, err_host, (size_t)ncol * n * 8, hipMemcpyHostToDevice, c->stream));
  }
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_in, nlimbs, n, ncol, 1, nullptr, d_A, L, nullptr));
  FHESI_TRY(row_fwd(c, d_A, ncol, L, nullptr, all.data()));
  // b[ind] = A[ind] * t; toPoly   (:180-187)
  FHESI_TRY(launch_rows_mul_bcast(c, d_b, d_A, dst_t->d_rows, ncol));
  FHESI_TRY(row_inv(c, d_b, ncol, L, nullptr, all.data()));
  d_bcoef = d_in;                                        // (the random coefficients are consumed)
  FHESI_TRY(launch_crt(c, t, d_b, L, nullptr, ncol, 0, 0, 0, (u64*)d_bcoef, W));
  // bCoeff += err + sCoeff[i] << (8 decompSize j); ReduceCoefficients; b[ind] = DoubleCRT(bCoeff)   (:189-204)
  FHESI_TRY(launch_keygen_combine(c, (const u64*)d_bcoef, W, (const u64*)d_scoef, W, (const i64*)d_err, ncol, nd, 8 * decomp_bytes, nlq, logQ, (u64*)d_comb));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_comb, nlq, n, ncol, 1, nullptr, d_b, L, nullptr));
  FHESI_TRY(row_fwd(c, d_b, ncol, L, nullptr, all.data()));
  // A[ind] *= -1   (:181)
  FHESI_TRY(fhesi_rows_mul_long_dev(c, d_A, -1, ncol));
  k->aux_valid = false;
  HIP_TRY(hipStreamSynchronize(c->stream));             // the host arrays and the scratch may be released on return
  return 0;
}
extern "C" int fhesi_keyswitch_init_batch(fhesi_ksk* k, const fhesi_dcrt* const* src, int32_t nsrc, const fhesi_dcrt* dst_t, int32_t logQ, int32_t decomp_bytes,
                                          const uint64_t* a_host, int32_t nlimbs, const int64_t* err_host) {
  if (!a_host || !err_host) FHESI_FAIL("KeySwitchSI::Init: null randomness (fhesi_keyswitch_init_batch_seeded draws it on the device)");
  return keyswitch_init_impl(k, src, nsrc, dst_t, logQ, decomp_bytes, a_host, nlimbs, err_host, false, 0, 0, 0);
}
// ... with the column randomness drawn on the device: column i takes the streams of object index first_index + i (philox.h); the public
// polynomials a draw from public_seed, the secret errors from seed
extern "C" int fhesi_keyswitch_init_batch_seeded(fhesi_ksk* k, const fhesi_dcrt* const* src, int32_t nsrc, const fhesi_dcrt* dst_t, int32_t logQ, int32_t decomp_bytes,
                                                 uint64_t seed, uint64_t public_seed, uint64_t first_index) {
  if (public_seed == seed) FHESI_FAIL("KeySwitchSI::Init (seeded): public_seed must differ from the secret seed (the polynomials a are public, the errors are not)");
  return keyswitch_init_impl(k, src, nsrc, dst_t, logQ, decomp_bytes, nullptr, (logQ + 63) / 64, nullptr, true, seed, public_seed, first_index);
}
// DoubleCRT::sampleHWt / sampleGaussian (DoubleCRT.h; NumbTh.cpp:340-404) with the polynomial drawn on the device: kind 0 = Hamming weight
// `param` with +-1 entries (the secret key, FHE-SI.cpp:90), kind 1 = rounded Gaussian with the context's stdev 3.2 (FHEContext.h:106)
extern "C" int fhesi_dcrt_sample(fhesi_dcrt* d, int32_t kind, int64_t param, uint64_t seed, uint64_t index) {
  if (!d) FHESI_FAIL("null DoubleCRT");
  fhesi_ctx* c = d->ctx;
  CHECK_CTX(c);
  if (d->coeff_form) FHESI_FAIL("sample: the object is a SingleCRT");
  if (kind == 0 && param < 0) FHESI_FAIL("sampleHWt: negative weight");
  const i64 n = c->phim;
  const int K = (int)d->idx.size();
  void* d_poly;
  FHESI_TRY(ws_reserve(c, 9, (size_t)n * 8, &d_poly));
  FHESI_TRY(launch_sample_poly(c, (i64*)d_poly, kind, param, seed, index));
  int* d_pos = nullptr;
  FHESI_TRY(upload_idx(c, d->idx, &d_pos));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)d_poly, 1, n, 1, 1, nullptr, d->d_rows, K, d_pos));
  FHESI_TRY(row_fwd(c, d->d_rows, 1, K, d_pos, d->idx.data()));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

