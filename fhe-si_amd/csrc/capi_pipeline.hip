// capi_pipeline.hip -- the key-switch matrix and the fused ciphertext multiplication + key switch, per stage and per batch (include/fhesi_hip.h)
#include "capi_common.h"
#include "copy_pool.h"
#include "wave_plan.h"
#include "poly_plan.h"
#include "conv_plan.h"
#include "lattice_plan.h"

// --------------------------------------------------------------------------------------------- key-switch matrix
extern "C" int fhesi_ksk_create(fhesi_ctx* c, int32_t ncomp, int32_t ndigits, fhesi_ksk** out) {
  CHECK_CTX(c);
  if (ncomp < 1 || ndigits < 1) FHESI_FAIL("KeySwitchSI: bad shape");
  fhesi_ksk* k = new fhesi_ksk();
  k->ctx = c; k->ncomp = ncomp; k->ndigits = ndigits;
  k->bytes = (size_t)2 * ncomp * ndigits * c->L * c->phim * 8;
  HIP_TRY(hipMalloc(&k->d_rows, k->bytes));
  HIP_TRY(hipMemsetAsync(k->d_rows, 0, k->bytes, c->stream));
  ++c->live_handles;
  *out = k;
  return 0;
}
extern "C" int fhesi_ksk_free(fhesi_ksk* k) {
  if (!k) return 0;
  hipSetDevice(k->ctx->device);
  hipStreamSynchronize(k->ctx->stream);
  hipFree(k->d_rows);
  if (k->d_aux) hipFree(k->d_aux);
  if (k->d_aux_consts) hipFree(k->d_aux_consts);
  if (k->d_limb_consts) hipFree(k->d_limb_consts);
  --k->ctx->live_handles;
  delete k;
  return 0;
}
extern "C" int fhesi_ksk_upload(fhesi_ksk* k, const uint64_t* rows_host) {
  if (!k) FHESI_FAIL("null key-switch matrix");
  CHECK_CTX(k->ctx);
  HIP_TRY(hipMemcpyAsync(k->d_rows, rows_host, k->bytes, hipMemcpyHostToDevice, k->ctx->stream));
  HIP_TRY(hipStreamSynchronize(k->ctx->stream));
  k->aux_valid = false;
  return 0;
}
// The library keeps tables derived from the rows; whoever writes the rows directly (a collective receiving into them) says so with
// fhesi_ksk_mark_dirty, and the next key switch rebuilds the tables.  The getter itself has no side effect.
extern "C" void* fhesi_ksk_device_ptr(fhesi_ksk* k) { return k ? k->d_rows : nullptr; }
extern "C" int fhesi_ksk_download(const fhesi_ksk* k, uint64_t* rows_host) {
  if (!k || !rows_host) FHESI_FAIL("null key-switch matrix");
  CHECK_CTX(k->ctx);
  HIP_TRY(hipMemcpyAsync(rows_host, k->d_rows, k->bytes, hipMemcpyDeviceToHost, k->ctx->stream));
  HIP_TRY(hipStreamSynchronize(k->ctx->stream));
  return 0;
}
extern "C" int fhesi_ksk_mark_dirty(fhesi_ksk* k) {
  if (!k) FHESI_FAIL("null key-switch matrix");
  k->aux_valid = false;
  return 0;
}
extern "C" int fhesi_ksk_upload_dev(fhesi_ksk* k, const uint64_t* rows_dev) {
  if (!k || !rows_dev) FHESI_FAIL("null key-switch matrix");
  CHECK_CTX(k->ctx);
  HIP_TRY(hipMemcpyAsync(k->d_rows, rows_dev, k->bytes, hipMemcpyDeviceToDevice, k->ctx->stream));
  HIP_TRY(hipStreamSynchronize(k->ctx->stream));
  k->aux_valid = false;
  return 0;
}
extern "C" size_t fhesi_ksk_bytes(const fhesi_ksk* k) { return k ? k->bytes : 0; }
extern "C" int fhesi_ksk_form(const fhesi_ksk* k, int32_t* form, int32_t* rows, int32_t* limb_bits) {
  if (!k) FHESI_FAIL("null key-switch matrix");
  if (form) *form = k->last_form;
  if (rows) *rows = k->last_form > 0 ? k->aux_rows : (k->last_form == 0 ? k->ctx->L : 0);
  if (limb_bits) *limb_bits = k->last_form > 0 ? k->aux_limb_bits : 0;
  return 0;
}

extern "C" int fhesi_ksk_key_bits(const fhesi_ksk* k, int32_t* centred, int32_t* key_bits) {
  if (!k) FHESI_FAIL("null key-switch matrix");
  if (centred) *centred = k->aux_valid && k->aux_centred ? 1 : 0;
  if (key_bits) *key_bits = k->aux_valid ? k->aux_key_bits : 0;
  return 0;
}

// --------------------------------------------------------------------------------------------- ciphertext pipeline
static i64 batch_chunk(fhesi_ctx* c, int ncol, bool ks32, i64 count = -1);
static int mul_relin_chunks(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* a, const uint64_t* b, uint64_t* out, int32_t nlimbs, int64_t count);

extern "C" int fhesi_ct_mul_dev(fhesi_ctx* c, uint64_t p, const uint64_t* a, const uint64_t* b, int32_t nlimbs, int64_t count, uint64_t* tprod) {
  CHECK_CTX(c);
  if (!count) return 0;
  const i64 n = c->phim;
  const int L = c->L;
  const std::vector<int> all = full_set(c);
  // c1[i] = DoubleCRT(parts[i].poly * p), c2[j] = DoubleCRT(other.parts[j].poly)   (Ciphertext.cpp:169-176)
  void* d_c;
  FHESI_TRY(ws_reserve(c, 0, (size_t)count * 4 * L * n * 8, &d_c));
  u64* ca = (u64*)d_c;
  u64* cb = ca + (size_t)count * 2 * L * n;
  const u64 lift[2] = {p, p};
  FHESI_TRY(launch_rns_reduce(c, (const u64*)a, nlimbs, n, count, 2, lift, ca, L, nullptr));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)b, nlimbs, n, count, 2, nullptr, cb, L, nullptr));
  FHESI_TRY(row_fwd(c, ca, count * 4, L, nullptr, all.data()));
  // tProd[i+j] += c1[i] * c2[j]   (Ciphertext.cpp:179-186)
  FHESI_TRY(launch_tensor2x2(c, ca, cb, (u64*)tprod, count));
  return 0;
}

// ByteDecomp + DoubleCRT(digit polys) + DotProduct + toPoly + ReduceCoefficients (FHE-SI.cpp:244-256) from parts that are already
// positive residues mod 2^logQ in limb-major layout [count*ncomp][nlq][n], in two halves: key_switch_digits leaves the digit rows in the
// running form's layout (workspace slot 0) and reads no matrix; key_switch_finish is everything that does -- dot product, inverse rows and
// recombination / CRT.  key_switch_tail runs one after the other; the hoisted rotations (below) run the first once and the second per matrix.
// The form that runs for this matrix, with its auxiliary table built (ksaux_build borrows workspace slot 0: before any digit rows exist).
static int key_switch_form(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, int* ks_mode_out) {
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t));
  // Dot product through the two largest chain primes (kernels_ksaux.hip): 2 transforms per digit polynomial instead of L.
  // option ks_direct keeps the per-prime dot product below (A/B measurements; also the path of every shape the other does not cover).
  const int ks_mode = ksaux_mode(c, t, k->ncomp * k->ndigits, 8 * decomp_bytes, logQ);
  fhesi_ksk* km = const_cast<fhesi_ksk*>(k);
  km->last_form = ks_mode;
  if (ks_mode != KS_MODE_DIRECT && (!k->aux_valid || k->aux_mode != ks_mode || k->aux_suborder != ntt_digits_suborder(c, 8 * decomp_bytes) || k->aux_logQ != logQ || k->aux_long_opt != c->opt.ks_long_keys))
    FHESI_TRY(ksaux_build(c, km, 8 * decomp_bytes, logQ, ks_mode));
  *ks_mode_out = ks_mode;
  return 0;
}
// parts_wm: d_parts are 32-bit word rows (launch_tensor32 parts_wm) -- only the four-prime limb form reads those; the caller asks for them
// only when ksaux_mode says that form runs.
static int key_switch_digits(fhesi_ctx* c, int ks_mode, int ncomp, int nd, int32_t logQ, int32_t decomp_bytes, const u64* d_parts, int64_t count, bool parts_wm, void** d_dig_out) {
  const i64 n = c->phim;
  const int L = c->L, ncol = ncomp * nd, nlq = (logQ + 63) / 64;
  if (parts_wm && ks_mode != KS_MODE_LIMB32) FHESI_FAIL("key switch: word-major parts handed to a form that reads limb rows (internal)");
  void* d_dig;
  if (ks_mode == KS_MODE_LIMB32) {       // four 30-bit primes (kernels_aux32.hip): the buffer of the 60-bit forms, u32 rows (always 2^14 or 2^15 elements: four 4-byte residues = two 8-byte ones)
    FHESI_TRY(ws_reserve(c, 0, (size_t)count * ncol * 2 * aux32_row_len(c) * 8, &d_dig));
    FHESI_TRY(launch_ntt32_fwd_digits(c, d_parts, nlq, 8 * decomp_bytes, nd, count * ncomp, (u32*)d_dig, kDigitSubCt * ncol, parts_wm));
  } else if (ks_mode != KS_MODE_DIRECT) {
    FHESI_TRY(ws_reserve(c, 0, (size_t)count * ncol * 2 * n * 8, &d_dig));
    FHESI_TRY(launch_ntt_fwd_digits(c, d_parts, nlq, logQ, 8 * decomp_bytes, nd, count * ncomp, (u64*)d_dig, 0, 2, 2));
  } else {
    // ByteDecomp + DoubleCRT(digit polys)   (Ciphertext.cpp:82-121, FHE-SI.cpp:244-249)
    FHESI_TRY(ws_reserve(c, 0, (size_t)count * ncol * L * n * 8, &d_dig));
    if (c->pow2) FHESI_TRY(launch_ntt_fwd_digits(c, d_parts, nlq, logQ, 8 * decomp_bytes, nd, count * ncomp, (u64*)d_dig));
    else {
      FHESI_TRY(launch_digits(c, d_parts, nlq, logQ, 8 * decomp_bytes, nd, count * ncomp, (u64*)d_dig));
      const std::vector<int> all = full_set(c);
      FHESI_TRY(row_fwd(c, (u64*)d_dig, count * ncol, L, nullptr, all.data()));
    }
  }
  if (c->mark_mid) { HIP_TRY(hipEventRecord(c->ev_mid, c->stream)); c->mark_mid = false; }
  *d_dig_out = d_dig;
  return 0;
}
// the four-prime form behind its dot product: d_o [count*2*R][4][row] -> inverse rows -> recombination
static int key_switch_close32(fhesi_ctx* c, const CrtTables* t, const fhesi_ksk* k, u32* d_o, int64_t count, bool mont, uint64_t* out, int32_t nlimbs) {
  const bool fold_tail = ks_recombine_takes_tail(c, t, k);      // (rows of 2^15 at the stress chain: the inverse's tail stage runs in the recombination's loader)
  FHESI_TRY(launch_ntt32_inv(c, d_o, count * 2 * k->aux_rows, 4, 0, mont, !fold_tail));
  return launch_ks_recombine(c, t, k, (const u64*)d_o, count * 2, (u64*)out, nlimbs, fold_tail);
}
// The per-prime and the residue forms need scratch for count*2 DoubleCRTs: workspace slot 1, reserved here (the limb forms never touch it).  Whatever a
// caller kept in slot 1 -- the scaled-up tProd, the automorphism's rows -- is dead by then: it was read into the parts in front of the digit rows.
// apply_key_switch_consume sizes slot 1 for max(ncomp, 2) parts, so the later reservation never regrows it.
static int key_switch_finish(fhesi_ctx* c, const fhesi_ksk* k, int ks_mode, int32_t logQ, int32_t decomp_bytes, const void* d_dig, int64_t count, uint64_t* out, int32_t nlimbs) {
  const i64 n = c->phim;
  const int L = c->L, ncol = k->ncomp * k->ndigits;
  const std::vector<int> all = full_set(c);
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  void *d_o = nullptr, *d_t;
  if (ks_mode != KS_MODE_DIRECT) {
    fhesi_ksk* km = const_cast<fhesi_ksk*>(k);
    const int R = k->aux_rows;        // L chain-prime residues, or the limbs of the key's integer coefficients (limb mode)
    const i64 nrow = k->aux32 ? aux32_row_len(c) : n;      // the 32-bit auxiliary rows always have 2^14 or 2^15 elements
    if (k->aux32 != (ks_mode == KS_MODE_LIMB32)) FHESI_FAIL("key switch: the matrix's table does not match the running form (internal)");
    FHESI_TRY(ws_reserve(c, 10, (size_t)count * 2 * R * 2 * nrow * 8, &d_o));
    if (k->aux32) {
      bool mont = true;                 // dot32_kernel2 leaves the factor 2^-32 of its Montgomery step; the matrix-core form does not
      FHESI_TRY(launch_dot32(c, km, (const u32*)d_dig, ncol, count, (u32*)d_o, &mont));
      return key_switch_close32(c, t, k, (u32*)d_o, count, mont, out, nlimbs);
    }
    FHESI_TRY(launch_dot_aux(c, k, (const u64*)d_dig, ncol, count, (u64*)d_o));
    FHESI_TRY(launch_ntt_inv(c, (u64*)d_o, count * 2 * R, 2, (const int*)(k->d_aux_consts + L), !k->aux_suborder));
    if (k->aux_limb_bits) return launch_ks_recombine(c, t, k, (const u64*)d_o, count * 2, (u64*)out, nlimbs);
  }
  FHESI_TRY(ws_reserve(c, 1, (size_t)count * 2 * L * n * 8, &d_t));
  if (ks_mode != KS_MODE_DIRECT) FHESI_TRY(launch_aux_crt(c, k, (const u64*)d_o, (u64*)d_t, count * 2 * L));
  else {
    // DotProduct with both key rows (FHE-SI.cpp:251-254), toPoly
    FHESI_TRY(launch_dot_accum(c, k->d_rows, (const u64*)d_dig, ncol, count, (u64*)d_t, 0, 0, c->pow2 && ntt_digits_suborder(c, 8 * decomp_bytes)));
    FHESI_TRY(row_inv(c, (u64*)d_t, count * 2, L, nullptr, all.data()));
  }
  // ReduceCoefficients (FHE-SI.cpp:255-256)
  return launch_crt(c, t, (const u64*)d_t, L, nullptr, count * 2, 2, 0, logQ, (u64*)out, nlimbs);
}
static int key_switch_tail(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, const u64* d_parts, int64_t count, uint64_t* out, int32_t nlimbs, bool parts_wm = false) {
  int ks_mode;
  FHESI_TRY(key_switch_form(c, k, logQ, decomp_bytes, &ks_mode));
  void* d_dig;
  FHESI_TRY(key_switch_digits(c, ks_mode, k->ncomp, k->ndigits, logQ, decomp_bytes, d_parts, count, parts_wm, &d_dig));
  return key_switch_finish(c, k, ks_mode, logQ, decomp_bytes, d_dig, count, out, nlimbs);
}

static int key_switch_args(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, int32_t nlimbs) {
  if (!k || k->ctx != c) FHESI_FAIL("KeySwitchSI: context mismatch");            // FHE-SI.cpp:279-281
  if (decomp_bytes < 1 || decomp_bytes > 7) FHESI_FAIL("decompSize %d not supported", decomp_bytes);
  const int nd = (logQ + 8 * decomp_bytes - 1) / (8 * decomp_bytes);            // FHEContext.h:115
  if (nd != k->ndigits) FHESI_FAIL("KeySwitchSI: matrix has %d digits per component, context needs %d", k->ndigits, nd);
  if (nlimbs * 64 < logQ) FHESI_FAIL("output coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  return 0;
}

// d_t: the scaled-up ciphertexts [count][ncomp][L][n] in workspace slot 1, with room for max(ncomp, 2) parts per ciphertext; consumed (transformed
// in place; key_switch_finish then takes the slot for the dot product's rows)
static int apply_key_switch_consume(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, u64* d_t, int64_t count, uint64_t* out, int32_t nlimbs) {
  const i64 n = c->phim;
  const int L = c->L, ncomp = k->ncomp, nlq = (logQ + 63) / 64;
  const std::vector<int> all = full_set(c);
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, all, &t));
  // ScaleDown (Ciphertext.cpp:194-218): toPoly + round(x/q) + Reduce, kept as positive residues for ByteDecomp
  FHESI_TRY(row_inv(c, d_t, count * ncomp, L, nullptr, all.data()));
  void* d_parts;
  FHESI_TRY(ws_reserve(c, 2, (size_t)count * ncomp * nlq * n * 8, &d_parts));
  FHESI_TRY(launch_crt(c, t, (const u64*)d_t, L, nullptr, count * ncomp, 1, 0, logQ, (u64*)d_parts, nlq));
  return key_switch_tail(c, k, logQ, decomp_bytes, (const u64*)d_parts, count, out, nlimbs);
}

extern "C" int fhesi_apply_key_switch_dev(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, const uint64_t* tprod, int64_t count,
                                          uint64_t* out, int32_t nlimbs) {
  CHECK_CTX(c);
  FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
  if (!count) return 0;
  const i64 n = c->phim;
  const int L = c->L, ncomp = k->ncomp;
  void* d_t;
  FHESI_TRY(ws_reserve(c, 1, (size_t)count * (ncomp > 2 ? ncomp : 2) * L * n * 8, &d_t));
  HIP_TRY(hipMemcpyAsync(d_t, tprod, (size_t)count * ncomp * L * n * 8, hipMemcpyDeviceToDevice, c->stream));      // the caller keeps its tProd
  return apply_key_switch_consume(c, k, logQ, decomp_bytes, (u64*)d_t, count, out, nlimbs);
}

// Ciphertext::operator>>= (Ciphertext.cpp:264-269 -> CiphertextPart::operator>>= :54-59: DoubleCRT(poly) >>= k; toPoly) for a batch
// of unscaled ciphertexts, rows left in d_rows [count*nparts][L][n] in coefficient (post-iFFT) form ready for the CRT.
static int automorph_rows(fhesi_ctx* c, int64_t kk, const uint64_t* in, int32_t nparts, int32_t nlimbs_in, int64_t count, u64** d_rows_out) {
  const i64 n = c->phim;
  if (!in_zm_star(c, kk)) FHESI_FAIL("automorph: k=%lld is not in Zm*", (long long)kk);
  const int L = c->L;
  const std::vector<int> all = full_set(c);
  const i64 nrows = count * nparts * L;
  void *d_a, *d_b;
  FHESI_TRY(ws_reserve(c, 3, (size_t)nrows * n * 8, &d_a));
  FHESI_TRY(ws_reserve(c, 1, (size_t)(nrows > count * 2 * L ? nrows : count * 2 * L) * n * 8, &d_b));
  FHESI_TRY(launch_rns_reduce(c, (const u64*)in, nlimbs_in, n, count, nparts, nullptr, (u64*)d_a, L, nullptr));
  FHESI_TRY(row_fwd(c, (u64*)d_a, count * nparts, L, nullptr, all.data()));
  FHESI_TRY(launch_automorph(c, (u64*)d_b, (const u64*)d_a, nrows, kk));
  FHESI_TRY(row_inv(c, (u64*)d_b, count * nparts, L, nullptr, all.data()));
  *d_rows_out = (u64*)d_b;
  return 0;
}
// The front half of a key switch of unscaled ciphertexts: sigma_kk of the count * nparts polynomials at src as positive residues mod 2^logQ, limb-major
// (what ByteDecomp reads), in workspace slot 2.  On power-of-two, prime-power and 2 x prime-power rings a(X^k) mod Phi_m is a signed gather of the
// coefficients, no row transform (kernels_ct.hip); on the others, and under option automorph_rows, the evaluation rows: toPoly (centred modulo the
// whole chain), then Reduce(..., positive) of ByteDecompPart (Ciphertext.cpp:94).  kk must be in Zm*.
static int unscaled_parts(fhesi_ctx* c, int64_t kk, const u64* src, int32_t nparts, int32_t nlimbs_in, int64_t count, int32_t logQ, u64** d_parts_out) {
  const int nlq = (logQ + 63) / 64;
  void* d_parts;
  FHESI_TRY(ws_reserve(c, 2, (size_t)count * nparts * nlq * c->phim * 8, &d_parts));
  *d_parts_out = (u64*)d_parts;
  const int r = c->opt.automorph_rows ? 2 : launch_ct_automorph_parts(c, src, nlimbs_in, count * nparts, kk, logQ, (u64*)d_parts, nlq);
  if (r != 2) return r;
  u64* d_rows;
  FHESI_TRY(automorph_rows(c, kk, src, nparts, nlimbs_in, count, &d_rows));
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t));
  return launch_crt(c, t, d_rows, c->L, nullptr, count * nparts, 3, 0, logQ, (u64*)d_parts, nlq);
}
// ... of two-part ciphertexts as they are (k = 1), on to the digit rows of the running form (slot 0): what a hoisted matrix is applied to
static int unscaled_digits(fhesi_ctx* c, int ks_mode, int nd, int32_t logQ, int32_t decomp_bytes, const u64* src, int32_t nlimbs_in, int64_t count, void** d_dig) {
  u64* d_parts;
  FHESI_TRY(unscaled_parts(c, 1, src, 2, nlimbs_in, count, logQ, &d_parts));
  return key_switch_digits(c, ks_mode, 2, nd, logQ, decomp_bytes, d_parts, count, false, d_dig);
}

extern "C" int fhesi_ct_automorph_dev(fhesi_ctx* c, int64_t kk, const uint64_t* in, int32_t nparts, int32_t nlimbs_in, int64_t count, uint64_t* out,
                                      int32_t nlimbs_out) {
  CHECK_CTX(c);
  if (nparts < 1 || nlimbs_in < 1 || nlimbs_out < 1) FHESI_FAIL("Ciphertext >>= : bad shape");
  if (!count) return 0;
  if (!in_zm_star(c, kk)) FHESI_FAIL("automorph: k=%lld is not in Zm*", (long long)kk);
  // the coefficient gather gives the integers a(X^k) mod Phi_m themselves; the reference's toPoly centres modulo the chain product: the
  // same thing as long as the sum of two input coefficients (64 nlimbs_in + 1 bits) stays below half of it
  if (!c->opt.automorph_rows && 64.0 * nlimbs_in + 2 < chain_bits(c)) {        // (fewer output limbs truncate the two's complement value in both forms)
    const int r = launch_ct_automorph_parts(c, (const u64*)in, nlimbs_in, count * nparts, kk, 0, (u64*)out, nlimbs_out);
    if (r != 2) return r;
  }
  u64* d_rows;
  FHESI_TRY(automorph_rows(c, kk, in, nparts, nlimbs_in, count, &d_rows));
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t));
  return launch_crt(c, t, d_rows, c->L, nullptr, count * nparts, 0, 0, 0, (u64*)out, nlimbs_out);
}

extern "C" int fhesi_ct_automorph_key_switch_dev(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes, int64_t kk, const uint64_t* in,
                                                 int32_t nlimbs_in, int64_t count, uint64_t* out, int32_t nlimbs) {
  CHECK_CTX(c);
  FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
  if (nlimbs_in < 1) FHESI_FAIL("Ciphertext >>= : bad shape");
  if (!count) return 0;
  if (!in_zm_star(c, kk)) FHESI_FAIL("automorph: k=%lld is not in Zm*", (long long)kk);
  u64* d_parts;      // (k = 1, no automorphism: ApplyKeySwitch on the unscaled ciphertext as it is)
  FHESI_TRY(unscaled_parts(c, kk, (const u64*)in, k->ncomp, nlimbs_in, count, logQ, &d_parts));
  return key_switch_tail(c, k, logQ, decomp_bytes, d_parts, count, out, nlimbs);
}

// --------------------------------------------------------------------------------------------- hoisted rotations
// sigma_k is a ring map, so  sum_j sigma_k(D_j(c)) W_k[j] = sigma_k( sum_j D_j(c) W'_k[j] )  with W'_k = sigma_k^-1(W_k), every column, both rows
// (DESIGN.md 9a): the digits of the UNTOUCHED ciphertext are decomposed and transformed once and serve every rotation; a rotation is one dot
// product with its derived matrix, one inverse, one recombination and the signed gather of two polynomials.
extern "C" int fhesi_ksk_hoist(const fhesi_ksk* k, int64_t kk, fhesi_ksk** out) {
  if (!k || !out) FHESI_FAIL("ksk_hoist: null argument");
  fhesi_ctx* c = k->ctx;
  CHECK_CTX(c);
  *out = nullptr;
  if (k->ncomp != 2) FHESI_FAIL("ksk_hoist: the matrix has %d source components, a rotation matrix (source key (1, s(X^k))) has 2", k->ncomp);
  if (!in_zm_star(c, kk)) FHESI_FAIL("ksk_hoist: k=%lld is not in Zm*", (long long)kk);
  fhesi_ksk* h;
  FHESI_TRY(fhesi_ksk_create(c, k->ncomp, k->ndigits, &h));
  // DoubleCRT::automorph by k^-1 on every evaluation row [2][ncol][L][phi(m)]: the same gather on every ring and for every prime
  const i64 nrows = (i64)2 * k->ncomp * k->ndigits * c->L, kinv = hm::inv_mod(kk, c->m), step = 32768;      // (k in Z_m^*: checked above)
  int rc = 0;
  for (i64 r0 = 0; r0 < nrows && !rc; r0 += step) rc = launch_automorph(c, h->d_rows + r0 * c->phim, k->d_rows + r0 * c->phim, std::min(step, nrows - r0), kinv);
  if (rc) { fhesi_ksk_free(h); return rc; }
  h->hoist_k = kk;
  *out = h;
  return 0;
}

// reduce_logq(Ciphertext >>= k) of count unscaled two-part ciphertexts: the signed gather where the ring has one (any input size: the gather's
// two's complement sum is exact modulo 2^(64 nlimbs), a multiple of 2^logQ), the evaluation rows otherwise; k = 1 is the reduced copy
static int rotation_close(fhesi_ctx* c, int64_t kk, int32_t logQ, const u64* src, int32_t nl_src, int64_t count, u64* out, int32_t nlimbs) {
  if (!c->opt.automorph_rows) {
    const int r = launch_ct_automorph_parts(c, src, nl_src, count * 2, kk, 0, out, nlimbs);
    if (r == 1) return 1;
    if (r == 0) return launch_ct_mul_long(c, out, count * 2 * c->phim, nlimbs, logQ, 1);      // (times one: the centred residue modulo 2^logQ, in place)
  }
  u64* d_rows;
  FHESI_TRY(automorph_rows(c, kk, src, 2, nl_src, count, &d_rows));
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t));
  return launch_crt(c, t, d_rows, c->L, nullptr, count * 2, 2, 0, logQ, out, nlimbs);
}
static int rotations_args(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes, int32_t nlimbs_in, int64_t count, int32_t nlimbs) {
  if (nk < 0 || count < 0) FHESI_FAIL("ct_rotations: negative count");
  if (nk && (!hoisted || !ks)) FHESI_FAIL("ct_rotations: null argument");
  if (nlimbs_in < 1) FHESI_FAIL("ct_rotations: bad shape (%d input limbs)", nlimbs_in);
  if (logQ < 1 || nlimbs < 1 || nlimbs * 64 < logQ) FHESI_FAIL("ct_rotations: output coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  if (nlimbs > 32) FHESI_FAIL("ct_rotations: ciphertext coefficients of %d limbs exceed the supported 32", nlimbs);
  for (int t = 0; t < nk; ++t) {
    const fhesi_ksk* k = hoisted[t];
    if (!k) {
      if (ks[t] != 1) FHESI_FAIL("ct_rotations: rotation %d has no matrix and k=%lld (only k = 1, the identity, goes without one)", t, (long long)ks[t]);
      continue;
    }
    if (k->ctx != c) FHESI_FAIL("ct_rotations: the matrix of rotation %d belongs to another context", t);
    if (!k->hoist_k) FHESI_FAIL("ct_rotations: the matrix of rotation %d was not made by fhesi_ksk_hoist", t);
    if (k->hoist_k != ks[t]) FHESI_FAIL("ct_rotations: the matrix of rotation %d was hoisted for k=%lld, the call asks k=%lld", t, (long long)k->hoist_k, (long long)ks[t]);
    FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
  }
  return 0;
}
// out[t][i], i < count, at out + (t * count + i) ciphertexts; every argument checked by the caller
static int rotations_run(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                         int32_t nlimbs_in, int64_t count, uint64_t* out, int32_t nlimbs) {
  const i64 n = c->phim;
  const size_t ct_in = (size_t)2 * n * nlimbs_in, ct_out = (size_t)2 * n * nlimbs;
  CrtTables* t_all;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t_all));
  // the matrices, with their tables built before any digit row exists (ksaux_build borrows the digits' workspace slot)
  std::vector<int> keyed;
  int ks_mode = -1, nd = 0;
  for (int t = 0; t < nk; ++t) {
    if (!hoisted[t]) continue;
    int mode;
    FHESI_TRY(key_switch_form(c, hoisted[t], logQ, decomp_bytes, &mode));
    if (ks_mode >= 0 && mode != ks_mode) FHESI_FAIL("ct_rotations: matrices of one call run different forms (internal)");
    ks_mode = mode; nd = hoisted[t]->ndigits;
    keyed.push_back(t);
  }
  const int ncol = 2 * nd;
  const int how = c->opt.hoist_dot;
  if (how == 2 && !keyed.empty() && ks_mode != KS_MODE_LIMB32) FHESI_FAIL("ct_rotations: hoist_dot = 2 (the multi-matrix dot product) needs the four-prime limb form, this ring and chain run form %d", ks_mode);
  const i64 chunk = std::min<i64>(16384, keyed.empty() ? std::max<i64>(count, 1) : batch_chunk(c, ncol, ks_mode == KS_MODE_LIMB32, count));      // (the gather puts two polynomials per ciphertext on grid.y)
  // automatic, as measured at (2^15, logQ 512), 44 columns, 7 limbs (profiles/hoist_bench.json, profiles/hoist_crossover.json): the multi-matrix kernel is the
  // faster one at every batch up to 64 ciphertexts whatever the number of matrices (a tile no deeper than the batch below 8; above, dot32_kernel4's groups of
  // 48 ciphertexts leave a ragged last group), with 4 matrices up to 256 (3-5 %; with one matrix the per-matrix launch is 1-2 % ahead from 128 on), and at
  // 1024 -- the batch dot32_kernel4 is tuned for -- the per-matrix launches win by 3-4 %
  const i64 cmax = std::min(chunk, count);
  const bool multi = ks_mode == KS_MODE_LIMB32 && (how == 2 || (how == 0 && (cmax <= 64 || (keyed.size() >= 4 && cmax <= 256))));
  // groups of one table shape (limb count, limb width, centred or not, folded or not): one launch covers one shape
  struct Group { std::vector<int> ts; };
  std::vector<Group> groups;
  if (multi) {
    auto same = [&](const fhesi_ksk* a, const fhesi_ksk* b) {
      return a->aux_rows == b->aux_rows && a->aux_limb_bits == b->aux_limb_bits && a->aux_centred == b->aux_centred && a->aux_fold == b->aux_fold &&
             ks_recombine_takes_tail(c, t_all, a) == ks_recombine_takes_tail(c, t_all, b);
    };
    for (int t : keyed) {
      Group* g = nullptr;
      for (Group& q : groups) if (same(hoisted[q.ts[0]], hoisted[t])) { g = &q; break; }
      if (!g) { groups.emplace_back(); g = &groups.back(); }
      g->ts.push_back(t);
    }
  }
  // matrices per launch: the dot outputs of (matrices x ciphertexts) stay within what a full chunk of the batch pipeline puts into workspace slot 10
  const i64 full = keyed.empty() ? 1 : batch_chunk(c, ncol, ks_mode == KS_MODE_LIMB32, -1);
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    const u64* src = (const u64*)in + done * ct_in;
    auto dst = [&](int t) { return (u64*)out + ((size_t)t * count + done) * ct_out; };
    for (int t = 0; t < nk; ++t) if (!hoisted[t]) FHESI_TRY(rotation_close(c, 1, logQ, src, nlimbs_in, cnt, dst(t), nlimbs));
    if (keyed.empty()) continue;
    void *d_dig, *d_pre;
    FHESI_TRY(unscaled_digits(c, ks_mode, nd, logQ, decomp_bytes, src, nlimbs_in, cnt, &d_dig));
    FHESI_TRY(ws_reserve(c, 4, (size_t)cnt * ct_out * 8, &d_pre));      // one rotation's key-switched ciphertexts, in front of their sigma_k
    if (!multi) {
      for (int t : keyed) {
        FHESI_TRY(key_switch_finish(c, hoisted[t], ks_mode, logQ, decomp_bytes, d_dig, cnt, (uint64_t*)d_pre, nlimbs));
        FHESI_TRY(rotation_close(c, ks[t], logQ, (const u64*)d_pre, nlimbs, cnt, dst(t), nlimbs));
      }
      continue;
    }
    const i64 per = std::min<i64>(kDot32MultiMax, std::max<i64>(1, full / cnt));
    std::vector<const fhesi_ksk*> batch;
    for (const Group& g : groups) {
      const fhesi_ksk* k0 = hoisted[g.ts[0]];
      const int R = k0->aux_rows;
      const size_t o_words = (size_t)cnt * 2 * R * 4 * aux32_row_len(c);      // u32 words of one matrix's outputs
      const bool fold_tail = ks_recombine_takes_tail(c, t_all, k0);
      for (size_t j0 = 0; j0 < g.ts.size(); j0 += (size_t)per) {
        const int nj = (int)std::min<size_t>((size_t)per, g.ts.size() - j0);
        batch.clear();
        for (int j = 0; j < nj; ++j) batch.push_back(hoisted[g.ts[j0 + j]]);
        void* d_o;
        FHESI_TRY(ws_reserve(c, 10, (size_t)nj * o_words * 4, &d_o));
        bool mont = true;
        FHESI_TRY(launch_dot32_multi(c, batch.data(), nj, (const u32*)d_dig, ncol, cnt, (u32*)d_o, &mont));
        FHESI_TRY(launch_ntt32_inv(c, (u32*)d_o, (i64)nj * cnt * 2 * R, 4, 0, mont, !fold_tail));
        for (int j = 0; j < nj; ++j) {
          const int t = g.ts[j0 + j];
          FHESI_TRY(launch_ks_recombine(c, t_all, hoisted[t], (const u64*)((const u32*)d_o + (size_t)j * o_words), cnt * 2, (u64*)d_pre, nlimbs, fold_tail));
          FHESI_TRY(rotation_close(c, ks[t], logQ, (const u64*)d_pre, nlimbs, cnt, dst(t), nlimbs));
        }
      }
    }
  }
  return 0;
}
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na && nb && a0 < b0 + nb && b0 < a0 + na;
}
extern "C" int fhesi_ct_rotations_dev(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes,
                                      const uint64_t* in, int32_t nlimbs_in, int64_t count, uint64_t* out, int32_t nlimbs) {
  CHECK_CTX(c);
  FHESI_TRY(rotations_args(c, hoisted, ks, nk, logQ, decomp_bytes, nlimbs_in, count, nlimbs));
  if (!count || !nk) return 0;
  if (!in || !out) FHESI_FAIL("ct_rotations: null argument");
  if (ranges_overlap(in, (size_t)count * 2 * c->phim * nlimbs_in * 8, out, (size_t)nk * count * 2 * c->phim * nlimbs * 8)) FHESI_FAIL("ct_rotations: out overlaps in");
  return rotations_run(c, hoisted, ks, nk, logQ, decomp_bytes, in, nlimbs_in, count, out, nlimbs);
}

// --------------------------------------------------------------------------------------------- baby-step/giant-step matrix-vector products
// out[i] = Reduce(base[i] + sum_t Ciphertext >>= ks[t] of pre[t][i]), pre[t] at pre + t * term_stride words: ct_rot_sum_kernel where the ring has the signed
// gather, the composition -- rotation_close per term into workspace slot 15, launch_ct_add -- where it has not or option automorph_rows asks for the
// evaluation rows.  The same words either way.  Every argument checked by the caller; out may be base.
static_assert(FHESI_ROT_SUM_MAX_TERMS == kRotSumMax, "terms of one rotated-sum launch");
static int rot_sum_run(fhesi_ctx* c, const int64_t* ks, int32_t nk, int32_t logQ, const u64* base, const u64* pre, i64 term_stride, int64_t count, int32_t nlimbs, u64* out) {
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  bool composed = c->opt.automorph_rows != 0;
  for (i64 done = 0; done < count && !composed; done += 16384) {      // (two polynomials per ciphertext on grid.y)
    const i64 cnt = std::min<i64>(16384, count - done);
    const int r = launch_ct_rot_sum(c, ks, nk, logQ, base ? base + done * ct_words : nullptr, pre + done * ct_words, term_stride, cnt * 2, nlimbs, out + done * ct_words);
    if (r == 1) return 1;
    if (r == 2) composed = true;      // (said at the first chunk, before anything is launched)
  }
  if (!composed) return 0;
  const i64 chunk = 256;              // (the evaluation rows of a chunk: workspace slots 1 and 3)
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    u64* o = out + done * ct_words;
    bool have = base != nullptr;
    if (base && base != out) HIP_TRY(hipMemcpyAsync(o, base + done * ct_words, (size_t)cnt * ct_words * 8, hipMemcpyDeviceToDevice, c->stream));
    for (int t = 0; t < nk; ++t) {
      const u64* src = pre + (i64)t * term_stride + done * ct_words;
      if (!have) { FHESI_TRY(rotation_close(c, ks[t], logQ, src, nlimbs, cnt, o, nlimbs)); have = true; continue; }
      void* d_term;
      FHESI_TRY(ws_reserve(c, 15, (size_t)cnt * ct_words * 8, &d_term));
      FHESI_TRY(rotation_close(c, ks[t], logQ, src, nlimbs, cnt, (u64*)d_term, nlimbs));
      FHESI_TRY(launch_ct_add(c, o, (const u64*)d_term, cnt * 2 * c->phim, nlimbs, logQ));
    }
  }
  return 0;
}
extern "C" int fhesi_ct_rot_sum_dev(fhesi_ctx* c, const int64_t* ks, int32_t nk, int32_t logQ, const uint64_t* base, const uint64_t* pre, int64_t count, int32_t nlimbs,
                                    uint64_t* out) {
  CHECK_CTX(c);
  if (nk < 1) FHESI_FAIL("ct_rot_sum: %d terms", nk);
  if (count < 0) FHESI_FAIL("ct_rot_sum: negative count");
  if (!ks) FHESI_FAIL("ct_rot_sum: null argument");
  if (nlimbs < 1 || nlimbs > 32) FHESI_FAIL("ct_rot_sum: ciphertext coefficients of %d limbs are outside the supported 1..32", nlimbs);
  if (logQ < 1 || nlimbs * 64 < logQ) FHESI_FAIL("ct_rot_sum: coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  for (int t = 0; t < nk; ++t)
    if (!in_zm_star(c, ks[t])) FHESI_FAIL("ct_rot_sum: k=%lld of term %d is not in Zm*", (long long)ks[t], t);
  if (!count) return 0;
  if (!pre || !out) FHESI_FAIL("ct_rot_sum: null argument");
  const size_t ct_bytes = (size_t)2 * c->phim * nlimbs * 8;
  if (ranges_overlap(pre, (size_t)nk * count * ct_bytes, out, (size_t)count * ct_bytes)) FHESI_FAIL("ct_rot_sum: out overlaps pre");
  if (base && base != out && ranges_overlap(base, (size_t)count * ct_bytes, out, (size_t)count * ct_bytes)) FHESI_FAIL("ct_rot_sum: out overlaps base without being base");
  return rot_sum_run(c, ks, nk, logQ, base, pre, (i64)count * (i64)(ct_bytes / 8), count, nlimbs, out);
}

// host only: the B that minimises the key switches (B - 1) + (G - 1), G = ceil(nk / B); of equal sums the larger B -- baby steps are the hoisted, cheaper ones
extern "C" int fhesi_matvec_bsgs_plan(int64_t nk, int32_t* baby, int32_t* giant) {
  if (nk < 1 || nk > ((i64)1 << 20)) FHESI_FAIL("matvec_bsgs_plan: %lld diagonals outside [1, 2^20]", (long long)nk);
  if (!baby || !giant) FHESI_FAIL("matvec_bsgs_plan: null output");
  i64 best = 0, cost = -1;
  for (i64 b = 1; b <= nk; ++b) {
    const i64 g = (nk + b - 1) / b, s = b + g - 2;
    if (cost < 0 || s <= cost) { cost = s; best = b; }
  }
  *baby = (int32_t)best;
  *giant = (int32_t)((nk + best - 1) / best);
  return 0;
}

// ApplyKeySwitch(k, src[i]) of count unscaled two-part ciphertexts as they are, no automorphism: what rotations_run computes in front of sigma_k, one matrix at
// a time (its table built by the caller's key_switch_form, in front of any digit rows)
static int key_switch_plain_run(fhesi_ctx* c, const fhesi_ksk* k, int ks_mode, int32_t logQ, int32_t decomp_bytes, const u64* in, int32_t nlimbs, int64_t count, u64* out) {
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  const i64 chunk = std::min<i64>(16384, batch_chunk(c, 2 * k->ndigits, ks_mode == KS_MODE_LIMB32, count));
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    void* d_dig;
    FHESI_TRY(unscaled_digits(c, ks_mode, k->ndigits, logQ, decomp_bytes, in + done * ct_words, nlimbs, cnt, &d_dig));
    FHESI_TRY(key_switch_finish(c, k, ks_mode, logQ, decomp_bytes, d_dig, cnt, out + done * ct_words, nlimbs));
  }
  return 0;
}

// What every matrix-vector entry checks behind rotations_args: the prepared plaintext -- nk diagonals for each of nI x nJ blocks --, the capacity rule of
// a sum of `terms` products, the buffers: in [nJ][count], out [nI][count]
static int matvec_args(fhesi_ctx* c, const char* who, const fhesi_plain* w, int nI, int nJ, int32_t nk, int terms, int32_t logQ, const uint64_t* in, int32_t nlimbs,
                       int64_t count, const uint64_t* out) {
  if (!w) FHESI_FAIL("%s: null prepared plaintext", who);
  if (w->ctx != c) FHESI_FAIL("%s: the prepared plaintext belongs to another context", who);
  if (w->nw < (i64)nI * nJ * nk) FHESI_FAIL("%s: %lld rotations against %lld prepared diagonals", who, (long long)nI * nJ * nk, (long long)w->nw);
  const double chain = chain_bits(c), bits = plain_sum_bits(c->phim, c->pow2, c->phi_two_term, logQ, w->maxabs, terms);
  if (bits >= chain) FHESI_FAIL("%s: a sum of %d products needs %.0f bits, the chain holds %.0f", who, terms, std::ceil(bits), std::floor(chain));
  if (!count) return 0;
  if (!in || !out) FHESI_FAIL("%s: null argument", who);
  const size_t bytes = (size_t)count * 2 * c->phim * nlimbs * 8;
  if (ranges_overlap(in, nJ * bytes, out, nI * bytes)) FHESI_FAIL("%s: out overlaps in", who);
  return 0;
}
// out[i] = Reduce( sum_g rot_kg[g]( sum_j rot_kb[j](in[i]) (*) w[g B + j] ) )  (include/fhesi_hip.h): per chunk of ciphertexts the baby rotations from one digit
// set into the pool (slot 12), ONE plaintext sum with G groups per ciphertext (slot 13), one key switch per giant into its slice of slot 14, one rotated sum.
// flat (G = 1, no giant): the plaintext sums ARE the result and go straight to out -- fhesi_ct_matvec_dev; no slot 13 or 14, no rotated sum.  With several
// output blocks and a chunk below count (fhesi_ct_conv2d_dev in its flat form) a chunk's sums [nI][cnt] go to slot 13 and are copied block by block.
// g_mode: the giants' forms, their tables built by the caller.  Every argument checked by the caller.
// The grid of nI x nJ blocks (fhesi_ct_linear_grid_dev) runs the same schedule with two of its three factors shared: in [nJ][count], out [nI][count], w row
// (I nJ + J) nk + t.  The babies of input block J, from one digit set, serve every output block -- pool [nJ][nb][cnt]; the ONE plaintext sum has the
// groups (I, g, i) with the terms (J, j), so the sum over J is taken where sums are exact and free; the giants of output block I run once, behind it.  Slot 14
// holds the G key-switched sums of one output block at a time.  One block (nI = nJ = 1) is the schedule above, launch for launch.
static int matvec_run(fhesi_ctx* c, const fhesi_ksk* const* baby_hoisted, const int64_t* kb, int32_t B, const fhesi_ksk* const* giant_hoisted, const int64_t* kg,
                      const int* g_mode, int32_t G, bool flat, int nI, int nJ, int32_t nk, const fhesi_plain* w, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                      int32_t nlimbs, int64_t count, uint64_t* out) {
  const int nb = std::min(B, nk);      // (G = 1 with a ragged group: the babies past nk are not run)
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  const i64 nterms = (i64)nI * nJ * nk;      // terms of one ciphertext's sums
  // ciphertexts per pass: about 4 GiB of rotated ciphertexts, of inner sums and of key-switched sums each; and index lists that 32 bits hold
  i64 chunk = std::max<i64>(1, std::min<i64>(std::min<i64>(count, ((i64)1 << 31) / (nterms + 1) - 1),
                                            (i64)(4.0 * 1024 * 1024 * 1024 / ((double)std::max(nJ * nb, nI * G) * ct_words * 8))));
  if (c->opt.wave_operands > 0) chunk = std::max<i64>(1, std::min<i64>(chunk, c->opt.wave_operands / std::max(nJ * nb, nI * G)));      // (for tests: chunks below count)
  // flat with several output blocks: a chunk's sums come out as [nI][cnt], out is [nI][count] -- the same place only where one chunk covers count
  const bool gather = flat && nI > 1 && chunk < count;
  std::vector<int32_t> a_idx((size_t)chunk * nterms), b_idx((size_t)chunk * nterms), seg((size_t)chunk * nI * G + 1);
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    void *d_pool, *d_inner = out + (size_t)done * ct_words, *d_pre = nullptr;
    FHESI_TRY(ws_reserve(c, 12, (size_t)nJ * nb * cnt * ct_words * 8, &d_pool));
    if (!flat || gather) FHESI_TRY(ws_reserve(c, 13, (size_t)nI * G * cnt * ct_words * 8, &d_inner));
    if (!flat) FHESI_TRY(ws_reserve(c, 14, (size_t)G * cnt * ct_words * 8, &d_pre));
    for (int J = 0; J < nJ; ++J)
      FHESI_TRY(rotations_run(c, baby_hoisted, kb, nb, logQ, decomp_bytes, in + ((size_t)J * count + done) * ct_words, nlimbs, cnt,
                              (uint64_t*)d_pool + (size_t)J * nb * cnt * ct_words, nlimbs));
    // group (I G + g) cnt + i = sum_J sum_j pool[J][j][i] (*) w[(I nJ + J) nk + g B + j]  (conv_plan.h)
    grid_sum_lists(nI, nJ, nk, B, G, cnt, a_idx.data(), b_idx.data(), seg.data());
    FHESI_TRY(fhesi_ct_plain_sum_dev(c, w, logQ, (const uint64_t*)d_pool, (int64_t)nJ * nb * cnt, nlimbs, a_idx.data(), b_idx.data(), seg.data(), cnt * nI * G, (uint64_t*)d_inner));
    if (gather)
      for (int I = 0; I < nI; ++I)
        HIP_TRY(hipMemcpyAsync(out + ((size_t)I * count + done) * ct_words, (const u64*)d_inner + (size_t)I * cnt * ct_words, (size_t)cnt * ct_words * 8, hipMemcpyDeviceToDevice, c->stream));
    if (flat) continue;
    for (int I = 0; I < nI; ++I) {
      for (int g = 0; g < G; ++g) {
        const u64* inner = (const u64*)d_inner + ((size_t)I * G + g) * cnt * ct_words;
        u64* pre = (u64*)d_pre + (size_t)g * cnt * ct_words;
        if (!giant_hoisted[g]) HIP_TRY(hipMemcpyAsync(pre, inner, (size_t)cnt * ct_words * 8, hipMemcpyDeviceToDevice, c->stream));      // (k = 1: the sum itself)
        else FHESI_TRY(key_switch_plain_run(c, giant_hoisted[g], g_mode[g], logQ, decomp_bytes, inner, nlimbs, cnt, pre));
      }
      FHESI_TRY(rot_sum_run(c, kg, G, logQ, nullptr, (const u64*)d_pre, (i64)cnt * (i64)ct_words, cnt, nlimbs, out + ((size_t)I * count + done) * ct_words));
    }
  }
  return 0;
}
// out[i] = sum_t rot_t(in[i]) (*) w[t]: one giant step that is the identity -- the composition of fhesi_ct_rotations_dev and fhesi_ct_plain_sum_dev itself, so its bits
extern "C" int fhesi_ct_matvec_dev(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, const fhesi_plain* w, int32_t logQ,
                                   int32_t decomp_bytes, const uint64_t* in, int32_t nlimbs, int64_t count, uint64_t* out) {
  CHECK_CTX(c);
  if (nk < 1) FHESI_FAIL("ct_matvec: %d diagonals", nk);
  FHESI_TRY(rotations_args(c, hoisted, ks, nk, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(matvec_args(c, "ct_matvec", w, 1, 1, nk, nk, logQ, in, nlimbs, count, out));
  if (!count) return 0;
  return matvec_run(c, hoisted, ks, nk, nullptr, nullptr, nullptr, 1, true, 1, 1, nk, w, logQ, decomp_bytes, in, nlimbs, count, out);
}
extern "C" int fhesi_ct_matvec_bsgs_dev(fhesi_ctx* c, const fhesi_ksk* const* baby_hoisted, const int64_t* kb, int32_t B, const fhesi_ksk* const* giant_hoisted,
                                        const int64_t* kg, int32_t G, int32_t nk, const fhesi_plain* w, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                                        int32_t nlimbs, int64_t count, uint64_t* out) {
  CHECK_CTX(c);
  if (B < 1 || G < 1) FHESI_FAIL("ct_matvec_bsgs: %d baby steps and %d giant steps (at least 1 of each)", B, G);
  if ((i64)nk <= (i64)(G - 1) * B || (i64)nk > (i64)G * B) FHESI_FAIL("ct_matvec_bsgs: %d diagonals outside (%lld, %lld], what %d giant steps of %d baby steps cover", nk, (long long)(G - 1) * B, (long long)G * B, G, B);
  FHESI_TRY(rotations_args(c, baby_hoisted, kb, B, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(rotations_args(c, giant_hoisted, kg, G, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(matvec_args(c, "ct_matvec_bsgs", w, 1, 1, nk, std::min(B, nk), logQ, in, nlimbs, count, out));
  if (!count) return 0;
  // the giants' tables before any digit row exists, as rotations_run builds its matrices'
  std::vector<int> g_mode((size_t)G, -1);
  for (int g = 0; g < G; ++g) if (giant_hoisted[g]) FHESI_TRY(key_switch_form(c, giant_hoisted[g], logQ, decomp_bytes, &g_mode[g]));
  return matvec_run(c, baby_hoisted, kb, B, giant_hoisted, kg, g_mode.data(), G, false, 1, 1, nk, w, logQ, decomp_bytes, in, nlimbs, count, out);
}

// --------------------------------------------------------------------------------------------- folds and dense linear layers
// y[i] <- Reduce(y[i] + rot_ks[s](y[i])) for s = 0 .. nk-1, in place (include/fhesi_hip.h): per chunk of ciphertexts and step one key switch of y as it is
// into workspace slot 14 (a copy where the step has no matrix: k = 1), then the rotated sum with base = out = y.  mode: the matrices' forms, their tables
// built by the caller in front of any digit row.  Every argument checked by the caller.
static int rot_fold_run(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, const int* mode, int32_t logQ, int32_t decomp_bytes, u64* y,
                        int32_t nlimbs, int64_t count) {
  if (!nk) return 0;
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  const i64 chunk = std::max<i64>(1, std::min<i64>(count, (i64)(4.0 * 1024 * 1024 * 1024 / ((double)ct_words * 8))));      // about 4 GiB of key-switched ciphertexts
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    u64* o = y + (size_t)done * ct_words;
    void* d_pre;
    FHESI_TRY(ws_reserve(c, 14, (size_t)cnt * ct_words * 8, &d_pre));
    for (int s = 0; s < nk; ++s) {
      if (!hoisted[s]) HIP_TRY(hipMemcpyAsync(d_pre, o, (size_t)cnt * ct_words * 8, hipMemcpyDeviceToDevice, c->stream));
      else FHESI_TRY(key_switch_plain_run(c, hoisted[s], mode[s], logQ, decomp_bytes, o, nlimbs, cnt, (u64*)d_pre));
      FHESI_TRY(rot_sum_run(c, ks + s, 1, logQ, o, (const u64*)d_pre, (i64)cnt * (i64)ct_words, cnt, nlimbs, o));
    }
  }
  return 0;
}
static int key_switch_forms(fhesi_ctx* c, const fhesi_ksk* const* hoisted, int32_t nk, int32_t logQ, int32_t decomp_bytes, std::vector<int>* mode) {
  mode->assign((size_t)nk, -1);
  for (int t = 0; t < nk; ++t) if (hoisted[t]) FHESI_TRY(key_switch_form(c, hoisted[t], logQ, decomp_bytes, &(*mode)[t]));
  return 0;
}
extern "C" int fhesi_ct_rot_fold_dev(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                                     int32_t nlimbs, int64_t count, uint64_t* out) {
  CHECK_CTX(c);
  FHESI_TRY(rotations_args(c, hoisted, ks, nk, logQ, decomp_bytes, nlimbs, count, nlimbs));
  if (!count) return 0;
  if (!in || !out) FHESI_FAIL("ct_rot_fold: null argument");
  const size_t bytes = (size_t)count * 2 * c->phim * nlimbs * 8;
  if (in != out && ranges_overlap(in, bytes, out, bytes)) FHESI_FAIL("ct_rot_fold: out overlaps in without being in");
  std::vector<int> mode;
  FHESI_TRY(key_switch_forms(c, hoisted, nk, logQ, decomp_bytes, &mode));
  // y_0 = Reduce(in): the copy, times one
  if (in != out) HIP_TRY(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
  FHESI_TRY(launch_ct_mul_long(c, (u64*)out, count * 2 * c->phim, nlimbs, logQ, 1));
  return rot_fold_run(c, hoisted, ks, nk, mode.data(), logQ, decomp_bytes, (u64*)out, nlimbs, count);
}

// host only.  The amounts in the order fhesi_ct_linear_dev takes their matrices: babies, giants, folds
extern "C" int fhesi_linear_plan(int64_t cols, int64_t R, int64_t C, int32_t baby, int32_t* T_out, int32_t* B_out, int32_t* G_out, int32_t* nfold_out, int64_t* amounts) {
  if (cols < 1 || cols > ((i64)1 << 20)) FHESI_FAIL("linear_plan: a row of %lld slots outside [1, 2^20]", (long long)cols);
  if (R < 1 || C < 1) FHESI_FAIL("linear_plan: a %lld x %lld matrix (both sizes at least 1)", (long long)R, (long long)C);
  const i64 D = std::max(R, C), T = std::min(R, C);
  if (D > cols) FHESI_FAIL("linear_plan: max(R, C) = %lld exceeds the row of %lld slots", (long long)D, (long long)cols);
  if (cols % D) FHESI_FAIL("linear_plan: max(R, C) = %lld does not divide the row of %lld slots", (long long)D, (long long)cols);
  if (D % T) FHESI_FAIL("linear_plan: min(R, C) = %lld does not divide max(R, C) = %lld", (long long)T, (long long)D);
  int32_t nfold = 0;
  if (R < C) {
    const i64 q = C / R;
    if (q & (q - 1)) FHESI_FAIL("linear_plan: C / R = %lld is not a power of two", (long long)q);
    while (((i64)1 << nfold) < q) ++nfold;
  }
  if (baby < 0) FHESI_FAIL("linear_plan: %d baby steps", baby);
  int32_t B = (int32_t)std::min<i64>(baby, T), G = 0;
  if (!baby) FHESI_TRY(fhesi_matvec_bsgs_plan(T, &B, &G));
  G = (int32_t)((T + B - 1) / B);
  if (T_out) *T_out = (int32_t)T;
  if (B_out) *B_out = B;
  if (G_out) *G_out = G;
  if (nfold_out) *nfold_out = nfold;
  if (amounts) {
    for (int j = 1; j < B; ++j) *amounts++ = j;
    for (int g = 1; g < G; ++g) *amounts++ = (i64)g * B;
    for (i64 a = C / 2; R < C && a >= R; a /= 2) *amounts++ = a;
  }
  return 0;
}

// host only.  The grid of nI x nJ blocks of Rb x Cb: the block's plan with the B that suits the shared schedule -- the babies run once per input block, the
// giants once per output block, so B minimises nJ (B - 1) + nI (G - 1); of equal costs the larger B.  One block: what fhesi_linear_plan picks.
int linear_grid_plan(int64_t cols, int64_t R, int64_t C, int64_t Rb, int64_t Cb, int32_t baby, int32_t* nI_out, int32_t* nJ_out, int32_t* T_out, int32_t* B_out, int32_t* G_out,
                     int32_t* nfold_out, std::vector<int64_t>* amounts) {
  int32_t T = 0, B = 0, G = 0, nfold = 0;
  FHESI_TRY(fhesi_linear_plan(cols, Rb, Cb, baby, &T, &B, &G, &nfold, nullptr));      // the block's shape, in the planner's own words
  if (R < 1 || C < 1) FHESI_FAIL("linear_grid_plan: a %lld x %lld matrix (both sizes at least 1)", (long long)R, (long long)C);
  if (R % Rb) FHESI_FAIL("linear_grid_plan: R = %lld is not a multiple of the block's %lld rows (pad the matrix with zero rows)", (long long)R, (long long)Rb);
  if (C % Cb) FHESI_FAIL("linear_grid_plan: C = %lld is not a multiple of the block's %lld columns (pad the matrix with zero columns)", (long long)C, (long long)Cb);
  const i64 nI = R / Rb, nJ = C / Cb;
  if (nI * nJ > 65535 || nI * nJ * T > 65535) FHESI_FAIL("linear_grid_plan: %lld x %lld blocks of %d diagonals per handle, 1 .. 65535 diagonals are taken", (long long)nI, (long long)nJ, T);
  if (!baby) {
    i64 cost = -1;
    for (i64 b = 1; b <= T; ++b) {
      const i64 s = nJ * (b - 1) + nI * ((T + b - 1) / b - 1);
      if (cost < 0 || s <= cost) { cost = s; B = (int32_t)b; }
    }
    G = (T + B - 1) / B;
  }
  if (nI_out) *nI_out = (int32_t)nI;
  if (nJ_out) *nJ_out = (int32_t)nJ;
  if (T_out) *T_out = T;
  if (B_out) *B_out = B;
  if (G_out) *G_out = G;
  if (nfold_out) *nfold_out = nfold;
  if (amounts) {
    amounts->resize((size_t)(B - 1 + G - 1 + nfold));
    FHESI_TRY(fhesi_linear_plan(cols, Rb, Cb, B, nullptr, nullptr, nullptr, nullptr, amounts->data()));      // (baby = B > 0: min(B, T) = B)
  }
  return 0;
}
extern "C" int fhesi_linear_grid_plan(int64_t cols, int64_t R, int64_t C, int64_t Rb, int64_t Cb, int32_t baby, int32_t* nI_out, int32_t* nJ_out, int32_t* T_out, int32_t* B_out,
                                      int32_t* G_out, int32_t* nfold_out, int64_t* amounts) {
  std::vector<int64_t> a;
  FHESI_TRY(linear_grid_plan(cols, R, C, Rb, Cb, baby, nI_out, nJ_out, T_out, B_out, G_out, nfold_out, amounts ? &a : nullptr));
  std::copy(a.begin(), a.end(), amounts);
  return 0;
}

// k = g^amount mod m for each rotation amount of a plan on the space's rows
static std::vector<int64_t> rotation_ks(const fhesi_slots* s, const std::vector<int64_t>& amounts) {
  std::vector<int64_t> ks(amounts.size());
  for (size_t t = 0; t < amounts.size(); ++t) ks[t] = (int64_t)hm::powmod(s->S.g, (u64)amounts[t], (u64)s->ctx->m);
  return ks;
}
// out[I][i] += b_I: the biases embedded into the message staging slot -- the sums' index lists in it are dead -- and added through launch_ct_add_const
static int layer_add_bias(fhesi_ctx* c, const GridLayer& L, int32_t logQ, int32_t nlimbs, int64_t count, uint64_t* out) {
  if (!L.d_bias) return 0;
  const size_t n = (size_t)c->phim;
  void* d_msg;
  FHESI_TRY(ws_reserve(c, 5, (size_t)L.nI * n * 8, &d_msg));
  FHESI_TRY(slots_embed_rows(L.slots, L.d_bias, c->phim, false, L.nI, (i64*)d_msg));
  for (int I = 0; I < L.nI; ++I)
    FHESI_TRY(grid_chunks(count, [&](i64 done, i64 cnt) {
      return launch_ct_add_const(c, (u64*)out + ((size_t)I * count + done) * 2 * n * nlimbs, (const i64*)d_msg + (size_t)I * n, 1, 2, nlimbs, logQ, L.slots->S.p, cnt);
    }));
  return 0;
}
// The ONE run path of a layer (GridLayer, fhesi_internal.h): out[I][i] = sum_J (block or channel pair (I, J))(in[J][i]) + b_I on the slots -- matvec_run over
// the layer's plaintexts with the blocks or channels as its grid, the folds in place on out -- nI count ciphertexts in a row --, the biases.  The caller's
// matrices go to their places among the babies, giants and folds; every other place is the identity.  A dense block: the words of fhesi_ct_matvec_bsgs_dev,
// fhesi_ct_rot_fold_dev and fhesi_ct_add_slots_dev in that order.  A convolution: flat, B = kh kw and the plaintext sums are the result; split, B = kw
// babies (horizontal) and G = kh giants (vertical).  who: the entry point, what: its layer, for the refusals.
static int layer_run(fhesi_ctx* c, const char* who, const char* what, const GridLayer* L, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes,
                     const uint64_t* in, int32_t nlimbs, int64_t count, uint64_t* out) {
  CHECK_CTX(c);
  if (!L) FHESI_FAIL("%s: null %s", who, what);
  if (L->ctx != c) FHESI_FAIL("%s: the %s belongs to another context", who, what);
  const int B = L->B, G = L->G, nf = L->nfold, nI = L->nI, nJ = L->nJ, want = (int)L->amounts.size();
  if (nh != want) {
    if (L->anchored) FHESI_FAIL("%s: %d matrices, the layer takes %d (one per amount of its plan, NULL at the anchor)", who, nh, want);
    FHESI_FAIL("%s: %d matrices, the layer takes %d (%d baby, %d giant and %d fold rotations)", who, nh, want, B - 1, G - 1, nf);
  }
  if (nh && !hoisted) FHESI_FAIL("%s: null argument", who);
  if ((double)std::max(nI, nJ) * (double)count > 2147483647.0) {
    if (L->anchored) FHESI_FAIL("%s: %lld ciphertexts per channel exceed what %d -> %d channels can index", who, (long long)count, nJ, nI);
    FHESI_FAIL("%s: %lld ciphertexts per block exceed what the grid of %d x %d blocks can index", who, (long long)count, nI, nJ);
  }
  // the row [B babies][G giants][nf folds], the identity wherever no entry goes; k = g^amount mod m
  std::vector<const fhesi_ksk*> hs((size_t)(B + G + nf), nullptr);
  std::vector<int64_t> ks((size_t)(B + G + nf), 1);
  const std::vector<int64_t> k_entry = rotation_ks(L->slots, L->amounts);
  for (int t = 0; t < nh; ++t) {
    const i64 a = L->amounts[(size_t)t];
    if (L->anchored && !a && hoisted[t]) FHESI_FAIL("%s: a matrix at entry %d, whose amount is 0 (the anchor takes none)", who, t);
    if (L->anchored && a && !hoisted[t]) FHESI_FAIL("%s: entry %d has no matrix and its amount is %lld (only the anchor goes without one)", who, t, (long long)a);
    hs[(size_t)L->place[(size_t)t]] = hoisted[t];
    ks[(size_t)L->place[(size_t)t]] = k_entry[(size_t)t];
  }
  const fhesi_ksk* const* hb = hs.data(), * const* hg = hb + B, * const* hf = hg + G;
  const int64_t *kb = ks.data(), *kg = kb + B, *kf = kg + G;
  FHESI_TRY(rotations_args(c, hb, kb, B, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(rotations_args(c, hg, kg, G, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(rotations_args(c, hf, kf, nf, logQ, decomp_bytes, nlimbs, count, nlimbs));
  FHESI_TRY(matvec_args(c, who, L->w, nI, nJ, L->nk, (int)L->terms, logQ, in, nlimbs, count, out));
  if (!count) return 0;
  // every table before any digit row exists, as rotations_run builds its matrices'
  std::vector<int> g_mode, f_mode;
  FHESI_TRY(key_switch_forms(c, hg, G, logQ, decomp_bytes, &g_mode));
  FHESI_TRY(key_switch_forms(c, hf, nf, logQ, decomp_bytes, &f_mode));
  FHESI_TRY(matvec_run(c, hb, kb, B, hg, kg, g_mode.data(), G, L->flat, nI, nJ, L->nk, L->w, logQ, decomp_bytes, in, nlimbs, count, out));
  FHESI_TRY(rot_fold_run(c, hf, kf, nf, f_mode.data(), logQ, decomp_bytes, (u64*)out, nlimbs, (i64)nI * count));
  return layer_add_bias(c, *L, logQ, nlimbs, count, out);
}
extern "C" int fhesi_ct_linear_dev(fhesi_ctx* c, const fhesi_linear* lin, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                                   int32_t nlimbs, int64_t count, uint64_t* out) {
  return layer_run(c, "ct_linear", "linear layer", lin, hoisted, nh, logQ, decomp_bytes, in, nlimbs, count, out);
}
extern "C" int fhesi_ct_linear_grid_dev(fhesi_ctx* c, const fhesi_linear_grid* lin, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes,
                                        const uint64_t* in, int32_t nlimbs, int64_t count, uint64_t* out) {
  return layer_run(c, "ct_linear_grid", "linear grid", lin, hoisted, nh, logQ, decomp_bytes, in, nlimbs, count, out);
}
extern "C" int fhesi_ct_conv2d_dev(fhesi_ctx* c, const fhesi_conv2d* cv, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes, const uint64_t* in,
                                   int32_t nlimbs, int64_t count, uint64_t* out) {
  return layer_run(c, "ct_conv2d", "convolution layer", cv, hoisted, nh, logQ, decomp_bytes, in, nlimbs, count, out);
}

// --------------------------------------------------------------------------------------------- sum pooling on a lattice of the plane
// fhesi_pool2d_plan, fhesi_ct_pool2d_dev (include/fhesi_hip.h; lattice_plan.h): non-overlapping windows that tile the plane never cross its border, so
// there is no mask and NO plaintext product -- rotations and sums only.
extern "C" int fhesi_pool2d_plan(int64_t cols, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sy, int64_t sx, int32_t form, int32_t* form_out, int32_t* nh, int32_t* nhor,
                                 int64_t* key_switches, int32_t* levels, int64_t* out_sy, int64_t* out_sx, int64_t* amounts) {
  char why[256];
  const PoolShape sh{cols, H, W, kh, kw, sy, sx};
  if (pool_refused(sh, form, why, sizeof why)) FHESI_FAIL("pool2d_plan: %s", why);
  const PoolPlan pl = pool_plan(sh, form);
  if (form_out) *form_out = pl.form;
  if (nh) *nh = pl.nh;
  if (nhor) *nhor = pl.nhor;
  if (key_switches) *key_switches = pl.key_switches;
  if (levels) *levels = pl.levels;
  if (out_sy) *out_sy = pl.oy;
  if (out_sx) *out_sx = pl.ox;
  if (amounts) std::copy(pl.amounts.begin(), pl.amounts.end(), amounts);
  return 0;
}
// y[i] <- Reduce(y[i] + sum_t rot_ks[t](y[i])), t < nk, in place: the step rot_fold_run takes with nk terms in place of 1.  Per chunk of ciphertexts the
// digit rows of y ONCE, one key switch per term from them into consecutive slices of workspace slot 14, in front of their sigma_k, then ONE rotated sum
// with base = out = y -- every term read once, the result written once.  Every matrix present and of one form `ks_mode`, its table built by the caller in
// front of any digit row.  Every argument checked by the caller.
static int rot_hoisted_sum_run(fhesi_ctx* c, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int ks_mode, int32_t logQ, int32_t decomp_bytes, u64* y,
                               int32_t nlimbs, int64_t count) {
  if (!nk) return 0;
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  const int nd = hoisted[0]->ndigits;
  // ciphertexts per chunk: what the digit rows of the batch pipeline admit, and about 4 GiB of key-switched terms
  i64 chunk = std::min<i64>(std::min<i64>(16384, batch_chunk(c, 2 * nd, ks_mode == KS_MODE_LIMB32, count)), (i64)(4.0 * 1024 * 1024 * 1024 / ((double)nk * ct_words * 8)));
  if (c->opt.wave_operands > 0) chunk = std::min<i64>(chunk, c->opt.wave_operands / nk);      // (for tests: chunks below count)
  chunk = std::max<i64>(1, std::min<i64>(chunk, count));
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    u64* o = y + (size_t)done * ct_words;
    void *d_dig, *d_pre;
    FHESI_TRY(ws_reserve(c, 14, (size_t)nk * cnt * ct_words * 8, &d_pre));
    FHESI_TRY(unscaled_digits(c, ks_mode, nd, logQ, decomp_bytes, o, nlimbs, cnt, &d_dig));
    for (int t = 0; t < nk; ++t)
      FHESI_TRY(key_switch_finish(c, hoisted[t], ks_mode, logQ, decomp_bytes, d_dig, cnt, (uint64_t*)d_pre + (size_t)t * cnt * ct_words, nlimbs));
    FHESI_TRY(rot_sum_run(c, ks, nk, logQ, o, (const u64*)d_pre, (i64)cnt * (i64)ct_words, cnt, nlimbs, o));
  }
  return 0;
}
// out[i] = the window sums of in[i] (include/fhesi_hip.h).  Form 1: rot_hoisted_sum_run over the horizontal amounts, then over the vertical ones.  Form 2:
// rot_fold_run over the plan's amounts.  Both on y_0 = Reduce(in), as fhesi_ct_rot_fold_dev starts.
extern "C" int fhesi_ct_pool2d_dev(fhesi_slots* s, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sy, int64_t sx, int32_t form, const fhesi_ksk* const* hoisted, int32_t nh,
                                   int32_t logQ, int32_t decomp_bytes, const uint64_t* in, int32_t nlimbs, int64_t count, uint64_t* out) {
  const char* who = "ct_pool2d";
  if (!s) FHESI_FAIL("%s: null plaintext space", who);
  fhesi_ctx* c = s->ctx;
  CHECK_CTX(c);
  char why[256];
  const PoolShape sh{s->S.phim / s->S.rows, H, W, kh, kw, sy, sx};
  if (pool_refused(sh, form, why, sizeof why)) FHESI_FAIL("%s: %s", who, why);
  const PoolPlan pl = pool_plan(sh, form);
  if (nh != pl.nh) FHESI_FAIL("%s: %d matrices, the pooling takes %d (%d horizontal, %d vertical, one per amount of its plan)", who, nh, pl.nh, pl.nhor, pl.nh - pl.nhor);
  if (nh && !hoisted) FHESI_FAIL("%s: null argument", who);
  for (int t = 0; t < nh; ++t)
    if (!hoisted[t]) FHESI_FAIL("%s: entry %d has no matrix and its amount is %lld (every amount of a pooling takes one)", who, t, (long long)pl.amounts[(size_t)t]);
  const std::vector<int64_t> ks = rotation_ks(s, pl.amounts);
  FHESI_TRY(rotations_args(c, hoisted, ks.data(), nh, logQ, decomp_bytes, nlimbs, count, nlimbs));
  if (!count) return 0;
  if (!in || !out) FHESI_FAIL("%s: null argument", who);
  const size_t bytes = (size_t)count * 2 * c->phim * nlimbs * 8;
  if (in != out && ranges_overlap(in, bytes, out, bytes)) FHESI_FAIL("%s: out overlaps in without being in", who);
  std::vector<int> mode;      // every table before any digit row exists, as rotations_run builds its matrices'
  FHESI_TRY(key_switch_forms(c, hoisted, nh, logQ, decomp_bytes, &mode));
  for (int t = 1; t < nh; ++t) if (mode[(size_t)t] != mode[0]) FHESI_FAIL("%s: matrices of one call run different forms (internal)", who);
  // y_0 = Reduce(in): the copy, times one
  if (in != out) HIP_TRY(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
  FHESI_TRY(launch_ct_mul_long(c, (u64*)out, count * 2 * c->phim, nlimbs, logQ, 1));
  if (pl.form == 2) return rot_fold_run(c, hoisted, ks.data(), nh, mode.data(), logQ, decomp_bytes, (u64*)out, nlimbs, count);
  FHESI_TRY(rot_hoisted_sum_run(c, hoisted, ks.data(), pl.nhor, nh ? mode[0] : -1, logQ, decomp_bytes, (u64*)out, nlimbs, count));
  return rot_hoisted_sum_run(c, hoisted + pl.nhor, ks.data() + pl.nhor, nh - pl.nhor, nh ? mode[0] : -1, logQ, decomp_bytes, (u64*)out, nlimbs, count);
}

// One wave of Matrix<Ciphertext> arithmetic followed by the key switch (see include/fhesi_hip.h).
// Every group a single product (a loop of `c *= d; ApplyKeySwitch(c)` recorded by the host mirror, fhesi_engine.h): the operands are
// gathered into two batches and take the batch pipeline of fhesi_ct_mul_relin_batch_dev -- the tensor products formed in the loader
// of the inverse transform instead of the sum kernels below (19.6 k -> 22 k multiplications per second at the metric ring with the
// operands gathered, more with them addressed through the indices)
static int wave_single_products(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* pool, int32_t nlimbs,
                                const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, uint64_t* out) {
  const i64 ct_words = (i64)2 * c->phim * nlimbs, step = 1024;
  std::vector<int> ix;
  for (i64 g0 = 0; g0 < ngroups; g0 += step) {
    const i64 cnt = std::min<i64>(step, ngroups - g0);
    const size_t ops_bytes = (size_t)2 * cnt * ct_words * 8;
    // where the tensor half runs over the 30-bit primes its first kernel takes the operands through the indices (no copy at all);
    // elsewhere they are gathered into two batches first
    const bool indexed = tensor32_applies(c, p, nlimbs, logQ);
    void* d_ops;
    FHESI_TRY(ws_reserve(c, 12, (indexed ? 0 : ops_bytes) + sizeof(int) * 2 * (size_t)cnt, &d_ops));      // (a slot of its own: the pipeline called below uses most of the others)
    int* d_ix = (int*)((char*)d_ops + (indexed ? 0 : ops_bytes));
    ix.resize(2 * cnt);
    for (i64 g = 0; g < cnt; ++g) { ix[g] = a_idx[seg[g0 + g]]; ix[cnt + g] = b_idx[seg[g0 + g]]; }
    HIP_TRY(hipMemcpyAsync(d_ix, ix.data(), sizeof(int) * ix.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));             // ix is reused by the next chunk
    if (indexed) {
      c->op_idx = d_ix; c->op_idx_n = cnt; c->op_idx_done = 0;
      const int rc = mul_relin_chunks(c, k, logQ, p, decomp_bytes, (const u64*)pool, (const u64*)pool, out + (size_t)g0 * ct_words, nlimbs, cnt);
      c->op_idx = nullptr;
      if (rc) return rc;
    } else {
      FHESI_TRY(launch_gather(c, (const u64*)pool, d_ix, 2 * cnt, ct_words, (u64*)d_ops));
      FHESI_TRY(fhesi_ct_mul_relin_batch_dev(c, k, logQ, p, decomp_bytes, (const u64*)d_ops, (const u64*)d_ops + (size_t)cnt * ct_words, out + (size_t)g0 * ct_words, nlimbs, cnt));
    }
  }
  return 0;
}
// One pass of the plan (wave_plan.h; dix: its index words on the device): every distinct operand gathered (slot 7) and brought to evaluation form ONCE
// (slot 0; the 30-bit path keeps rows of its own) -- a matrix entry or a minor typically feeds many products --, the products formed and summed per
// group into d_sum (u32 rows on the 30-bit path)
static int wave_sum_pass(fhesi_ctx* c, const WavePass& P, const int* dix, bool t32, uint64_t p, const uint64_t* pool, int32_t nlimbs, u64* d_sum) {
  const i64 n = c->phim, ct_words = (i64)2 * n * nlimbs, nu = P.nua + P.nub;
  const int L = c->L;
  const int *slot_a = dix + nu, *slot_b = slot_a + P.nt, *gseg = slot_b + P.nt;
  void *d_ops, *d_rows = nullptr;
  FHESI_TRY(ws_reserve(c, 7, (size_t)nu * ct_words * 8, &d_ops));
  if (!t32) FHESI_TRY(ws_reserve(c, 0, (size_t)nu * 2 * L * n * 8, &d_rows));
  u64* d_a = (u64*)d_ops;
  u64* d_b = d_a + (size_t)P.nua * ct_words;
  FHESI_TRY(launch_gather(c, (const u64*)pool, dix, nu, ct_words, d_a));
  if (t32) return tensor32_sum_pass(c, d_a, P.nua, P.nub, slot_a, slot_b, gseg, P.ng, P.nt, P.accumulate, d_sum);
  // c1 = DoubleCRT(parts * p), c2 = DoubleCRT(other.parts)   (Ciphertext.cpp:169-176)
  const u64 lift[2] = {p, p};
  const std::vector<int> all = full_set(c);
  u64* ca = (u64*)d_rows;
  u64* cb = ca + (size_t)P.nua * 2 * L * n;
  FHESI_TRY(launch_rns_reduce(c, d_a, nlimbs, n, P.nua, 2, lift, ca, L, nullptr));
  FHESI_TRY(launch_rns_reduce(c, d_b, nlimbs, n, P.nub, 2, nullptr, cb, L, nullptr));
  FHESI_TRY(row_fwd(c, ca, nu * 2, L, nullptr, all.data()));
  return launch_tensor_sum(c, ca, cb, slot_a, slot_b, gseg, P.ng, P.accumulate, d_sum, (double)P.nt);
}
// The sums of all groups and their key switches.  The passes are planned first and their index words uploaded once (slot 5: alive to the last pass, across the
// key switches of earlier groups -- nothing on this path reserves it); the sums of a run of groups (slot 4) are key-switched together behind the pass that closes them.
static int wave_sums(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* pool, int32_t nlimbs,
                     const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, uint64_t* out) {
  const i64 n = c->phim;
  const int L = c->L;
  const i64 ct_words = (i64)2 * n * nlimbs, tp_words = (i64)3 * L * n;
  CrtTables* t_all;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t_all));
  const bool ks32 = ksaux_mode(c, t_all, k->ncomp * k->ndigits, 8 * decomp_bytes, logQ) == KS_MODE_LIMB32;
  const i64 chunk = batch_chunk(c, 3 * k->ndigits, ks32);           // groups per key-switch call
  // distinct operands per pass: bound their evaluation-form rows (2 L n words each) to about 4 GiB
  i64 ucap = (i64)(4.0 * 1024 * 1024 * 1024 / ((double)2 * L * n * 8));
  // the sums' integers over primes below 2^30 where that path applies (kernels_tensor32.hip; tProd is not visible from here either)
  i64 gmax = 1;
  for (i64 g = 0; g < ngroups; ++g) gmax = std::max<i64>(gmax, seg[g + 1] - seg[g]);
  const bool t32 = tensor32_sum_applies(c, p, nlimbs, logQ, gmax);
  if (t32) {
    FHESI_TRY(tensor32_sum_begin(c, p, nlimbs, logQ, gmax));
    ucap = (i64)(4.0 * 1024 * 1024 * 1024 / ((double)tensor32_sum_bytes(c, 1) / 3 * 2));
  }
  if (c->opt.wave_operands > 1) ucap = c->opt.wave_operands;
  if (ucap < 2) ucap = 2;
  // a's and b's are operands alike, counted apart; one group over ucap goes in pieces of ucap / 2 terms
  const WavePlan plan = wave_plan(a_idx, b_idx, seg, ngroups, chunk, ucap, true);
  void* d_ix;
  FHESI_TRY(ws_reserve(c, 5, sizeof(int) * plan.ix.size(), &d_ix));
  HIP_TRY(hipMemcpyAsync(d_ix, plan.ix.data(), sizeof(int) * plan.ix.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                 // the one synchronisation: the plan lives on this frame
  void* d_sum = nullptr;
  for (const WavePass& P : plan.passes) {
    // (a piece that accumulates keeps the rows its first piece reserved)
    if (!P.accumulate) FHESI_TRY(ws_reserve(c, 4, t32 ? tensor32_sum_bytes(c, P.ng) : (size_t)P.ng * tp_words * 8, &d_sum));
    FHESI_TRY(wave_sum_pass(c, P, (const int*)d_ix + P.off, t32, p, pool, nlimbs, (u64*)d_sum));
    if (!P.close) continue;
    uint64_t* o = out + (size_t)P.g * ct_words;
    if (t32) {
      void* d_parts;
      FHESI_TRY(ws_reserve(c, 2, (size_t)P.ng * 3 * ((logQ + 63) / 64) * n * 8, &d_parts));
      const bool wm = c->opt.parts_words && ks32;
      FHESI_TRY(tensor32_sum_finish(c, d_sum, P.ng, (u64*)d_parts, wm));
      FHESI_TRY(key_switch_tail(c, k, logQ, decomp_bytes, (const u64*)d_parts, P.ng, o, nlimbs, wm));
    } else {
      FHESI_TRY(fhesi_apply_key_switch_dev(c, k, logQ, decomp_bytes, (const uint64_t*)d_sum, P.ng, o, nlimbs));
    }
  }
  return 0;
}
extern "C" int fhesi_ct_mul_sum_relin_dev(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* pool,
                                          int32_t nlimbs, const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, uint64_t* out) {
  CHECK_CTX(c);
  FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
  if (k->ncomp != 3) FHESI_FAIL("ct_mul_sum_relin needs the s^2 -> s matrix (3 source components), got %d", k->ncomp);
  if (!ngroups) return 0;
  for (i64 g = 0; g < ngroups; ++g) if (seg[g + 1] <= seg[g]) FHESI_FAIL("ct_mul_sum_relin: group %lld is empty", (long long)g);
  bool single = c->opt.wave_single != 0;
  for (i64 g = 0; single && g < ngroups; ++g) single = seg[g + 1] - seg[g] == 1;
  return (single ? wave_single_products : wave_sums)(c, k, logQ, p, decomp_bytes, pool, nlimbs, a_idx, b_idx, seg, ngroups, out);
}

// --------------------------------------------------------------------------------------------- polynomial activations
// host only: the plan of a dense polynomial (poly_plan.h; tests/poly_model.py states it)
extern "C" int fhesi_poly_eval_plan(int32_t degree, int32_t baby, int32_t* B, int32_t* G, int32_t* nprod, int32_t* nks, int32_t* depth) {
  if (degree < 1 || degree > kPolyMaxDegree) FHESI_FAIL("poly_eval_plan: degree %d outside 1 .. %d", degree, kPolyMaxDegree);
  if (baby < 0 || baby > degree) FHESI_FAIL("poly_eval_plan: %d baby powers outside 0 .. %d (0 = choose)", baby, degree);
  const PolyCounts pc = poly_plan(degree, baby);
  if (B) *B = pc.B;
  if (G) *G = pc.G;
  if (nprod) *nprod = pc.nprod;
  if (nks) *nks = pc.nks;
  if (depth) *depth = pc.depth;
  return 0;
}
// out[i] = f(in[i]) slot by slot (include/fhesi_hip.h): the schedule of poly_plan.h through the public entry points, per chunk of ciphertexts.  One workspace
// slot (13: nothing fhesi_ct_mul_sum_relin_dev or fhesi_ct_lin_comb_dev calls reserves it) holds the entries of a chunk, entry e of item i at e cnt + i: the
// powers (the input copied to entry 0), the inner sums, W -- one buffer, because the outer sum's operands and the closing combination's are each ONE pool.
// A level of powers is one wave of single products written into the pool it reads (its destinations are entries no product of the level reads); all inner
// sums one scalar combination (pool: the powers; out: the entries behind them); W one wave of one group per item; y one scalar combination into out.
// Every argument checked and the schedule built by the caller.
static int poly_eval_run(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const PolySchedule& s, const uint64_t* in, int32_t nlimbs,
                         int64_t count, uint64_t* out) {
  const size_t ct_words = (size_t)2 * c->phim * nlimbs;
  const int ninner = (int)s.inner.size();
  // ciphertexts per chunk: about 4 GiB of powers and of sums each (option "wave_operands": at most that many entries, for tests); index lists that 32 bits hold
  i64 chunk = (i64)(4.0 * 1024 * 1024 * 1024 / ((double)std::max(s.npowers, ninner + 1) * ct_words * 8));
  if (c->opt.wave_operands > 0) chunk = std::min<i64>(chunk, c->opt.wave_operands / s.nentries);
  chunk = std::max<i64>(1, std::min<i64>(std::min<i64>(chunk, count), ((i64)1 << 30) / ((i64)s.nentries * (s.B + 1))));
  void* d_pool_v;
  FHESI_TRY(ws_reserve(c, 13, (size_t)s.nentries * chunk * ct_words * 8, &d_pool_v));
  u64* d_pool = (u64*)d_pool_v;
  std::vector<int32_t> a_idx, b_idx, seg;
  std::vector<int64_t> coef, konst;
  for (i64 done = 0; done < count; done += chunk) {
    const i64 cnt = std::min(chunk, count - done);
    auto at = [&](int entry, i64 i) { return (int32_t)((i64)entry * cnt + i); };
    HIP_TRY(hipMemcpyAsync(d_pool, in + (size_t)done * ct_words, (size_t)cnt * ct_words * 8, hipMemcpyDeviceToDevice, c->stream));      // x^1: the input as it is
    for (const std::vector<PolyProduct>& level : s.levels) {
      a_idx.clear(); b_idx.clear(); seg.assign(1, 0);
      for (const PolyProduct& pr : level)
        for (i64 i = 0; i < cnt; ++i) { a_idx.push_back(at(pr.a, i)); b_idx.push_back(at(pr.b, i)); seg.push_back((int32_t)a_idx.size()); }
      FHESI_TRY(fhesi_ct_mul_sum_relin_dev(c, k, logQ, p, decomp_bytes, d_pool, nlimbs, a_idx.data(), b_idx.data(), seg.data(), (int64_t)level.size() * cnt,
                                           d_pool + (size_t)level[0].dst * cnt * ct_words));
    }
    if (ninner) {
      a_idx.clear(); coef.clear(); konst.clear(); seg.assign(1, 0);
      for (const PolyInner& u : s.inner)
        for (i64 i = 0; i < cnt; ++i) {
          for (const PolyTerm& t : u.terms) { a_idx.push_back(at(t.entry, i)); coef.push_back(t.c); }
          seg.push_back((int32_t)a_idx.size());
          konst.push_back(u.konst);
        }
      FHESI_TRY(fhesi_ct_lin_comb_dev(c, logQ, p, d_pool, (int64_t)s.npowers * cnt, nlimbs, a_idx.data(), coef.data(), seg.data(), konst.data(), (int64_t)ninner * cnt,
                                      d_pool + (size_t)s.npowers * cnt * ct_words));
      a_idx.clear(); b_idx.clear(); seg.assign(1, 0);
      for (i64 i = 0; i < cnt; ++i) {
        for (int u = 0; u < ninner; ++u) { a_idx.push_back(at(s.npowers + u, i)); b_idx.push_back(at(s.power_entry(s.inner[u].g * s.B), i)); }
        seg.push_back((int32_t)a_idx.size());
      }
      FHESI_TRY(fhesi_ct_mul_sum_relin_dev(c, k, logQ, p, decomp_bytes, d_pool, nlimbs, a_idx.data(), b_idx.data(), seg.data(), cnt, d_pool + (size_t)s.w_entry * cnt * ct_words));
    }
    a_idx.clear(); coef.clear(); konst.assign((size_t)cnt, s.final_konst); seg.assign(1, 0);
    for (i64 i = 0; i < cnt; ++i) {
      for (const PolyTerm& t : s.final_terms) { a_idx.push_back(at(t.entry, i)); coef.push_back(t.c); }
      seg.push_back((int32_t)a_idx.size());
    }
    FHESI_TRY(fhesi_ct_lin_comb_dev(c, logQ, p, d_pool, (int64_t)s.nentries * cnt, nlimbs, a_idx.data(), coef.data(), seg.data(), konst.data(), cnt, out + (size_t)done * ct_words));
  }
  return 0;
}
extern "C" int fhesi_ct_poly_eval_dev(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const int64_t* coef, int32_t degree, int32_t baby,
                                      const uint64_t* in, int32_t nlimbs, int64_t count, uint64_t* out) {
  CHECK_CTX(c);
  FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
  if (k->ncomp != 3) FHESI_FAIL("ct_poly_eval needs the s^2 -> s matrix (3 source components), got %d", k->ncomp);
  if (nlimbs < 1 || nlimbs > 32) FHESI_FAIL("ct_poly_eval: ciphertext coefficients of %d limbs are outside the supported 1..32", nlimbs);
  if (logQ < 1) FHESI_FAIL("ct_poly_eval: logQ=%d", logQ);
  if (p < 2 || p >= (1ull << 62)) FHESI_FAIL("ct_poly_eval: plaintext modulus %llu outside [2, 2^62)", (unsigned long long)p);
  if (degree < 1 || degree > kPolyMaxDegree) FHESI_FAIL("ct_poly_eval: degree %d outside 1 .. %d", degree, kPolyMaxDegree);
  if (baby < 0 || baby > degree) FHESI_FAIL("ct_poly_eval: %d baby powers outside 0 .. %d (0 = choose)", baby, degree);
  if (count < 0) FHESI_FAIL("ct_poly_eval: negative count");
  if (!coef) FHESI_FAIL("ct_poly_eval: null coefficients");
  if (!count) return 0;
  if (!in || !out) FHESI_FAIL("ct_poly_eval: null argument");
  const size_t bytes = (size_t)count * 2 * c->phim * nlimbs * 8;
  if (ranges_overlap(in, bytes, out, bytes)) FHESI_FAIL("ct_poly_eval: out overlaps in");
  return poly_eval_run(c, k, logQ, p, decomp_bytes, poly_schedule(coef, degree, p, poly_plan(degree, baby).B), in, nlimbs, count, out);
}

// Ciphertexts per launch of the fused multiplication.  ks32: the key switch really runs over the four 30-bit auxiliary primes (ksaux_mode
// said KS_MODE_LIMB32) -- only then does the large-launch policy below apply; the 64-bit forms keep the smaller chunks measured for them.
static i64 batch_chunk(fhesi_ctx* c, int ncol, bool ks32, i64 count) {
  if (c->opt.batch_chunk > 0) return c->opt.batch_chunk;
  i64 ch;
  double per;                                              // workspace bytes per ciphertext of a chunk (estimate)
  if (ks32) {
    // the 32-bit pipelines (key switch over the four auxiliary primes, tensor half over primes below 2^30): the larger the launch the
    // better -- 64 per launch 22.1 k mults/s, 128: 22.5 k, 512: 22.7 k, 1024: 23.0 k at the metric ring (more ciphertext tiles per key
    // block in the dot product, fewer launch tails; running the tensor half and the digit transforms in sub-chunks of 64 so that their
    // intermediate rows stay in the Infinity Cache, and only the dot product and what follows per chunk, measured 22.8 k against 23.3 k
    // for every stage per chunk) -- so: what fits about 48 GiB of workspace (digit rows ncol * 2 * row * 8 bytes per
    // ciphertext, the dot product's outputs and the tensor half's rows about 1.6 times that again), at most 1024
    per = (double)ncol * 2 * (double)aux32_row_len(c) * 8.0 * 2.6;
    ch = (i64)(48.0 * 1024 * 1024 * 1024 / per);
    ch = ch < 1 ? 1 : (ch > 1024 ? 1024 : ch);
  } else {
    // about 75k digit rows per chunk (150 rounds of the transform's 512 resident workgroups): measured best on MI355X at both the
    // metric ring (64 mults, 9.3 GiB of digit rows) and the stress ring (16-17 mults, 18 GiB) -- smaller chunks pay launch tails in
    // every stage, larger ones push the key rows out of the Infinity Cache during the dot product.  Capped at 32 GiB of digit rows.
    const double rows_per = (double)ncol * c->L, bytes_per = rows_per * c->phim * 8.0;
    ch = (i64)(76800.0 / rows_per);
    const i64 cap = (i64)(32.0 * 1024 * 1024 * 1024 / bytes_per);
    if (ch > cap) ch = cap;
    per = bytes_per + 5.0 * c->L * c->phim * 8.0;          // + tProd and the two scratch DoubleCRTs
  }
  // never more than the device can hold: what is free now plus what this lane's workspace already owns, minus a margin (the other lane of
  // option lanes = 2 keeps a second set, hence half of the free memory each)
  // (a call whose whole batch needs less than a gigabyte skips the query: hipMemGetInfo costs tens of microseconds, a quarter of the issue
  // time of a single multiplication; should the allocation fail after all, the chunk is halved and retried like any other)
  size_t free_b = 0, total_b = 0;
  if (count >= 0 && (double)count * per * 1.15 < 1024.0 * 1024 * 1024) return std::min<i64>(ch, std::max<i64>(count, 1));
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    double have = (double)free_b / (c->opt.lanes >= 2 ? 2.0 : 1.0);
    for (int i = 0; i < FHESI_WS_SLOTS; ++i) have += (double)c->ws_bytes[i];
    have -= 2.0 * 1024 * 1024 * 1024;
    const i64 fit = have > per ? (i64)(have / (per * 1.15)) : 1;
    if (ch > fit) ch = fit;
  } else (void)hipGetLastError();
  return ch < 1 ? 1 : ch;
}

static int mul_relin_chunks(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* a, const uint64_t* b,
                            uint64_t* out, int32_t nlimbs, int64_t count) {
  const i64 n = c->phim;
  const int L = c->L;
  CrtTables* t;
  FHESI_TRY(get_crt_tables(c, full_set(c), &t));
  const int ks_mode = ksaux_mode(c, t, k->ncomp * k->ndigits, 8 * decomp_bytes, logQ);
  i64 chunk = batch_chunk(c, 3 * k->ndigits, ks_mode == KS_MODE_LIMB32, count);
  for (i64 done = 0; done < count;) {
    const i64 cnt = std::min(chunk, count - done);
    const size_t off = (size_t)done * 2 * n * nlimbs;
    c->ws_oom = false;
    int rc;
    if (k->ncomp == 3 && tensor32_applies(c, p, nlimbs, logQ)) {
      // tProd is not visible from here: its integers are formed over primes below 2^30 (kernels_tensor32.hip), straight to the scaled-down parts
      FHESI_TRY(key_switch_args(c, k, logQ, decomp_bytes, nlimbs));
      void* d_parts = nullptr;
      rc = ws_reserve(c, 2, (size_t)cnt * 3 * ((logQ + 63) / 64) * n * 8, &d_parts);
      if (c->op_idx) c->op_idx_done = done;                  // indexed operands: the chunk is a window of the index arrays, the buffer stays put
      const bool wm = ks_mode == KS_MODE_LIMB32 && c->opt.parts_words;      // (the digit loader of the four-prime form reads word rows in whole lines)
      if (!rc) rc = launch_tensor32(c, p, c->op_idx ? a : a + off, c->op_idx ? b : b + off, nlimbs, logQ, cnt, (u64*)d_parts, wm);
      if (!rc) rc = key_switch_tail(c, k, logQ, decomp_bytes, (const u64*)d_parts, cnt, out + off, nlimbs, wm);
    } else {
      if (c->op_idx) FHESI_FAIL("ct_mul_relin: indexed operands reached the chain path");      // (only the 30-bit tensor half reads through indices; the caller checks tensor32_applies)
      void* d_tp = nullptr;
      rc = ws_reserve(c, 1, (size_t)cnt * 3 * L * n * 8, &d_tp);
      if (!rc) rc = fhesi_ct_mul_dev(c, p, a + off, b + off, nlimbs, cnt, (uint64_t*)d_tp);
      if (!rc) rc = key_switch_args(c, k, logQ, decomp_bytes, nlimbs);
      if (!rc) rc = apply_key_switch_consume(c, k, logQ, decomp_bytes, (u64*)d_tp, cnt, out + off, nlimbs);      // the chunk's tProd is ours: no copy
    }
    if (rc) {
      // a workspace allocation failed (a device with less free memory than the estimate assumed): the chunk is redone at half the size --
      // every stage of a chunk writes only workspace and its own slice of `out`, so nothing of the failed attempt survives
      // The grow-only slots that already grew for the oversized attempt are released first: left in place they would compete with the smaller
      // attempt for the same memory and the halving could run down to one ciphertext on a device that fits a mid-sized chunk.
      if (c->ws_oom && cnt > 1) {
        hipStreamSynchronize(c->stream);
        for (int slot : {0, 1, 2, 5, 10}) if (c->ws[slot]) { hipFree(c->ws[slot]); c->ws[slot] = nullptr; c->ws_bytes[slot] = 0; }
        (void)hipGetLastError();
        fhesi_set_error("%s", "");
        chunk = (cnt + 1) / 2;
        continue;
      }
      c->ws_oom = false;
      return rc;
    }
    done += cnt;
  }
  c->ws_oom = false;
  return 0;
}
static void swap_lane(fhesi_ctx* c) {
  std::swap(c->stream, c->lane_stream);
  for (int i = 0; i < FHESI_WS_SLOTS; ++i) { std::swap(c->ws[i], c->lane_ws[i]); std::swap(c->ws_bytes[i], c->lane_ws_bytes[i]); }
}

extern "C" int fhesi_ct_mul_relin_batch_dev(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* a,
                                            const uint64_t* b, uint64_t* out, int32_t nlimbs, int64_t count) {
  CHECK_CTX(c);
  if (!k || k->ctx != c) FHESI_FAIL("KeySwitchSI: context mismatch");
  if (k->ncomp != 3) FHESI_FAIL("ct_mul_relin needs the s^2 -> s matrix (3 source components), got %d", k->ncomp);
  if (nlimbs * 64 < logQ) FHESI_FAIL("coefficients of %d limbs cannot hold logQ=%d bits", nlimbs, logQ);
  const int lanes = c->opt.lanes;    // 2: two concurrent half-batches (+4 % with launches of 64 ciphertexts, +0.6 % with launches of 1024; kernels of the halves time-share the GPU)
  if (lanes < 2 || count < 8 || !c->pow2) return mul_relin_chunks(c, k, logQ, p, decomp_bytes, a, b, out, nlimbs, count);
  // two lanes: the second half of the batch runs on a second stream with its own workspace.  Ciphertexts are independent, so
  // the halves never touch the same memory; the fork / join events keep the call's stream semantics (work is ordered after
  // what was enqueued on the context's stream before the call, and fhesi_ctx_sync covers both halves afterwards).
  const int64_t h0 = (count + 1) / 2, h1 = count - h0;
  const size_t off = (size_t)h0 * 2 * c->phim * nlimbs;
  const int stagger = c->opt.stagger;   // measured slower than starting both lanes together
  HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
  HIP_TRY(hipStreamWaitEvent(c->lane_stream, c->ev_fork, 0));
  c->mark_mid = stagger != 0;
  int r = mul_relin_chunks(c, k, logQ, p, decomp_bytes, a, b, out, nlimbs, h0);
  if (!r) {
    // stagger: the second lane starts when the first lane's digit NTT (VALU-bound) has been issued, so that its own NTT
    // runs against the first lane's HBM-bound dot product / CRT tail instead of in lockstep with its NTT
    if (stagger) HIP_TRY(hipStreamWaitEvent(c->lane_stream, c->ev_mid, 0));
    swap_lane(c);
    r = mul_relin_chunks(c, k, logQ, p, decomp_bytes, a + off, b + off, out + off, nlimbs, h1);
    hipEventRecord(c->ev_join, c->stream);        // (c->stream is the lane stream here)
    swap_lane(c);
    if (!r) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  return r;
}

// ---------------------------------------------------------------------------------------------- host buffers
// fhesi_ct_mul_relin_batch takes and returns HOST buffers (what a caller of the class surface holds: Test_AddMul.cpp:59-67).  6 MiB cross the
// bus per multiplication at the metric ring (two operands in, one result out), and a pageable hipMemcpy moves them through the runtime's
// own bounce buffer on one thread, strictly before and after the compute: 2.9 k mults/s where the device does 24 k and the bus allows ~12 k.
// Here the batch runs as a pipeline of stages of `host_chunk` ciphertexts over a ring of two PINNED slots:
//     caller's a, b --(copy threads)--> pinned slot --(stream `up`, DMA)--> device slot --(context stream: the fused pipeline)-->
//     device slot --(stream `down`, DMA)--> pinned slot --(copy threads)--> caller's out
// so the upload of stage i + 1, the compute of stage i and the download of stage i - 1 overlap, and the pageable side is copied by several
// threads.  Buffers the caller allocated pinned (fhesi_host_alloc, or any hipHostMalloc / registered memory) skip the copy threads: the DMA
// reads and writes them directly.  Results are those of fhesi_ct_mul_relin_batch_dev bit for bit (the same calls on the same values).
struct HostStage {
  static constexpr int NS = 2;
  size_t slot_bytes = 0;                 // bytes per operand per slot
  void* pin[NS][3] = {};                 // a, b, out
  void* dev[NS][3] = {};
  hipStream_t up = nullptr, down = nullptr;
  hipEvent_t ev_up[NS] = {}, ev_comp[NS] = {}, ev_down[NS] = {};
  std::vector<hipEvent_t> ev_piece[NS];  // one per downloaded piece of a stage (pageable results)
  CopyPool pool;                         // copy threads between pageable memory and the ring (copy_pool.h)
  void copy(void* d, const void* s, size_t n) { pool.copy(d, s, n); }
  void release() {
    pool.stop();
    for (int s = 0; s < NS; ++s) for (int k = 0; k < 3; ++k) { if (pin[s][k]) hipHostFree(pin[s][k]); if (dev[s][k]) hipFree(dev[s][k]); pin[s][k] = dev[s][k] = nullptr; }
    for (int s = 0; s < NS; ++s) { if (ev_up[s]) hipEventDestroy(ev_up[s]); if (ev_comp[s]) hipEventDestroy(ev_comp[s]); if (ev_down[s]) hipEventDestroy(ev_down[s]); for (hipEvent_t e : ev_piece[s]) hipEventDestroy(e); ev_piece[s].clear(); }
    if (up) hipStreamDestroy(up);
    if (down) hipStreamDestroy(down);
  }
};
void host_stage_free(fhesi_ctx* c) {
  if (!c->host_stage) return;
  c->host_stage->release();
  delete c->host_stage;
  c->host_stage = nullptr;
}
static int host_stage_get(fhesi_ctx* c, size_t slot_bytes, HostStage** out) {
  HostStage* h = c->host_stage;
  if (!h) {
    h = new HostStage();
    c->host_stage = h;
    HIP_TRY(hipStreamCreateWithFlags(&h->up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&h->down, hipStreamNonBlocking));
    for (int s = 0; s < HostStage::NS; ++s) {
      HIP_TRY(hipEventCreateWithFlags(&h->ev_up[s], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_comp[s], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_down[s], hipEventDisableTiming));
    }
  }
  {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int T = c->opt.host_threads > 0 ? c->opt.host_threads : (int)std::min(8u, hw);      // (8 measured best on a 256-thread host: 4 slightly slower, 16 - 64 progressively slower -- the pieces are 8 MiB)
    if (h->pool.threads() != T) { h->pool.stop(); h->pool.start(T - 1); }      // (first use, or the option changed)
  }
  if (h->slot_bytes < slot_bytes) {
    HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipStreamSynchronize(h->up)); HIP_TRY(hipStreamSynchronize(h->down));
    for (int s = 0; s < HostStage::NS; ++s) for (int k = 0; k < 3; ++k) {
      if (h->pin[s][k]) { hipHostFree(h->pin[s][k]); h->pin[s][k] = nullptr; }
      if (h->dev[s][k]) { hipFree(h->dev[s][k]); h->dev[s][k] = nullptr; }
    }
    h->slot_bytes = 0;
    for (int s = 0; s < HostStage::NS; ++s) for (int k = 0; k < 3; ++k) {
      if (hipHostMalloc(&h->pin[s][k], slot_bytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&h->dev[s][k], slot_bytes) != hipSuccess) { (void)hipGetLastError(); FHESI_FAIL("host staging: allocation of %zu bytes (pinned + device) failed", slot_bytes); }
    }
    h->slot_bytes = slot_bytes;
  }
  *out = h;
  return 0;
}
// 0: pageable (or unknown to the runtime), 1: pinned / registered host memory covering [p, p + bytes), 2: device or managed memory (rejected
// by the host-buffer entry: its staging copies are CPU memcpy).  A range only partly registered counts as pageable: the copy threads can
// read and write it, the DMA engines could not.
static int host_ptr_kind(const void* p, size_t bytes) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray) return 2;
  if (at.type != hipMemoryTypeHost) return 0;          // (unregistered and MANAGED memory: the CPU can read it -- the staging path, like pageable memory)
  if (bytes > 1) {
    hipPointerAttribute_t end;
    if (hipPointerGetAttributes(&end, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (end.type != hipMemoryTypeHost) return 0;
  }
  return 1;
}
extern "C" int fhesi_host_alloc(fhesi_ctx* c, size_t bytes, void** out) {
  CHECK_CTX(c);
  if (!out) FHESI_FAIL("host_alloc: null output pointer");
  if (hipHostMalloc(out, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; FHESI_FAIL("host_alloc: %zu pinned bytes not available", bytes); }
  return 0;
}
// (the context is NOT dereferenced: pinned allocations are not counted in live_handles, so a caller -- or a garbage collector -- may free
// them after fhesi_ctx_destroy; hipHostFree needs no current device)
extern "C" int fhesi_host_free(fhesi_ctx* /*ctx: unused, may be null or already destroyed*/, void* p) {
  if (p) HIP_TRY(hipHostFree(p));
  return 0;
}
// the staging ring of fhesi_ct_mul_relin_batch (two slots of pinned + device memory for three operands, ~1.5 GiB of each at the stress
// ring) is kept between calls; a caller that is done with host-buffer batches hands it back here (the next call allocates it again)
extern "C" int fhesi_host_stage_release(fhesi_ctx* c) {
  CHECK_CTX(c);
  if (c->host_stage) { HIP_TRY(hipStreamSynchronize(c->stream)); host_stage_free(c); }
  return 0;
}

extern "C" int fhesi_ct_mul_relin_batch(fhesi_ctx* c, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* a,
                                        const uint64_t* b, uint64_t* out, int32_t nlimbs, int64_t count) {
  CHECK_CTX(c);
  if (!count) return 0;
  if (!a || !b || !out) FHESI_FAIL("ct_mul_relin: null host buffer");
  const size_t ct_bytes = (size_t)2 * c->phim * nlimbs * 8;
  // stage size: the whole batch in at least two stages (so that transfers and compute overlap), at most 32 ciphertexts (64 MiB per operand
  // at the metric ring; larger stages only lengthen the pipeline's fill and drain)
  // (measured at the metric ring, profiles/r04_host_buffers.txt: 1024 per call 7.9 / 9.6 / 9.7 / 10.6 k mults/s with stages of 8 / 16 / 32
  // ciphertexts and 4 - 8 copy threads, 7.7 k with 128; 64 per call 8.5 k with stages of 16, 7.6 k with 32; 8 per call 5.1 k with two stages of 4)
  i64 hc = c->opt.host_chunk > 0 ? c->opt.host_chunk : (count >= 256 ? 32 : (count >= 32 ? 16 : std::max<i64>(1, (count + 1) / 2)));
  if (hc > count) hc = count;
  const size_t total_bytes = (size_t)count * ct_bytes;
  const int ka = host_ptr_kind(a, total_bytes), kb = host_ptr_kind(b, total_bytes), ko = host_ptr_kind(out, total_bytes);
  if (ka == 2 || kb == 2 || ko == 2) FHESI_FAIL("ct_mul_relin_batch takes HOST buffers (operand %s is device memory): use fhesi_ct_mul_relin_batch_dev", ka == 2 ? "a" : kb == 2 ? "b" : "out");
  const bool pa = ka == 1, pb = kb == 1, po = ko == 1;
  HostStage* h;
  FHESI_TRY(host_stage_get(c, (size_t)hc * ct_bytes, &h));
  const i64 nst = (count + hc - 1) / hc;
  // inside a stage the pageable side moves in pieces: the copy threads fill piece j + 1 of the ring while the DMA engine takes piece j up,
  // and on the way back they empty piece j while piece j + 1 comes down (one event per piece)
  const size_t piece = (size_t)8 << 20;
  const size_t npc_max = ((size_t)hc * ct_bytes + piece - 1) / piece;
  for (int s = 0; s < HostStage::NS; ++s)
    while (h->ev_piece[s].size() < npc_max) { hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ev_piece[s].push_back(e); }
  int rc = 0;
  auto upload = [&](int s, int which, const void* src, bool pinned, size_t bytes) -> bool {
    if (pinned) return hipMemcpyAsync(h->dev[s][which], src, bytes, hipMemcpyHostToDevice, h->up) == hipSuccess;
    for (size_t o = 0; o < bytes; o += piece) {
      const size_t len = std::min(piece, bytes - o);
      h->copy((char*)h->pin[s][which] + o, (const char*)src + o, len);
      if (hipMemcpyAsync((char*)h->dev[s][which] + o, (char*)h->pin[s][which] + o, len, hipMemcpyHostToDevice, h->up) != hipSuccess) return false;
    }
    return true;
  };
  auto finish = [&](i64 st) -> int {            // stage st: as its pieces arrive, hand them to the caller's buffer
    const int s = (int)(st % HostStage::NS);
    const size_t bytes = (size_t)std::min(hc, count - st * hc) * ct_bytes, off = (size_t)st * hc * ct_bytes;
    if (po) { if (hipEventSynchronize(h->ev_down[s]) != hipSuccess) { fhesi_set_error("download of ciphertext batch failed"); return 1; } return 0; }
    size_t j = 0;
    for (size_t o = 0; o < bytes; o += piece, ++j) {
      if (hipEventSynchronize(h->ev_piece[s][j]) != hipSuccess) { fhesi_set_error("download of ciphertext batch failed"); return 1; }
      h->copy((char*)out + off + o, (char*)h->pin[s][2] + o, std::min(piece, bytes - o));
    }
    return 0;
  };
  for (i64 st = 0; st < nst && !rc; ++st) {
    const int s = (int)(st % HostStage::NS);
    const i64 cnt = std::min(hc, count - st * hc);
    const size_t bytes = (size_t)cnt * ct_bytes, off = (size_t)st * hc * ct_bytes;
    // the slot's previous user (stage st - 2) was finished before stage st - 1 was issued: its pinned and device buffers are free
    if (!upload(s, 0, (const char*)a + off, pa, bytes) || !upload(s, 1, (const char*)b + off, pb, bytes) ||
        hipEventRecord(h->ev_up[s], h->up) != hipSuccess || hipStreamWaitEvent(c->stream, h->ev_up[s], 0) != hipSuccess) { fhesi_set_error("upload of ciphertext batch failed"); rc = 1; break; }
    rc = fhesi_ct_mul_relin_batch_dev(c, k, logQ, p, decomp_bytes, (const u64*)h->dev[s][0], (const u64*)h->dev[s][1], (u64*)h->dev[s][2], nlimbs, cnt);
    if (rc) break;
    bool ok = hipEventRecord(h->ev_comp[s], c->stream) == hipSuccess && hipStreamWaitEvent(h->down, h->ev_comp[s], 0) == hipSuccess;
    if (ok && po) ok = hipMemcpyAsync((char*)out + off, h->dev[s][2], bytes, hipMemcpyDeviceToHost, h->down) == hipSuccess;
    else if (ok) {
      size_t j = 0;
      for (size_t o = 0; ok && o < bytes; o += piece, ++j)
        ok = hipMemcpyAsync((char*)h->pin[s][2] + o, (char*)h->dev[s][2] + o, std::min(piece, bytes - o), hipMemcpyDeviceToHost, h->down) == hipSuccess &&
             hipEventRecord(h->ev_piece[s][j], h->down) == hipSuccess;
    }
    if (!ok || hipEventRecord(h->ev_down[s], h->down) != hipSuccess) { fhesi_set_error("download of ciphertext batch failed"); rc = 1; break; }
    if (st >= 1) rc = finish(st - 1);              // (overlaps stage st on the device; frees the other slot for stage st + 1)
  }
  if (!rc) rc = finish(nst - 1);
  if (rc) { hipStreamSynchronize(h->up); hipStreamSynchronize(c->stream); hipStreamSynchronize(h->down); }
  return rc;
}
