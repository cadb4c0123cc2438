/* fhesi_hip.h -- C ABI of the MI355X (gfx950) DoubleCRT backend for fhe-si.
 *
 * The reference (dwu4/fhe-si) has no FFI: its hot path is the C++ class graph
 *   Ciphertext / KeySwitchSI  ->  DoubleCRT methods  ->  Cmodulus::FFT / iFFT  ->  BluesteinFFT  ->  NTL fftRep.
 * This header is the seam a maintainer binds the *bodies* of those methods to (INTEGRATION.md shows the
 * binding); every entry point names the reference interface it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - plain C, no C++/torch/NTL types; all functions return 0 on success, non-zero on error
 *     (fhesi_last_error() gives the message).  The reference aborts through NTL Error()/assert
 *     (e.g. DoubleCRT.cpp:83,316,443; FHEContext.cpp:34): the C++ mirror turns a non-zero status
 *     into the same abort-style Error(msg).  No exception crosses this boundary.
 *   - residue rows: uint64_t[phi(m)], canonical values in [0,q_i), Z_m^* ascending order
 *     (the reference's vec_long rows, CModulus.cpp:103-106).
 *   - big integers: little-endian 64-bit limbs, two's complement, fixed nlimbs per call,
 *     coefficient-major [ncoeffs][nlimbs] (the reference's ZZX coefficients).
 *   - "host" pointers are ordinary memory; "_dev" entry points take device (HBM) pointers that
 *     must belong to the context's device.  Work is enqueued on the context's HIP stream;
 *     functions that return data to the host synchronise that stream.
 *   - one host thread per context; contexts are independent (one per GPU in the multi-GPU model).
 */
#ifndef FHESI_HIP_H_
#define FHESI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fhesi_ctx fhesi_ctx;     /* FHEcontext + vector<Cmodulus> + PAlgebra (FHEContext.h, CModulus.h, PAlgebra.h) */
typedef struct fhesi_dcrt fhesi_dcrt;   /* one DoubleCRT object (DoubleCRT.h:83-365), rows resident in HBM */
typedef struct fhesi_ksk fhesi_ksk;     /* one KeySwitchSI matrix (FHE-SI.cpp:206-208), resident in HBM */
typedef struct fhesi_slots fhesi_slots; /* one PlaintextSpace (PlaintextSpace.h): slot <-> root tables and chirps of the DFT modulo the plaintext prime */
typedef struct fhesi_plain fhesi_plain; /* nw prepared plaintext operands: DoubleCRT rows over the whole chain, resident in HBM */
typedef struct fhesi_comm fhesi_comm;   /* one rank of a multi-GPU group: an RCCL communicator (ncclComm_t) over xGMI */

enum { FHESI_OP_ADD = 0, FHESI_OP_SUB = 1, FHESI_OP_MUL = 2, FHESI_OP_DIV = 3, FHESI_OP_SET = 4 };

const char* fhesi_last_error(void);
int fhesi_device_count(int32_t* count);
/* ABI revision of this header.  It changes whenever an existing entry point changes its parameters (revision 5:
 * fhesi_keyswitch_init_batch_seeded took its public_seed argument in round 4; revision 6 adds this query and
 * fhesi_host_stage_release; revision 8 adds fhesi_ctx_lin_class; revision 9 adds the prepared plaintext operands, fhesi_plain_*).  A binding compiled or written against another revision must refuse to run: the Python binding
 * (fhe-si_amd/binding.py) and the C++ mirror (fhe-si_amd/host/fhesi_context.h) compare FHESI_ABI_VERSION with the library's
 * answer when they load it -- a stale ctypes table or mirror would otherwise link and silently shift arguments. */
#define FHESI_ABI_VERSION 9
int32_t fhesi_abi_version(void);

/* ---- context: FHEcontext::AddPrime (FHEContext.cpp:30-43) + Cmod::privateInit (CModulus.cpp:60-86) +
 * PAlgebra::init (PAlgebra.cpp:40-56).  Tables (twiddles / Bluestein powers and Rb) are built eagerly and
 * uploaded once (the reference fills them lazily: bluestein.cpp:103,121).  Rejects q not prime, q != 1 mod 2m,
 * duplicate q (FHEContext.cpp:34), m outside [2, 2^20] (FHEContext.cpp:89), or root not a primitive 2m-th root.
 * root[i] must be supplied (the reference draws a random one when 0, NumbTh.cpp:101-115; the C++ mirror does
 * that search on the host and passes the result here so row values are reproducible). */
int fhesi_ctx_create(fhesi_ctx** out, int64_t m, int32_t nprimes, const uint64_t* q, const uint64_t* root, int32_t device);
int fhesi_ctx_destroy(fhesi_ctx* ctx);
int64_t fhesi_ctx_m(const fhesi_ctx* ctx);
int64_t fhesi_ctx_phim(const fhesi_ctx* ctx);               /* PAlgebra::phiM (PAlgebra.h:78) */
int32_t fhesi_ctx_nprimes(const fhesi_ctx* ctx);            /* FHEcontext::numPrimes (FHEContext.h:149) */
int fhesi_ctx_prime(const fhesi_ctx* ctx, int32_t i, uint64_t* q, uint64_t* root);   /* ithPrime / getRoot */
int fhesi_ctx_zms_idx(const fhesi_ctx* ctx, int32_t* out_m);                        /* PAlgebra::indexInZmstar table */
int fhesi_ctx_phi_m(const fhesi_ctx* ctx, int64_t* out_phim_plus_1);                /* PAlgebra::PhimX coefficients */
/* Which class of ring the fused 30-bit paths took (read-only).  Phi_m as PAlgebra::init builds it (PAlgebra.cpp:40-56) is a three-term fold
 * exactly for m = Q or 2Q with Q = q^k, q an odd prime: Phi_m(X) = Phi_q(+-X^s), s = q^(k-1).  On those rings the integer products run as linear
 * convolutions on zero-padded rows of 2^lin_lg points (14 .. 20, from 2 phi(m) - 1 <= 2^lin_lg) and are folded with offset = Q (m = 2Q) or m (m odd)
 * and stride = s (1 for a prime or 2 x prime m).  offset = stride = lin_lg = 0: a power of two (negacyclic rows) or any other m (per-prime
 * Bluestein rows).  ctx != NULL: what that context took (m is ignored); ctx == NULL: what a context on m would take -- no device is touched. */
int fhesi_ctx_lin_class(const fhesi_ctx* ctx, int64_t m, int64_t* offset, int64_t* stride, int32_t* lin_lg);
int fhesi_ctx_sync(fhesi_ctx* ctx);
void* fhesi_ctx_stream(fhesi_ctx* ctx);                     /* the hipStream_t all work of this context runs on */
/* Behaviour switches of one context (A/B measurements, test hooks).  Names: "ks_direct" (1 = per-chain-prime key-switch dot product, the
 * reference's own structure FHE-SI.cpp:251-254), "ks_residues", "ks_aux60", "crt_exact", "crt_skip_cleanup" (test hook), "lanes" (2 = two
 * concurrent half-batches), "stagger", "batch_chunk", "wave_operands", "stage_chunk_bytes" (test hook: the chunk of channel pairs
 * while fhesi_conv2d_create stages its plaintexts), "tensor32" (0 = the fused pipeline keeps the tensor product on the
 * chain primes), "tensor_bits" (30 / 29: the size of the tensor half's primes -- below 2^29 the row transforms skip half of their range steps
 * for one or two primes more; the integers formed are the same); layout switches that never change a result (round 5): "dot32_k4" (0 = the digit-tile dot product dot32_kernel2 where the
 * key-in-LDS form dot32_kernel4 would run), "parts_words" (0 = 64-bit limb rows between the tensor half and the digit loader),
 * "ks_long_keys", "host_chunk", "host_threads"; "hoist_dot" (the dot product of fhesi_ct_rotations_dev: 1 = one launch per matrix of what a plain key
 * switch would run, 2 = the multi-matrix kernel, refused where the form is not the four-prime limb form, 0 = automatic; never changes a result).
 * The FHESI_<NAME> environment variables give the initial values, read once in fhesi_ctx_create -- never per call.  FHESI_LIN_LG (also read
 * there; a test hook) asks for LONGER zero-padded rows than a linear-convolution ring needs (15 .. 20: the fused loaders of rows of 2^15 / 2^16 and
 * the paths of rings with safe primes beyond 65 537, on rings small enough for an oracle).  FHESI_WS_POISON=1 (also a test hook) fills every
 * workspace reservation with 0xA5 bytes before use: results must not depend on what a workspace held.  FHESI_PHI_CONV=1 (test hook) makes
 * the reduction modulo Phi_m of a generic m (not a power of two, a prime or twice a prime) run as two convolutions at any size; above
 * m = 16384 that is the only form.
 * fhesi_ctx_destroy fails while DoubleCRT / key-switch handles of the context are alive (they hold the reference's `const FHEcontext&`). */
int fhesi_ctx_set_option(fhesi_ctx* ctx, const char* name, int64_t value);
int fhesi_ctx_get_option(const fhesi_ctx* ctx, const char* name, int64_t* value);
int fhesi_ctx_copy_options(fhesi_ctx* dst, const fhesi_ctx* src);      /* every switch of src onto dst: the per-GPU replicas of one FHEcontext run the same forms */
/* HIP-event stopwatch on the context's stream (bench.py's per-kernel timing) */
int fhesi_timer_start(fhesi_ctx* ctx);
int fhesi_timer_stop(fhesi_ctx* ctx, float* elapsed_ms);

/* per-kernel-class stopwatch: while enabled every launch of a class is bracketed by a HIP-event pair on the context's
 * stream; read returns (#launches, units processed -- rows for the NTT classes, polynomials/ciphertexts otherwise --, total ms) */
enum { FHESI_PROF_NTT_FWD = 0, FHESI_PROF_NTT_INV = 1, FHESI_PROF_RNS = 2, FHESI_PROF_TENSOR = 3, FHESI_PROF_CRT = 4,
       FHESI_PROF_DIGITS = 5, FHESI_PROF_DOT = 6, FHESI_PROF_EW = 7,
       FHESI_PROF_NTT_FWD_DIGITS_MAIN = 8 /* the fused ByteDecomp + forward-NTT tile kernel alone; units = rows it transformed */,
       FHESI_PROF_PLAIN_SUM = 15 /* plain_sum_kernel of fhesi_ct_plain_sum_dev; units = terms.  Numbered behind the name-only records below,
                                    which keep the numbers revision 8 gave them; 14 stays unassigned */ };
int fhesi_prof_enable(fhesi_ctx* ctx, int32_t on);      /* also clears the records */
int fhesi_prof_read(fhesi_ctx* ctx, int32_t kernel_class, int64_t* launches, double* units, double* total_ms);
/* demangled name (as rocprofv3 prints it, without the argument list) of the kernel the most recent profiled launch of that class ran:
 * the roofline line of bench.py names kernels by what the library launched, not by string literals.
 * The classes from FHESI_PROF_NAME_CRT_EXACT on carry a name only (no stopwatch: fhesi_prof_read refuses them): which closing kernel of the
 * big-integer conversions the last profiled launch ran -- the exact mixed-radix CRT (on its own or as the sum form's clean-up; FHESI_PROF_CRT
 * keeps naming crt_sum_kernel / crt32_scale*), the key-switch recombination, the RNS reduction of coefficients wider than 20 limbs, the
 * modulus switch and the plain digit rows.  The dispatch tests pin every branch of those launchers by these names. */
enum { FHESI_PROF_NAME_CRT_EXACT = 9, FHESI_PROF_NAME_KS_RECOMBINE = 10, FHESI_PROF_NAME_RNS_GENERIC = 11, FHESI_PROF_NAME_MODSWITCH = 12,
       FHESI_PROF_NAME_DIGITS = 13 };
int fhesi_prof_kernel_name(fhesi_ctx* ctx, int32_t kernel_class, char* name_out, size_t name_cap);

/* ---- Cmodulus::FFT / iFFT, one row (CModulus.h:165-166; CModulus.cpp:90-107, 110-132) */
int fhesi_cmod_fft(fhesi_ctx* ctx, int32_t prime, const uint64_t* coeff_limbs, int32_t nlimbs, int64_t ncoeffs, uint64_t* y_out);
int fhesi_cmod_ifft(fhesi_ctx* ctx, int32_t prime, const uint64_t* y, uint64_t* x_out /* phi(m) values in [0,q) */);

/* ---- DoubleCRT objects (DoubleCRT.h:83-365).  prime_idx = ascending index set; nidx==0 means ctxtPrimes = all
 * (DoubleCRT.cpp:244-250).  A new object holds the zero polynomial (DoubleCRT.cpp:261-311). */
int fhesi_dcrt_alloc(fhesi_ctx* ctx, const int32_t* prime_idx, int32_t nidx, fhesi_dcrt** out);
int fhesi_dcrt_free(fhesi_dcrt* d);
int fhesi_dcrt_copy(fhesi_dcrt* dst, const fhesi_dcrt* src);        /* operator=(DoubleCRT) DoubleCRT.cpp:313-320: error if contexts differ */
int fhesi_dcrt_index_set(const fhesi_dcrt* d, int32_t* idx_out, int32_t* nidx);   /* getIndexSet (DoubleCRT.h:303) */
int fhesi_dcrt_equal(const fhesi_dcrt* a, const fhesi_dcrt* b, int32_t* equal);  /* operator== (DoubleCRT.h:167-169) */
int fhesi_dcrt_upload_row(fhesi_dcrt* d, int32_t prime, const uint64_t* row);      /* setMap / Import (Serialization.cpp:56-81) */
int fhesi_dcrt_download_row(const fhesi_dcrt* d, int32_t prime, uint64_t* row);    /* getMap / Export */
void* fhesi_dcrt_device_ptr(fhesi_dcrt* d);                                          /* [nidx][phi(m)] uint64 in HBM */
int fhesi_dcrt_from_poly(fhesi_dcrt* d, const uint64_t* coeff_limbs, int32_t nlimbs, int64_t ncoeffs);   /* DoubleCRT(const ZZX&) / operator=(ZZX): DoubleCRT.cpp:212-257,323-331 */
int fhesi_dcrt_to_poly(const fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx, int32_t positive,
                       uint64_t* coeff_limbs_out, int32_t nlimbs);                   /* toPoly: DoubleCRT.cpp:349-404 (+ intVecCRT NumbTh.cpp:307-335) */
int fhesi_dcrt_op(fhesi_dcrt* dst, const fhesi_dcrt* src, int32_t op);              /* Op(DoubleCRT): DoubleCRT.cpp:79-113 (equal index sets; ADD/SUB/MUL) */
int fhesi_dcrt_op_scalar(fhesi_dcrt* d, const uint64_t* num_limbs, int32_t nlimbs, int32_t op);
                                                                                     /* Op(ZZ) :115-129, operator/= :407-420, operator=(ZZ) :333-347 */
int fhesi_dcrt_exp(fhesi_dcrt* d, int64_t e);                                       /* Exp: DoubleCRT.cpp:423-434 (PowerMod per element; e < 0 needs every element invertible) */
int fhesi_dcrt_automorph(fhesi_dcrt* d, int64_t k);                                 /* automorph: DoubleCRT.cpp:439-465; error if k not in Zm* */
int fhesi_dcrt_add_primes(fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx);   /* addPrimes: DoubleCRT.cpp:142-156 */
int fhesi_dcrt_remove_primes(fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx);/* removePrimes: DoubleCRT.h:197-199 */
/* BGV-style modulus switching (no caller inside fhe-si, part of the DoubleCRT surface); p = FHEcontext::ModulusP().
 * addPrimesAndScale (DoubleCRT.cpp:162-208): existing rows *= F (F^-1 mod p), F = product of the added primes; the added rows are zero;
 *   *log_factor_out (may be null) = log F + log(F^-1 mod p), the method's return value.  Errors: sets not disjoint, F not invertible mod p.
 * scaleDownToSet (DoubleCRT.cpp:518-558): drop the primes outside `prime_idx`, dividing by their product D with the correction term
 *   delta (D (D^-1 mod p) - 1) reduced modulo D p.  Errors mirror the asserts of :525-526 (empty intersection, nothing to drop). */
int fhesi_dcrt_add_primes_and_scale(fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx, uint64_t p, double* log_factor_out);
int fhesi_dcrt_scale_down_to_set(fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx, uint64_t p);
/* SingleCRT <-> DoubleCRT (DoubleCRT.cpp:484-515): coefficient-domain residues per prime, [nidx][phi(m)] */
int fhesi_dcrt_from_scrt(fhesi_dcrt* d, const uint64_t* coeff_rows);
int fhesi_dcrt_to_scrt(const fhesi_dcrt* d, uint64_t* coeff_rows_out);

/* ---- SingleCRT (SingleCRT.h:41-175, SingleCRT.cpp): the coefficient-domain RNS form -- for every prime of the index set the
 * polynomial's phi(m) coefficients modulo that prime.  It shares the DoubleCRT handle type and row storage; a handle made by
 * fhesi_scrt_alloc holds coefficient residues, and calls of the other family on it fail.  Shared entry points: fhesi_dcrt_free,
 * fhesi_dcrt_copy (operator=, SingleCRT.cpp:219-228), fhesi_dcrt_index_set, fhesi_dcrt_equal (SingleCRT.h:98-100),
 * fhesi_dcrt_upload_row / download_row (getMap), fhesi_dcrt_op with ADD / SUB (Op(SingleCRT, AddMod / SubMod), SingleCRT.cpp:61-103),
 * fhesi_dcrt_remove_primes (SingleCRT.h:117-119). */
int fhesi_scrt_alloc(fhesi_ctx* ctx, const int32_t* prime_idx, int32_t nidx, fhesi_dcrt** out);     /* SingleCRT(context, s): zero polynomial (SingleCRT.cpp:188-203) */
int fhesi_scrt_from_poly(fhesi_dcrt* s, const uint64_t* coeff_limbs, int32_t nlimbs, int64_t ncoeffs);   /* operator=(ZZX): PolyRed(poly, p_i, abs=true) per prime
                                                                                        (SingleCRT.cpp:239-251, NumbTh.cpp:210-233); ncoeffs <= phi(m) */
int fhesi_scrt_to_poly(const fhesi_dcrt* s, const int32_t* prime_idx, int32_t nidx, uint64_t* coeff_limbs_out, int32_t nlimbs);
                                                                                     /* toPoly (SingleCRT.cpp:299-334): centred CRT over (index set & s) */
int fhesi_scrt_op_scalar(fhesi_dcrt* s, const uint64_t* num_limbs, int32_t nlimbs, int32_t op);
                                                                                     /* Op(ZZ, add / sub / mul) (SingleCRT.cpp:137-153) and operator/= (:279-296):
                                                                                        ADD / SUB change the constant coefficient only (NTL add(ZZX, ZZX, ZZ)) */
int fhesi_dcrt_assign_scrt(fhesi_dcrt* d, const fhesi_dcrt* s);                      /* DoubleCRT::operator=(SingleCRT): DoubleCRT.cpp:484-496, in HBM */
int fhesi_scrt_assign_dcrt(fhesi_dcrt* s, const fhesi_dcrt* d, const int32_t* prime_idx, int32_t nidx);
                                                                                     /* DoubleCRT::toSingleCRT(scrt, s) / SingleCRT::operator=(DoubleCRT):
                                                                                        DoubleCRT.cpp:498-515, SingleCRT.cpp:231-235; nidx = 0 and null = all */

/* ---- batched device-resident row kernels.  rows_dev: [count][L][phi(m)] uint64 in HBM, all L primes */
int fhesi_rows_ntt_fwd_dev(fhesi_ctx* ctx, uint64_t* rows_dev, int64_t count);      /* coefficient residues -> evaluations, in place (Cmod::FFT after conv) */
int fhesi_rows_ntt_inv_dev(fhesi_ctx* ctx, uint64_t* rows_dev, int64_t count);      /* evaluations -> coefficient residues, in place (Cmod::iFFT) */
int fhesi_rows_op_dev(fhesi_ctx* ctx, uint64_t* dst_dev, const uint64_t* src_dev, int64_t count, int32_t op);   /* DoubleCRT::Op over a batch */

/* ---- key-switch matrix (KeySwitchSI::keySwitchMatrix, FHE-SI.cpp:206-208): [2][ncomp*ndigits][L][phi(m)],
 * matrix[0]=b, matrix[1]=A, column i*ndigits+j (FHE-SI.cpp:176-177) */
int fhesi_ksk_create(fhesi_ctx* ctx, int32_t ncomp, int32_t ndigits, fhesi_ksk** out);
int fhesi_ksk_free(fhesi_ksk* k);
int fhesi_ksk_upload(fhesi_ksk* k, const uint64_t* rows_host);                       /* whole matrix, host layout as above */
void* fhesi_ksk_device_ptr(fhesi_ksk* k);                                            /* HBM buffer of the rows (pure getter) */
int fhesi_ksk_mark_dirty(fhesi_ksk* k);                                              /* call after writing the rows through the pointer (a collective that
                                                                                        received into them): the library keeps tables derived from the rows
                                                                                        and rebuilds them at the next key switch */
int fhesi_ksk_upload_dev(fhesi_ksk* k, const uint64_t* rows_dev);                    /* whole matrix from another HBM buffer (copies and invalidates) */
size_t fhesi_ksk_bytes(const fhesi_ksk* k);
/* Which form of KeySwitchSI::ApplyKeySwitch's dot product (Util.h:79-98 at FHE-SI.cpp:251-254) the last key switch with this matrix ran:
 * form 0 = one dot product per chain prime (the reference's own structure), 1 = exact integer dot product over four 30-bit auxiliary
 * primes in limb mode, 2 = over the two largest chain primes in limb mode, 3 = over them in residue mode; rows = limbs (or residues) per
 * key coefficient, limb_bits = their width (0 in residue mode).  All forms give the reference's bits; a caller (bench, tests) reads this to
 * state which one it measured.  Before the first key switch: form -1. */
int fhesi_ksk_form(const fhesi_ksk* k, int32_t* form, int32_t* rows, int32_t* limb_bits);
/* Form 1 looks at the matrix it is given: KeySwitchSI::Init (FHE-SI.cpp:176-204) samples its polynomial modulo 2^logQ and reduces b modulo
 * 2^logQ, so the integer coefficients of a generated matrix lie in [-2^(logQ-1), 2^(logQ-1)] -- less than half the bits of the chain
 * product.  The library measures the coefficients when it builds its table; when they are that small it cuts the limbs from the CENTRED
 * integers (7 instead of 15 at the metric ring; `rows` above says how many) and the dot product needs no reduction modulo the chain product.
 * Any other matrix (uniform residues, say) takes the general limbs.  centred: 1 if the last table was built that way; key_bits: the measured
 * nb with every coefficient in [-2^nb, 2^nb] (0 if the table was not measured).  Option "ks_long_keys" = 1 forces the general limbs. */
int fhesi_ksk_key_bits(const fhesi_ksk* k, int32_t* centred, int32_t* key_bits);

int fhesi_selftest_aux32(fhesi_ctx* c);                                              /* diagnostic: checks the 32-bit auxiliary transforms of the key switch
                                                                                        (n = 2^14 only) as a ring isomorphism; 0 = ok */

/* ---- the metric's unit of work, batched: Ciphertext::operator*= (Ciphertext.cpp:167-192) followed by
 * KeySwitchSI::ApplyKeySwitch (FHE-SI.cpp:241-260) = ScaleDown (Ciphertext.cpp:194-218) + ByteDecomp (:82-121)
 * + DotProduct (Util.h:79-98) + toPoly + ReduceCoefficients (Util.cpp:3-33).
 * a, b: [count][2][phi(m)][nlimbs] two's complement coefficients mod 2^logQ (centered); out: same shape.
 * nlimbs must be >= ceil(logQ/64).  decomp_bytes = FHEcontext::decompSize (3 at every reference call site). */
int fhesi_ct_mul_relin_batch(fhesi_ctx* ctx, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes,
                             const uint64_t* a_host, const uint64_t* b_host, uint64_t* out_host, int32_t nlimbs, int64_t count);
/* The host-buffer form runs as a pipeline of stages over a pinned staging ring: upload of stage i + 1, compute of stage i and download of
 * stage i - 1 overlap on three streams, and pageable buffers are copied into / out of the ring by several threads (options "host_chunk":
 * ciphertexts per stage, "host_threads").  Buffers allocated with fhesi_host_alloc (pinned) are read and written by the DMA engines
 * directly, without the copy (only when the WHOLE batch lies in pinned / registered memory; a partly registered range is treated as
 * pageable).  Device or managed pointers are rejected with an error: this entry takes host memory, the _dev form device memory.
 * Same bits as the _dev form. */
int fhesi_host_alloc(fhesi_ctx* ctx, size_t bytes, void** out);                      /* pinned host memory for ciphertext batches */
int fhesi_host_free(fhesi_ctx* ctx, void* p);                                        /* ctx is not dereferenced (may be null or already destroyed) */
int fhesi_host_stage_release(fhesi_ctx* ctx);                                        /* frees the pinned + device staging ring kept between host-buffer calls */
int fhesi_ct_mul_relin_batch_dev(fhesi_ctx* ctx, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes,
                                 const uint64_t* a_dev, const uint64_t* b_dev, uint64_t* out_dev, int32_t nlimbs, int64_t count);
/* Separately callable stages of the same pipeline (parity tests check each against the oracle) */
int fhesi_ct_mul_dev(fhesi_ctx* ctx, uint64_t p, const uint64_t* a_dev, const uint64_t* b_dev, int32_t nlimbs, int64_t count,
                     uint64_t* tprod_dev /* [count][3][L][phi(m)] */);              /* Ciphertext::operator*= */
int fhesi_apply_key_switch_dev(fhesi_ctx* ctx, const fhesi_ksk* k, int32_t logQ, int32_t decomp_bytes,
                               const uint64_t* tprod_dev, int64_t count, uint64_t* out_dev, int32_t nlimbs);   /* ApplyKeySwitch */

/* ---- ciphertext algebra between multiplications, on batches resident in HBM: what Matrix<Ciphertext> (Matrix.cpp:57-98,
 * 150-174,182-263) and Regression::Regress / SumBatchedData (Regression.h:102-149,166-178) call on Ciphertext objects.
 * Unscaled ciphertexts: [count][nparts][phi(m)][nlimbs] two's complement; scaled-up ones (tProd): [count][3][L][phi(m)] rows. */
int fhesi_ct_add_dev(fhesi_ctx* ctx, int32_t logQ, uint64_t* dst_dev, const uint64_t* src_dev, int32_t nparts, int32_t nlimbs, int64_t count);
                                                                                     /* Ciphertext::operator+= unscaled: Ciphertext.cpp:123-134 (scaled-up: fhesi_rows_op_dev) */
int fhesi_ct_add_const_dev(fhesi_ctx* ctx, int32_t logQ, uint64_t p, uint64_t* ct_dev, int32_t nparts, int32_t nlimbs, int64_t count,
                           const int64_t* poly_host /* [npoly][phi(m)] */, int32_t npoly /* 1 = the same constant for every ciphertext, or count */);
                                                                                     /* Ciphertext::operator+=(const ZZX&) unscaled: Ciphertext.cpp:147-156 -- part 0 += (other << logQ) / p
                                                                                        (floor), ReduceCoefficients; the scaled-up branch (:157-159) is DoubleCRT += ZZX = fhesi_dcrt_from_poly + fhesi_dcrt_op */
int fhesi_ct_mul_poly_dev(fhesi_ctx* ctx, int32_t logQ, uint64_t* ct_dev, int32_t nparts, int32_t nlimbs, int64_t count,
                          const int64_t* poly_host /* [npoly][phi(m)] */, int32_t npoly);
                                                                                     /* Ciphertext::operator*=(const ZZX&) unscaled: Ciphertext.cpp:245-249 -> CiphertextPart::operator*=(ZZX) :29-36
                                                                                        (integer product, rem Phi_m, Reduce); scaled-up (:250-254): tProd[i] *= DoubleCRT(other) = fhesi_dcrt_op */
int fhesi_ct_mul_long_dev(fhesi_ctx* ctx, int32_t logQ, uint64_t* ct_dev, int64_t l, int32_t nparts, int32_t nlimbs, int64_t count);
                                                                                     /* Ciphertext::operator*=(long) unscaled: Ciphertext.cpp:232-237 -> :21-27 */
int fhesi_rows_mul_long_dev(fhesi_ctx* ctx, uint64_t* rows_dev, int64_t l, int64_t count);   /* ... scaled-up: Ciphertext.cpp:238-241 (DoubleCRT *= long); count DoubleCRTs */
int fhesi_ct_automorph_dev(fhesi_ctx* ctx, int64_t k, const uint64_t* in_dev, int32_t nparts, int32_t nlimbs_in, int64_t count,
                           uint64_t* out_dev, int32_t nlimbs_out);                   /* Ciphertext::operator>>= unscaled: Ciphertext.cpp:264-269 -> :54-59; the result is
                                                                                        centred modulo the prime chain, not modulo 2^logQ; error if k not in Zm* */
/* (ctxt >>= k) followed by KeySwitchSI::ApplyKeySwitch with the matrix of KeySwitchSI(secretKey, k) (FHE-SI.cpp:229-260): one
 * step of Regression::SumBatchedData (Regression.h:170-172).  k = 1 applies the key switch to the unscaled ciphertext as it is.
 * in: [count][ncomp][phi(m)][nlimbs_in], ncomp = the matrix's source components; out: [count][2][phi(m)][nlimbs] */
int fhesi_ct_automorph_key_switch_dev(fhesi_ctx* ctx, const fhesi_ksk* k_matrix, int32_t logQ, int32_t decomp_bytes, int64_t k,
                                      const uint64_t* in_dev, int32_t nlimbs_in, int64_t count, uint64_t* out_dev, int32_t nlimbs);
/* out[i] = pool[idx[i]] for elements of `words` uint64 each (operands of one wave of products) */
int fhesi_ct_gather_dev(fhesi_ctx* ctx, const uint64_t* pool_dev, const int32_t* idx_host, int64_t count, int64_t words, uint64_t* out_dev);
/* One wave of Matrix<Ciphertext> arithmetic: for every group g
 *     out[g] = ApplyKeySwitch( sum_{t in [seg[g], seg[g+1])}  pool[a_idx[t]] *= pool[b_idx[t]] )
 * i.e. the inner loops of Matrix::operator*= (Matrix.cpp:57-79), MultByTranspose (:150-174) and Determinant (:227-263) -- products of
 * unscaled ciphertexts (Ciphertext.cpp:167-192) summed while scaled up (:135-142) -- followed by the `reduce` / MapAll key switch
 * (Regression.h:112-115,127-134).  pool: unscaled 2-part ciphertexts [npool][2][phi(m)][nlimbs]; a_idx, b_idx, seg: host arrays. */
int fhesi_ct_mul_sum_relin_dev(fhesi_ctx* ctx, const fhesi_ksk* k, int32_t logQ, uint64_t p, int32_t decomp_bytes, const uint64_t* pool_dev,
                               int32_t nlimbs, const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups, uint64_t* out_dev);

/* ---- Encrypt / Decrypt in batches.  The polynomial arithmetic runs on the device; the randomness stays the
 * caller's (the reference draws it from NTL's PRNG, FHE-SI.cpp:14-25), which keeps results reproducible bit for bit.
 * FHESIPubKey::Encrypt (FHE-SI.cpp:10-36): pk0, pk1 = publicKey[0..1] over all primes;
 *   rand_host [count][3][phi(m)] int64 = (r: binary polynomial, e0, e1: Gaussian samples BEFORE the multiplication by p);
 *   msg_host [count][phi(m)] int64 in [0,p) (coefficient form);  out_dev [count][2][phi(m)][nlimbs] centred mod 2^logQ. */
int fhesi_encrypt_batch(fhesi_ctx* ctx, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t p, const int64_t* rand_host,
                        const int64_t* msg_host, int64_t count, uint64_t* out_dev, int32_t nlimbs);
/* FHESISecKey::Decrypt (FHE-SI.cpp:93-119) of unscaled 2-part ciphertexts: sk1 = sKeys[1] (sKeys[0] = 1);
 *   msg_host [count][phi(m)] = round(p * (c0 + c1 t) / 2^logQ) mod p, floor((2 p z + q) / (2 q)) as in the reference. */
int fhesi_decrypt_batch(fhesi_ctx* ctx, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                        int64_t* msg_host);
/* The NOISE BUDGET of unscaled 2-part ciphertexts, for the holder of the secret key: how far each is from decrypting wrongly.  An extension of
 * the mirror (the reference only has the end-to-end predicate decrypt(f(enc x)) == f(x)).  With q = 2^logQ and z = c0 + c1 t as in Decrypt, per
 * coefficient P = (2 p z + q) mod 2q is the remainder Decrypt's rounding throws away and r = P - q in [-q, q) the decryption RESIDUAL (the
 * invariant noise is r / 2q in [-1/2, 1/2)).  Per ciphertext:
 *   maxres = max over the phi(m) coefficients of |r|, exact, nw = ceil((logQ + 1) / 64) little-endian 64-bit words;
 *   budget = max(0, logQ - bitlen(maxres)), bitlen(0) = 0: the noise may grow by a factor 2^budget and every coefficient still rounds to the
 *            same message (maxres 2^budget < q whenever budget > 0).
 * WHAT IS MEASURED.  The residual equals the true noise only while the true noise is below 1/2.  A ciphertext whose noise has passed 1/2 has
 * already rounded to a neighbouring message and shows the distance to THAT one, which may look small.  So budget 0 means "at or within one bit
 * of failure", a positive budget is meaningful for a ciphertext that was computed within its budget so far, and a budget that RISES along a
 * computation is the sign that it failed in between.  Nothing here estimates noise without the key.
 * One pass over z gives both results of fhesi_decrypt_noise_batch; its msg_host is fhesi_decrypt_batch's bit for bit.  Arguments and refusals are
 * those of fhesi_decrypt_batch; maxres_host may be null.  Deterministic: no atomics, the result does not depend on the launch shape. */
int fhesi_ct_noise_batch(fhesi_ctx* ctx, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                         int32_t* budget_host /* [count] */, uint64_t* maxres_host /* [count][nw] or null */);
int fhesi_decrypt_noise_batch(fhesi_ctx* ctx, const fhesi_dcrt* sk1, int32_t logQ, uint64_t p, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                              int64_t* msg_host, int32_t* budget_host /* [count] */, uint64_t* maxres_host /* [count][nw] or null */);

/* KeySwitchSI::Init (FHE-SI.cpp:153-209) for every column of a matrix in one call: k = the matrix (ncomp = components of the source
 * key: 3 for InitS2's (1, t, t^2), 2 for InitAutomorph), src[i] = the source key's DoubleCRT components, dst_t = dst[1].
 *   a_host   [ncomp*ndigits][phi(m)][nlimbs]  the SampleRandom polynomials (:174-175), centred modulo 2^logQ, column i*ndigits+j
 *   err_host [ncomp*ndigits][phi(m)] int64    the Gaussian errors (:189-190)
 * drawn by the caller in the reference's order (poly, err per column).  Result: k[1][col] = -DoubleCRT(a), k[0][col] =
 * DoubleCRT(Reduce(toPoly(a t) + err + (toPoly(s_i) << 8 decompSize j))), all transforms, products and conversions on the device. */
int fhesi_keyswitch_init_batch(fhesi_ksk* k, const fhesi_dcrt* const* src, int32_t nsrc, const fhesi_dcrt* dst_t, int32_t logQ, int32_t decomp_bytes,
                               const uint64_t* a_host, int32_t nlimbs, const int64_t* err_host);
int fhesi_ksk_download(const fhesi_ksk* k, uint64_t* rows_host);                         /* whole matrix to the host (Export, FHE-SI.cpp:270-272) */

/* ---- the same three with the randomness drawn ON THE DEVICE (sampleHWt / sampleGaussian NumbTh.cpp:340-404, the binary
 * and Gaussian polynomials of Encrypt FHE-SI.cpp:14-25, SampleRandom + sampleGaussian per key-switch column FHE-SI.cpp:174-190).  NTL's
 * sequential PRNG cannot be reproduced outside NTL, so these entry points use a counter-based generator instead -- Philox-4x32-10 keyed by
 * `seed`, counter = (coefficient, object index, purpose); definition in fhe-si_amd/csrc/philox.h, restated by the oracle and the Python
 * model -- which makes a ciphertext or a key a function of (seed, index) alone: the same on every GPU, in any batch split, and on the CPU.
 * The explicit-randomness forms above remain for callers that bring their own randomness (and for reproducing fixtures).
 *
 * WHAT THE CALLER OWES THESE ENTRY POINTS.  (1) Philox is a reproducible counter-based generator with a 64-bit key, NOT a CSPRNG: use it for
 * fixtures, tests and deployments whose threat model accepts that; key material that must withstand more takes the explicit-randomness
 * entry points with randomness from the caller's CSPRNG.  `seed` must in any case be secret, uniformly random 64 bits.  (2) An
 * (seed, object index) pair must never be used twice: two encryptions under the same pair share r, e0, e1, so their difference is
 * delta * (m1 - m2) in the clear; two key-switch columns under the same pair share a and the error.  There is no default index -- every call
 * names the first index of a range nobody else uses (the C++ mirror's SeedSequence hands out disjoint ranges from one counter shared by
 * Encrypt and every KeySwitchSI).  (3) The polynomials `a` of a key-switch matrix are public; they draw from `public_seed`, the errors from
 * `seed`: publishing public_seed (a matrix shipped as its seed) discloses nothing secret.  public_seed != seed. */
int fhesi_encrypt_batch_seeded(fhesi_ctx* ctx, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t p, uint64_t seed, uint64_t first_index,
                               const int64_t* msg_host, int64_t count, uint64_t* out_dev, int32_t nlimbs);      /* plaintext i <-> object index first_index + i */
int fhesi_keyswitch_init_batch_seeded(fhesi_ksk* k, const fhesi_dcrt* const* src, int32_t nsrc, const fhesi_dcrt* dst_t, int32_t logQ, int32_t decomp_bytes,
                                      uint64_t seed, uint64_t public_seed, uint64_t first_index);                /* column c <-> object index first_index + c; a from public_seed, errors from seed */
int fhesi_dcrt_sample(fhesi_dcrt* d, int32_t kind, int64_t param, uint64_t seed, uint64_t index);               /* DoubleCRT::sampleHWt(param) (kind 0), ::sampleGaussian() with
                                                                                                                    stdev 3.2 (kind 1): DoubleCRT.h:340-345 */

/* ---- plaintext slots: PlaintextSpace (PlaintextSpace.cpp:20-135) and the slot-valued forms of Plaintext, Encrypt, Decrypt and
 * Regression::GenerateNoise, batched on the device (fhe-si_amd/csrc/kernels_slots.hip).
 *
 * SCOPE.  plaintext modulus p PRIME, p < 2^32, p = 1 mod m (Phi_m splits into phi(m) linear factors: every slot is one element of Z_p), and the
 * generator g generates (Z/m)^* (PlaintextSpace.cpp:103 asserts that one generator walks all slots), which forces m in {2, 4, q^k, 2 q^k}, q an
 * odd prime.  That is every ring of Test_AddMul / Test_General / Test_Regression / Test_Statistics (m = p - 1).  Everything else -- ord_m(p) > 1
 * (slots in GF(p^d): e.g. m = 2^15, p = 23), non-cyclic (Z/m)^*, p >= 2^32, composite p, g not a generator -- is REFUSED by fhesi_slots_create /
 * fhesi_slots_plan on the host, before anything is launched, and fhesi_last_error names the failed condition.  Nothing is half-supported.
 *
 * SLOT ORDER.  Slot j sits on the root rho0^(e_j), e_j = g^j mod m, j = 0 .. phi(m)-1 (what FindSlots / ReorderSlots produce, :69-110, for
 * linear factors).  The reference's rho0 is whichever factor NTL's randomised factoriser returned first; here rho0 = the smallest integer in
 * [1, p) that is a primitive m-th root of unity modulo p.  Consequences that do not depend on rho0: Decode(Embed(v)) = v; Embed is linear;
 * products modulo (Phi_m, p) multiply slot by slot; the automorphism X -> X^(g^t) (Ciphertext >>= g^t, fhesi_ct_automorph_dev) moves slot j + t
 * into slot j -- a rotation LEFT by t, the direction of Plaintext::operator>>=(t) (Plaintext.h:87-96).
 * usable = 2^floor(log2 phi(m)) (:37-42).  only_usable != 0 (the reference's default): embed takes min(nvals, usable) values into slots
 * 0 .. , the other slots are 0; decode fills the first min(nvals, usable) of the nvals entries per plaintext and zeroes the rest.
 * only_usable = 0: the same with phi(m) in place of usable.  1 <= nvals <= phi(m).  Values may be any int64 (reduced modulo p); results lie in [0, p).
 * A slot space holds a pointer to its context and counts as one of its live handles (fhesi_ctx_destroy). */
int fhesi_slots_plan(int64_t m, uint64_t p, int64_t generator, int64_t* total, int64_t* usable, uint64_t* rho0, int32_t* aux_primes,
                     int32_t* e_out /* [phi(m)] or null */);                      /* the host half of PlaintextSpace::Init: checks and tables, no device, no context */
int fhesi_slots_create(fhesi_ctx* ctx, uint64_t p, int64_t generator, fhesi_slots** out);    /* PlaintextSpace::Init(PhiX, p, generator) :20-60 */
int fhesi_slots_free(fhesi_slots* s);
int fhesi_slots_info(const fhesi_slots* s, int64_t* total, int64_t* usable, uint64_t* rho0, int32_t* aux_primes_used);
                                                                                    /* GetTotalSlots / GetUsableSlots :62-68; aux_primes_used: 1 when m p^2 < 2^59, else 2 */
int fhesi_slots_exponents(const fhesi_slots* s, int32_t* e_out /* [phi(m)] */);    /* e_j: the root slot j sits on is rho0^(e_j) */
int fhesi_slots_embed(fhesi_slots* s, const int64_t* vals_host /* [count][nvals] */, int64_t nvals, int32_t only_usable, int64_t count,
                      int64_t* msg_host /* [count][phi(m)] */);                     /* EmbedInSlots :112-121, `count` plaintexts in one call */
int fhesi_slots_decode(fhesi_slots* s, const int64_t* msg_host /* [count][phi(m)] */, int64_t count, int64_t nvals, int32_t only_usable,
                       int64_t* vals_host /* [count][nvals] */);                    /* DecodeSlots / DecodeSlot :123-135 */
int fhesi_slots_embed_dev(fhesi_slots* s, const int64_t* vals_dev, int64_t nvals, int32_t only_usable, int64_t count, int64_t* msg_dev);
int fhesi_slots_decode_dev(fhesi_slots* s, const int64_t* msg_dev, int64_t count, int64_t nvals, int32_t only_usable, int64_t* vals_dev);
                                                                                    /* the same on HBM buffers: no copies, enqueued on the context's stream, not synchronised */
/* Plaintext(context, values) + FHESIPubKey::Encrypt (Regression.h:84-92) / FHESISecKey::Decrypt + Plaintext::DecodeSlots (Test_Regression.cpp:47-58)
 * with the message polynomials kept in HBM; p is the slot space's.  fhesi_encrypt_slots_batch_seeded(vals) equals
 * fhesi_encrypt_batch_seeded(fhesi_slots_embed(vals)) bit for bit under the same (seed, first_index).
 * fhesi_encrypt_noise_batch_seeded: Regression::GenerateNoise (Regression.h:180-191) for `count` masks -- slot 0 is 0, slot j >= 1 is
 * floor(u p / 2^64) for the 64-bit Philox draw u of (seed, first_index + i, j, purpose 7) (bias below p / 2^64 per value), all phi(m) slots embedded
 * (onlyUsable = false), then an ordinary encryption under the same (seed, first_index + i).  The warning block above (WHAT THE CALLER OWES THESE
 * ENTRY POINTS) applies unchanged: a mask hides the other slots only as well as Philox's 64-bit key allows, and an index is never used twice. */
int fhesi_encrypt_slots_batch_seeded(fhesi_ctx* ctx, fhesi_slots* s, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                     const int64_t* vals_host /* [count][nvals] */, int64_t nvals, int32_t only_usable, int64_t count, uint64_t* out_dev, int32_t nlimbs);
int fhesi_decrypt_slots_batch(fhesi_ctx* ctx, fhesi_slots* s, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev, int32_t nlimbs, int64_t count,
                              int64_t nvals, int32_t only_usable, int64_t* vals_host /* [count][nvals] */);
int fhesi_encrypt_noise_batch_seeded(fhesi_ctx* ctx, fhesi_slots* s, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                     int64_t count, uint64_t* out_dev, int32_t nlimbs);

/* ---- plaintext slots on the power-of-two rings: the TWO-ROW space (fhe-si_amd/csrc/kernels_slots_pow2.hip).  An extension of the mirror: the
 * reference's single-generator walk (PlaintextSpace.cpp:88-103) asserts on these rings, and fhesi_slots_create / fhesi_slots_plan keep refusing them.
 *
 * SCOPE.  m = 2^k with k >= 3, n = m / 2, h = n / 2; p PRIME, p < 2^32, p = 1 mod m (X^n + 1 splits into n linear factors); generator g = 3 or 5
 * mod 8 (g then has order h modulo m and -1 is not among its powers: (Z/m)^* = <-1> x <g>).  Everything else -- k < 3 (cyclic: the constructor
 * above), m not a power of two, p not prime, p >= 2^32, p != 1 mod m, another g -- is REFUSED on the host before anything is launched, the
 * message names the condition.
 *
 * SLOT ORDER.  rho0 = the least primitive m-th root of unity in [1, p), as above.  Slot s = r h + j (row r = 0, 1; column j = 0 .. h-1) sits on
 * rho0^(e_s), e_s = (-1)^r g^j mod m.  total = usable = n.  X -> X^(g^t) rotates BOTH rows left by t columns (the direction of
 * Plaintext::operator>>=), X -> X^(m-1) swaps the rows (fhesi_ct_automorph_key_switch_dev takes any k in Z_m^*).  The automorphisms g, g^2, g^4,
 * ..., g^(h/2), m - 1, each followed by an addition (log2 n steps), leave the sum of all n slots in EVERY slot.
 *
 * PATH.  0: n <= 2^15 and p < 2^31 -- one negacyclic transform of length n modulo p per plaintext (psi = rho0, no chirp, no auxiliary prime),
 * one workgroup per plaintext with the row in LDS.  1 / 2: otherwise the chirp of the single-generator spaces on the two-row exponent table,
 * with one / two auxiliary primes (m p^2 against 2^59).  Both compute the same words.
 *
 * The handle is a fhesi_slots: fhesi_slots_free / info / exponents / embed / decode / embed_dev / decode_dev, fhesi_encrypt_slots_batch_seeded,
 * fhesi_decrypt_slots_batch and fhesi_encrypt_noise_batch_seeded take it unchanged (only_usable makes no difference: usable = total). */
int fhesi_slots_plan_pow2(int64_t m, uint64_t p, int64_t generator, int64_t* total, int64_t* rows, int64_t* cols, uint64_t* rho0,
                          int32_t* path /* 0 direct, 1 chirp with one prime, 2 chirp with two */, int32_t* e_out /* [n] or null */);
int fhesi_slots_create_pow2(fhesi_ctx* ctx, uint64_t p, int64_t generator, fhesi_slots** out);
int fhesi_slots_shape(const fhesi_slots* s, int64_t* rows, int64_t* cols, int32_t* path);   /* (1, phi(m), aux primes) for the single-generator spaces */
int fhesi_slots_set_path(fhesi_slots* s, int32_t path);      /* two-row spaces: 0 = the direct transform (refused where the plan does not admit it), otherwise the chirp.
                                                                Result-neutral; for measurements and for comparing the two.  Synchronises the context's stream. */

/* ---- integer slots over a BASIS of plaintext primes on a two-row ring (fhe-si_amd/csrc/kernels_slots_basis.hip).  A residue modulo one
 * prime p < 2^32 is what a two-row space gives back; results of real data (det(X^T X) of thousands of rows) need hundreds of bits.  A slot
 * basis is k distinct primes p_c = 1 mod m on ONE ring, P = prod p_c: the computation runs once per prime ("channel") and the results are
 * recombined by the Chinese remainder theorem on the device.
 *
 * CONVENTION.  A slot holds an integer modulo P, given and returned as a SIGNED integer in (-P/2, P/2) (P is odd: no tie).  A logical
 * plaintext / ciphertext is k channel plaintexts / ciphertexts; channel c is the two-row space of (m, p_c, g) exactly as fhesi_slots_create_pow2
 * makes it (same rho0 rule per prime, same generator, same slot order s = r h + j), so every existing operation applies channel by channel with
 * that channel's p: products, sums, row rotations, the row swap, the total-sum walk, the noise masks.  Nothing on the device knows p until a
 * call passes it: ONE context and ONE key set (secret key, public key, key-switch matrices) serve every channel.  The chain of the context must
 * be sized for the LARGEST prime of the basis (every multiplication pays log2 p_c bits of logQ).
 *
 * VALUES travel as L little-endian 64-bit limbs in two's complement.  On output L = limbs = ceil((bitlen(P) + 1) / 64) <= 16.  On input any
 * L_in in 1 .. 16 is taken and reduced modulo each p_c (plain int64 data is L_in = 1).
 * CAPACITY.  The caller owes |result| < P / 2 for everything the computation produces; a result that wraps modulo P comes back as another
 * integer of (-P/2, P/2) and nothing on the device can detect it.  fhesi_slots_basis_plan sizes a basis for a bound of `bits` bits.
 *
 * SCOPE.  m = 2^k with 3 <= k <= 16 and every p_c < 2^31 (the direct transform, PATH 0 above), 1 <= k <= 32 primes, each prime, = 1 mod m, no
 * prime twice, g = 3 or 5 mod 8.  Everything else is REFUSED on the host before anything is launched, fhesi_last_error names the condition and
 * the context stays usable.
 *
 * INDEX RULE of the seeded forms.  A batch of `count` logical plaintexts uses the object indices first_index .. first_index + k count - 1:
 * channel c, plaintext i takes first_index + c count + i, so channel c of fhesi_encrypt_int_slots_batch_seeded equals
 * fhesi_encrypt_slots_batch_seeded(channel c's space, first_index + c count, vals mod p_c) BIT FOR BIT, and the caller advances by k count.
 * fhesi_encrypt_noise_int_batch_seeded draws k independent masks per logical mask under the same rule: slot 0 of every channel is 0, hence
 * slot 0 modulo P is untouched; the other slots are uniform modulo every p_c, hence modulo P.
 *
 * LAYOUTS.  vals [count][nvals][L] limbs; msg [k][count][n] int64 in [0, p_c) (what the encryption's message staging takes);
 * ciphertexts [k][count] of [2][n][nlimbs] words.  The _dev forms take HBM buffers, enqueue on the context's stream and do not synchronise. */
typedef struct fhesi_slots_basis fhesi_slots_basis;
int fhesi_slots_basis_plan(int64_t m, int32_t bits, int32_t prime_bits, int64_t generator, int32_t* k, uint64_t* primes_out /* [32] */, int32_t* limbs);
                                   /* host only, no device, no context: the largest primes = 1 mod m below 2^prime_bits (prime_bits <= 31), descending,
                                      until P > 2^(bits + 1); refused when there are not enough of them or more than 32 would be needed */
int fhesi_slots_basis_check(int64_t m, const uint64_t* primes, int32_t k, int64_t generator, int32_t* limbs, uint64_t* modulus_out /* [16] or null: P, little-endian */);
                                   /* host only: the checks of fhesi_slots_basis_create on a ring given by m */
int fhesi_slots_basis_create(fhesi_ctx* ctx, const uint64_t* primes, int32_t k, int64_t generator, fhesi_slots_basis** out);
int fhesi_slots_basis_free(fhesi_slots_basis* b);                                  /* frees the channels' spaces with it */
int fhesi_slots_basis_info(const fhesi_slots_basis* b, int32_t* k, uint64_t* primes /* [k] or null */, int32_t* limbs, int64_t* total, int64_t* rows, int64_t* cols);
int fhesi_slots_basis_channel(fhesi_slots_basis* b, int32_t c, fhesi_slots** slots); /* channel c's fhesi_slots for every existing call; OWNED by the basis: never fhesi_slots_free it */
int fhesi_slots_basis_embed(fhesi_slots_basis* b, const int64_t* vals_host /* [count][nvals][L_in] */, int32_t L_in, int64_t nvals, int64_t count,
                            int64_t* msg_host /* [k][count][n] */);                /* slots nvals .. n-1 are zero */
int fhesi_slots_basis_decode(fhesi_slots_basis* b, const int64_t* msg_host /* [k][count][n] */, int64_t count, int64_t nvals,
                             int64_t* vals_host /* [count][nvals][limbs] */);
int fhesi_slots_basis_embed_dev(fhesi_slots_basis* b, const int64_t* vals_dev, int32_t L_in, int64_t nvals, int64_t count, int64_t* msg_dev);
int fhesi_slots_basis_decode_dev(fhesi_slots_basis* b, const int64_t* msg_dev, int64_t count, int64_t nvals, int64_t* vals_dev);
int fhesi_encrypt_int_slots_batch_seeded(fhesi_ctx* ctx, fhesi_slots_basis* b, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                         const int64_t* vals_host /* [count][nvals][L_in] */, int32_t L_in, int64_t nvals, int64_t count, uint64_t* out_dev /* [k][count] */, int32_t nlimbs);
int fhesi_decrypt_int_slots_batch(fhesi_ctx* ctx, fhesi_slots_basis* b, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev /* [k][count] */, int32_t nlimbs, int64_t count,
                                  int64_t nvals, int64_t* vals_host /* [count][nvals][limbs] */);
int fhesi_encrypt_noise_int_batch_seeded(fhesi_ctx* ctx, fhesi_slots_basis* b, const fhesi_dcrt* pk0, const fhesi_dcrt* pk1, int32_t logQ, uint64_t seed, uint64_t first_index,
                                         int64_t count, uint64_t* out_dev /* [k][count] */, int32_t nlimbs);
/* fhesi_ct_noise_batch channel by channel, channel c with p = p_c: a logical ciphertext is as good as its worst channel (the minimum over c) */
int fhesi_ct_noise_int_batch(fhesi_ctx* ctx, fhesi_slots_basis* b, const fhesi_dcrt* sk1, int32_t logQ, const uint64_t* ct_dev /* [k][count] */, int32_t nlimbs, int64_t count,
                             int32_t* budget_host /* [k][count] */);

/* ---- prepared plaintext operands: a ciphertext combined with PLAINTEXT slot values on the device -- a mask, a model applied to encrypted data
 * (y = sum_j theta_j o x_j + b), a diagonal of a plaintext matrix (fhe-si_amd/csrc/kernels_plain.hip, capi_ct.hip).  An extension of the mirror's
 * Ciphertext *= ZZX / += ZZX for callers that hold slot values and reuse an operand many times.
 *
 * SCOPE.  Unscaled two-part ciphertexts [..][2][phi(m)][nlimbs], centred modulo 2^logQ.  A fhesi_plain owns nw <= 65535 plaintext polynomials in evaluation
 * form over ALL chain primes, uint64 [nw][L][phi(m)] canonical residues in HBM: made once (embedding, reduction and forward transforms on the
 * device; the message polynomials never visit the host), read by any number of calls.  It holds a pointer to its context and counts as one of its
 * live handles, exactly as a fhesi_slots does (fhesi_ctx_destroy).
 *   _create_slots: vals_host [nw][nvals] slot values of the space s (any fhesi_slots: single-generator, two-row, a channel of a basis), embedded as
 *     fhesi_slots_embed does: message polynomials in [0, p).  Records maxabs = p - 1.
 *   _create_poly:  poly_host [nw][phi(m)] SIGNED coefficient polynomials, the operand of Ciphertext::operator*=(const ZZX&).  Records maxabs = the
 *     largest magnitude seen; p = 0.
 * fhesi_ct_plain_sum_dev: for every group g,  out[g] = sum_{t in [seg[g], seg[g+1])} pool[a_idx[t]] (*) w[b_idx[t]].  Each product is
 *   CiphertextPart::operator*=(ZZX) (Ciphertext.cpp:29-36: integer product, rem Phi_m, Reduce) on both parts, each sum Ciphertext::operator+=
 *   unscaled (:123-134): bit for bit what fhesi_ct_mul_poly_dev on a copy of the operand and fhesi_ct_add_dev per term give.  Every distinct pool
 *   entry is transformed once however many terms use it, the terms are accumulated exactly in the evaluation domain, and every GROUP is inverted
 *   and reduced once.  a_idx, b_idx, seg are host arrays (seg[0] = 0, non-decreasing, ngroups + 1 entries), the caller's again on return; an empty
 *   segment gives the zero ciphertext.  out_dev [ngroups][2][phi(m)][nlimbs] must not overlap pool_dev.
 * CAPACITY.  Every coefficient of the integer sum is at most T growth n 2^(logQ-1) maxabs in magnitude: T the longest segment, n = phi(m), growth = 1
 *   (m a power of two), 2 (m = q^k or 2 q^k, q an odd prime) or n (any other m), as fhesi_ct_mul_poly_dev sizes its product.  That bound must stay
 *   below HALF the chain product: fhesi_plain_sum_bits returns log2 of twice the bound (0 for no terms or maxabs = 0), which must be below
 *   sum_i log2 q_i.  Host only: no device, no context.
 * REFUSED on the host before anything is launched, with the condition named and the context usable afterwards: a handle of another context, an
 *   index outside the pool or the handle, seg not starting at 0 or decreasing, out overlapping pool, nvals outside 1 .. phi(m), coefficients that
 *   cannot hold logQ, a sum the chain cannot hold (the message gives the bits needed and the bits of the chain), chain primes above 61 bits.
 * fhesi_ct_add_slots_dev: Ciphertext::operator+=(const ZZX&) unscaled (Ciphertext.cpp:147-156) with the constant given as slot values
 *   vals_host [nv][nvals], nv = 1 (one constant for every ciphertext) or count, embedded on the device; p is the space's.  Equals
 *   fhesi_ct_add_const_dev(fhesi_slots_embed(vals)) bit for bit. */
int fhesi_plain_create_slots(fhesi_slots* s, const int64_t* vals_host /* [nw][nvals] */, int64_t nvals, int32_t only_usable, int64_t nw, fhesi_plain** out);
int fhesi_plain_create_poly(fhesi_ctx* ctx, const int64_t* poly_host /* [nw][phi(m)] */, int64_t nw, fhesi_plain** out);
int fhesi_plain_free(fhesi_plain* w);
int fhesi_plain_info(const fhesi_plain* w, int64_t* nw, uint64_t* maxabs, uint64_t* p /* 0 for the polynomial form */);
int fhesi_plain_sum_bits(int64_t m, int32_t logQ, uint64_t maxabs, int64_t terms, double* bits);
int fhesi_ct_plain_sum_dev(fhesi_ctx* ctx, const fhesi_plain* w, int32_t logQ, const uint64_t* pool_dev /* [npool][2][phi(m)][nlimbs] */, int64_t npool,
                           int32_t nlimbs, const int32_t* a_idx, const int32_t* b_idx, const int32_t* seg, int64_t ngroups,
                           uint64_t* out_dev /* [ngroups][2][phi(m)][nlimbs] */);
int fhesi_ct_add_slots_dev(fhesi_ctx* ctx, fhesi_slots* s, int32_t logQ, uint64_t* ct_dev, int32_t nparts, int32_t nlimbs, int64_t count,
                           const int64_t* vals_host /* [nv][nvals] */, int64_t nvals, int32_t only_usable, int64_t nv /* 1 or count */);

/* ---- hoisted rotations: MANY automorphism key switches of ONE ciphertext -- the T rotations of a matrix-vector product by diagonals
 * (fhe-si_amd/csrc/capi_pipeline.hip, dot32_kernel2m in kernels_aux32.hip).  sigma_k is a ring map, so for the key-switch matrix W_k
 * of the automorphism k (source key (1, s(X^k)), target s: KeySwitchSI::InitAutomorph)
 *     sum_j sigma_k(D_j(c)) W_k[j]  =  sigma_k( sum_j D_j(c) W'_k[j] ),     W'_k = sigma_k^-1(W_k)  (every column, both rows)
 * modulo (Phi_m, 2^logQ): the digits D_j of the UNTOUCHED ciphertext are decomposed and transformed once and serve every rotation; a rotation then
 * costs one dot product with its derived matrix, one inverse, one recombination and a signed gather of two polynomials.
 *
 * fhesi_ksk_hoist: out = a new matrix of k's shape and context whose rows are k's evaluation rows moved by kk^-1 mod m (on the device, any ring); it
 *   remembers kk.  For every other entry point it is an ordinary matrix (fhesi_ksk_free / _bytes / _form / _key_bits / _download / a key switch with
 *   it); its auxiliary tables are built at its first use, like any matrix's, and may take one limb more than the source's where sigma reduces modulo
 *   Phi_m (m not a power of two).  It costs the memory of a second matrix: fhesi_ksk_bytes plus the table.  Refused: kk outside Z_m^*, a matrix with
 *   other than 2 source components.
 * fhesi_ct_rotations_dev: for t < nk, i < count
 *       out[t][i] = Reduce( Ciphertext >>= ks[t]  of  ApplyKeySwitch(hoisted[t], in[i]) )        (centred modulo 2^logQ)
 *   -- a ciphertext of the plaintext of in[i] moved by ks[t], under the same key, with noise of the same distribution as `>>= k; ApplyKeySwitch(W_k)`
 *   gives.  NOT that path's bits: it decomposes sigma_k(c), this one applies sigma_k to the digits of c.  It IS, bit for bit,
 *   fhesi_ct_automorph_key_switch_dev(hoisted[t], k = 1) followed by fhesi_ct_automorph_dev(ks[t]) and the reduction, whatever the option "hoist_dot"
 *   says.  hoisted[t] == NULL with ks[t] == 1 is the identity: the reduced copy of the input (diagonal 0).  in_dev [count][2][phi(m)][nlimbs_in],
 *   out_dev [nk][count][2][phi(m)][nlimbs], not overlapping.  All four forms of the key switch run it; in the four-prime limb form few ciphertexts
 *   meet all matrices of one table shape in ONE launch of the dot product (matrices whose tables differ in limb count or width go in groups).
 * fhesi_ct_matvec_dev: out[i] = sum_t<nk rot_t(in[i]) (*) w[t], w a fhesi_plain of nw >= nk diagonals (w[t] goes with ks[t]): bit for bit
 *   fhesi_ct_rotations_dev into a pool followed by fhesi_ct_plain_sum_dev; the pool lives in the workspace, in chunks of ciphertexts.  The capacity
 *   rule of fhesi_ct_plain_sum_dev (nk terms) is checked before anything is launched.
 * REFUSED on the host with the condition named, the context usable afterwards: a matrix not made by fhesi_ksk_hoist or hoisted for another k than
 *   ks[t]; a missing matrix with ks[t] != 1; a matrix of another context; digit count or limb capacity as for any key switch; out overlapping in;
 *   a prepared plaintext of another context or with fewer than nk diagonals; a sum the chain cannot hold. */
int fhesi_ksk_hoist(const fhesi_ksk* k, int64_t kk, fhesi_ksk** out);
int fhesi_ct_rotations_dev(fhesi_ctx* ctx, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes,
                           const uint64_t* in_dev /* [count][2][phi(m)][nlimbs_in] */, int32_t nlimbs_in, int64_t count,
                           uint64_t* out_dev /* [nk][count][2][phi(m)][nlimbs] */, int32_t nlimbs);
int fhesi_ct_matvec_dev(fhesi_ctx* ctx, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, const fhesi_plain* w /* nw >= nk diagonals */,
                        int32_t logQ, int32_t decomp_bytes, const uint64_t* in_dev, int32_t nlimbs, int64_t count,
                        uint64_t* out_dev /* [count][2][phi(m)][nlimbs] */);

/* ---- baby-step/giant-step matrix-vector products on the hoisted rotations (capi_pipeline.hip, ct_rot_sum_kernel in kernels_ct.hip).
 * With T = B G diagonals and t = g B + j
 *     sum_t d_t (*) rot_t(x)  =  sum_{g<G} rot_{gB}( sum_{j<B} rot_{-gB}(d_{gB+j}) (*) rot_j(x) ):
 * B - 1 baby rotations of x from ONE digit decomposition, G plaintext sums over diagonals rotated in the clear, G - 1 further key switches and one
 * sum of rotated ciphertexts -- about 2 sqrt(T) matrices and key switches where fhesi_ct_matvec_dev takes T of each.
 *
 * fhesi_ct_rot_sum_dev: out[i] = Reduce( base[i] + sum_t<nk  Ciphertext >>= ks[t]  of  pre[t][i] )  (centred modulo 2^logQ), i < count two-part
 *   ciphertexts of nlimbs limbs; base_dev NULL: no base.  Bit for bit fhesi_ct_automorph_dev(ks[t]) per term, fhesi_ct_add_dev, and the reduction.
 *   On m = 2^k, q^k and 2 q^k one kernel reads every term once and writes once (FHESI_ROT_SUM_MAX_TERMS terms per launch, more terms chain launches);
 *   on other rings, or with option "automorph_rows", the library runs the composition itself: the same words.  out_dev may be base_dev.
 *   REFUSED on the host with the condition named: out overlapping pre, or overlapping base without being base; a k outside Z_m^*; nlimbs outside
 *   1..32 or too few for logQ; nk < 1.
 * fhesi_matvec_bsgs_plan (host only): the B that minimises (B - 1) + (G - 1) with G = ceil(nk / B); of equal sums the larger B (baby steps are the
 *   hoisted, cheaper ones).
 * fhesi_ct_matvec_bsgs_dev:
 *       out[i] = Reduce( sum_{g<G} rot_kg[g]( sum_{j<B, gB+j<nk} rot_kb[j](in[i]) (*) w[gB+j] ) )
 *   rot_k exactly what fhesi_ct_rotations_dev gives for (matrix, k); a NULL matrix with k = 1 is the identity; the last group may be ragged:
 *   (G - 1) B < nk <= G B.  DEFINED as, and word for word equal to, fhesi_ct_rotations_dev for the babies, fhesi_ct_plain_sum_dev with G groups per
 *   ciphertext, fhesi_ct_rotations_dev with nk = 1 per giant, fhesi_ct_add_dev; with G = 1 it is fhesi_ct_matvec_dev.  The caller rotates the
 *   diagonals in the clear: w[gB+j] holds rot_{-gB}(d_{gB+j}) (SlotSpace.bsgs_diagonals in the Python binding).  The capacity rule of
 *   fhesi_ct_plain_sum_dev is checked with min(B, nk) terms, the longest inner sum.  Everything between in and out lives in the workspace, in chunks
 *   of ciphertexts.  REFUSED as fhesi_ct_matvec_dev refuses, and: B or G below 1; nk outside ((G - 1) B, G B]. */
#define FHESI_ROT_SUM_MAX_TERMS 16
int fhesi_ct_rot_sum_dev(fhesi_ctx* ctx, const int64_t* ks, int32_t nk, int32_t logQ, const uint64_t* base_dev /* [count][2][phi(m)][nlimbs] or NULL */,
                         const uint64_t* pre_dev /* [nk][count][2][phi(m)][nlimbs] */, int64_t count, int32_t nlimbs, uint64_t* out_dev);
int fhesi_matvec_bsgs_plan(int64_t nk, int32_t* baby, int32_t* giant);
int fhesi_ct_matvec_bsgs_dev(fhesi_ctx* ctx, const fhesi_ksk* const* baby_hoisted, const int64_t* kb, int32_t B, const fhesi_ksk* const* giant_hoisted,
                             const int64_t* kg, int32_t G, int32_t nk, const fhesi_plain* w /* nw >= nk, term t = g*B + j */, int32_t logQ,
                             int32_t decomp_bytes, const uint64_t* in_dev, int32_t nlimbs, int64_t count, uint64_t* out_dev);

/* ---- dense linear layers on packed slots: y = M x + b for an R x C matrix given as a matrix (capi_ct.hip, capi_pipeline.hip, linear_diag_kernel in
 * kernels_slots.hip).  The space has rows (1 or 2) rows of cols slots, rot_t moves every row t slots to the left.  D = max(R, C),
 * T = min(R, C).  ADMITTED: R, C >= 1, T | D, D | cols, and for R < C the ratio C / R a power of two.
 *   input      slot (r, i) = x_r[i mod C]: a vector of length C per row, replicated with period C
 *   diagonals  e_t[i] = M[(i mod D) mod R][((i mod D) + t) mod C], t < T, alike in every row, period D
 *   prepared   w_t = rot_{-gB}(e_t) for t = g B + j, j < B:  w_t[i] = e_t[(i - g B) mod D]
 *   product    y = sum_g rot_{gB}( sum_j w_{gB+j} (*) rot_j(x) )                                    (fhesi_ct_matvec_bsgs_dev)
 *   folds      only for R < C: for a = C/2, C/4, .., R:  y <- y + rot_a(y)                          (fhesi_ct_rot_fold_dev)
 *   bias       y <- y + (b[i mod R])                                                                (fhesi_ct_add_slots_dev)
 *   result     slot (r, i) = (M x_r + b)[i mod R], period R: the replicated input of a following layer with C' = R.
 * R diagonals where the matrix padded to a D x D square takes D: B + G - 2 + log2(C / R) key switches instead of about 2 sqrt(D).
 *
 * fhesi_linear_plan (host only): T, B (baby = 0: what fhesi_matvec_bsgs_plan(T) picks; otherwise min(baby, T)), G = ceil(T / B), nfold = log2(C / R) for
 *   R < C and 0 otherwise, and -- amounts != NULL -- the B - 1 + G - 1 + nfold rotation amounts in the order every call below takes their matrices:
 *   the babies 1 .. B - 1, the giants B, 2B, .., (G - 1) B, the folds C/2 .. R.  An amount two lists share is listed once per use.  Any output may be
 *   NULL.  REFUSED with the condition named: a size below 1, D above cols, D not dividing cols, T not dividing D, C / R not a power of two, baby < 0.
 * fhesi_linear_create / _create_dev: the handle of one layer on the space s -- M [R][C] row-major and bias [R] (or NULL) any int64, reduced into [0, p)
 *   on the device; _dev takes both in HBM, where they stay (the call synchronises).  linear_diag_kernel writes the T slot vectors w_t, the embedding and
 *   the transforms of fhesi_plain_create_slots follow: the handle's plaintext IS fhesi_plain_create_slots(w, only_usable = 0).  The handle owns that
 *   plaintext, the replicated bias as slot values and the plan; it counts as a live handle of the context and borrows s, which must outlive it.
 *   T <= 65535 as for any fhesi_plain.  fhesi_linear_info: shape, plan, whether it has a bias, the amounts (any pointer may be NULL).
 * fhesi_linear_diagonals: the same stage without a handle -- vals_host [T][phi(m)] receives the slot vectors w_t.
 * fhesi_ct_rot_fold_dev: y_0 = Reduce(in), y_{s+1} = Reduce(y_s + rot_ks[s](y_s)), out = y_nk -- SumBatchedData on hoisted matrices.  rot_k exactly what
 *   fhesi_ct_rotations_dev gives for (hoisted[s], ks[s]).  DEFINED as, and word for word equal to, per step fhesi_ct_rotations_dev with nk = 1 followed
 *   by fhesi_ct_add_dev.  Per step and chunk of ciphertexts one key switch into the workspace and one rotated sum with base y_s.  out_dev may be in_dev
 *   (the same address; any other overlap is refused).  REFUSED as fhesi_ct_rotations_dev refuses.
 * fhesi_ct_linear_dev: out[i] = the layer of in[i].  hoisted [nh]: the matrices of the amounts in fhesi_linear_info's order (k = g^amount mod m), NULL
 *   only where that k is 1.  DEFINED as, and word for word equal to, fhesi_ct_matvec_bsgs_dev with the handle's plaintext, fhesi_ct_rot_fold_dev over
 *   the fold amounts, fhesi_ct_add_slots_dev with the replicated bias.  The capacity rule of fhesi_ct_plain_sum_dev is checked with min(B, T) terms
 *   before anything is launched.  REFUSED on the host with the condition named, the context usable afterwards: nh other than the plan's count; a
 *   matrix not hoisted or hoisted for another k; a handle or a matrix of another context; out overlapping in; what fhesi_ct_matvec_bsgs_dev refuses. */
typedef struct fhesi_linear fhesi_linear; /* one R x C layer on a slot space: its prepared diagonals, its replicated bias and its plan */
int fhesi_linear_plan(int64_t cols, int64_t R, int64_t C, int32_t baby /* 0: the planner's */, int32_t* T, int32_t* B, int32_t* G, int32_t* nfold,
                      int64_t* amounts /* [B - 1 + G - 1 + nfold] or NULL */);
int fhesi_linear_create(fhesi_slots* s, const int64_t* M_host /* [R][C] */, int64_t R, int64_t C, const int64_t* bias_host /* [R] or NULL */, int32_t baby,
                        fhesi_linear** out);
int fhesi_linear_create_dev(fhesi_slots* s, const int64_t* M_dev /* [R][C] */, int64_t R, int64_t C, const int64_t* bias_dev /* [R] or NULL */, int32_t baby,
                            fhesi_linear** out);
int fhesi_linear_free(fhesi_linear* lin);
int fhesi_linear_info(const fhesi_linear* lin, int64_t* R, int64_t* C, int32_t* T, int32_t* B, int32_t* G, int32_t* nfold, int32_t* has_bias,
                      int64_t* amounts /* [B - 1 + G - 1 + nfold] or NULL */);
int fhesi_linear_diagonals(fhesi_slots* s, const int64_t* M_host /* [R][C] */, int64_t R, int64_t C, int32_t baby, int64_t* vals_host /* [T][phi(m)] */);
int fhesi_ct_rot_fold_dev(fhesi_ctx* ctx, const fhesi_ksk* const* hoisted, const int64_t* ks, int32_t nk, int32_t logQ, int32_t decomp_bytes,
                          const uint64_t* in_dev /* [count][2][phi(m)][nlimbs] */, int32_t nlimbs, int64_t count, uint64_t* out_dev);
int fhesi_ct_linear_dev(fhesi_ctx* ctx, const fhesi_linear* lin, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes,
                        const uint64_t* in_dev /* [count][2][phi(m)][nlimbs] */, int32_t nlimbs, int64_t count, uint64_t* out_dev);

/* ---- dense layers larger than a row of slots: an R x C matrix as a grid of nI x nJ blocks of Rb x Cb, R = nI Rb, C = nJ Cb (capi_ct.hip,
 * capi_pipeline.hip, linear_diag_kernel in kernels_slots.hip).  The block shape is one fhesi_linear_plan(cols, Rb, Cb, .) admits;
 * T = min(Rb, Cb), D = max(Rb, Cb), nfold and the folds are the block's.  Rotations are ring maps and plaintext sums are exact, so
 *   input      nJ ciphertexts per item, ciphertext J: slot (r, i) = x_r[J Cb + (i mod Cb)]
 *   diagonals  of block (I, J): those of fhesi_linear_create on the sub-matrix M[I Rb .., J Cb ..] with the grid's B,
 *              e_t[i] = M[I Rb + (i mod D) mod Rb][J Cb + ((i mod D) + t) mod Cb],  w^{IJ}_t = rot_{-gB}(e_t), t = g B + j
 *   output     y_I = fold( sum_{g<G} rot_{gB}( sum_{J<nJ} sum_{j<B, gB+j<T} w^{IJ}_{gB+j} (*) rot_j(x_J) ) ) + b_I
 *   result     slot (r, i) of y_I = (M x_r + b)[I Rb + (i mod Rb)]
 * the baby rotations of input block J serve every output block and the giants and folds of output block I run behind the sum over J:
 * nJ (B - 1) + nI (G - 1) + nI nfold key switches where one fhesi_linear per block takes nI nJ (B + G - 2 + nfold).
 *
 * fhesi_linear_grid_plan (host only): nI, nJ, the block's T and nfold, B (baby = 0: the B in 1 .. T that minimises nJ (B - 1) + nI (ceil(T / B) - 1),
 *   of equal costs the larger; otherwise min(baby, T)), G = ceil(T / B), and the amounts in fhesi_linear_plan's order: babies 1 .. B - 1, giants
 *   B .. (G - 1) B, the block's folds Cb/2 .. Rb.  A 1 x 1 grid plans as fhesi_linear_plan does.  Any output may be NULL.  REFUSED with the condition
 *   named: a block shape fhesi_linear_plan refuses (in its words); R not a multiple of Rb or C not a multiple of Cb (the caller pads with zeros);
 *   more than 65535 diagonals nI nJ T per handle.
 * fhesi_linear_grid_create / _create_dev: M [R][C] row-major and bias [R] (or NULL) any int64, on the host or in HBM as for fhesi_linear_create.  The
 *   handle owns ONE prepared plaintext of nI nJ T diagonals, row (I nJ + J) T + t, the replicated biases [nI][phi(m)] and the plan; the diagonals
 *   are written, embedded and transformed in chunks of whole blocks, so the workspace holds a chunk and never the grid.  It counts as a live handle
 *   of the context and borrows s.  fhesi_linear_grid_info: shapes, plan, whether it has a bias, the amounts (any pointer may be NULL).
 * fhesi_linear_grid_diagonals: the same stage without a handle -- vals_host [nI][nJ][T][phi(m)] receives the slot vectors.
 * fhesi_ct_linear_grid_dev: in_dev [nJ][count], out_dev [nI][count] two-part ciphertexts; hoisted [nh] as fhesi_ct_linear_dev takes them.  DEFINED
 *   as, and word for word equal to: fhesi_ct_rotations_dev per input block (identity first) into one pool [nJ][min(B, T)][count]; ONE
 *   fhesi_ct_plain_sum_dev with the groups (I, g, i) and the terms (J, j); per output block fhesi_ct_rotations_dev of each inner sum by its giant
 *   and fhesi_ct_add_dev; fhesi_ct_rot_fold_dev; fhesi_ct_add_slots_dev with the block's replicated bias.  A 1 x 1 grid returns the words of
 *   fhesi_ct_linear_dev.  The capacity rule of fhesi_ct_plain_sum_dev is checked with nJ min(B, T) terms before anything is launched; pool, inner
 *   sums and key-switched sums live in the workspace, in chunks of ciphertexts.  REFUSED as fhesi_ct_linear_dev refuses.
 * NOT HERE: a form of the C++ mirror; a form over a slot basis (a caller runs one grid per channel); Cb / Rb other than a power of two inside a
 *   block; mixing the two rows of a two-row space. */
typedef struct fhesi_linear_grid fhesi_linear_grid; /* a grid of blocks on a slot space: its prepared diagonals, its replicated biases and its plan */
int fhesi_linear_grid_plan(int64_t cols, int64_t R, int64_t C, int64_t Rb, int64_t Cb, int32_t baby /* 0: the planner's */, int32_t* nI, int32_t* nJ, int32_t* T,
                           int32_t* B, int32_t* G, int32_t* nfold, int64_t* amounts /* [B - 1 + G - 1 + nfold] or NULL */);
int fhesi_linear_grid_create(fhesi_slots* s, const int64_t* M_host /* [R][C] */, int64_t R, int64_t C, int64_t Rb, int64_t Cb,
                             const int64_t* bias_host /* [R] or NULL */, int32_t baby, fhesi_linear_grid** out);
int fhesi_linear_grid_create_dev(fhesi_slots* s, const int64_t* M_dev /* [R][C] */, int64_t R, int64_t C, int64_t Rb, int64_t Cb,
                                 const int64_t* bias_dev /* [R] or NULL */, int32_t baby, fhesi_linear_grid** out);
int fhesi_linear_grid_free(fhesi_linear_grid* grid);
int fhesi_linear_grid_info(const fhesi_linear_grid* grid, int64_t* R, int64_t* C, int64_t* Rb, int64_t* Cb, int32_t* nI, int32_t* nJ, int32_t* T, int32_t* B,
                           int32_t* G, int32_t* nfold, int32_t* has_bias, int64_t* amounts /* [B - 1 + G - 1 + nfold] or NULL */);
int fhesi_linear_grid_diagonals(fhesi_slots* s, const int64_t* M_host /* [R][C] */, int64_t R, int64_t C, int64_t Rb, int64_t Cb, int32_t baby,
                                int64_t* vals_host /* [nI][nJ][T][phi(m)] */);
int fhesi_ct_linear_grid_dev(fhesi_ctx* ctx, const fhesi_linear_grid* grid, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes,
                             const uint64_t* in_dev /* [nJ][count][2][phi(m)][nlimbs] */, int32_t nlimbs, int64_t count,
                             uint64_t* out_dev /* [nI][count][2][phi(m)][nlimbs] */);

/* ---- convolution layers on packed slots: a 2-D convolution over image planes, one channel per ciphertext (capi_ct.hip, capi_pipeline.hip, conv_plan.h,
 * conv_lattice_mask_kernel in kernels_slots.hip; tests/conv_model.py is the normative statement).  The space has rows of `cols` slots; rot_a moves
 * every row a slots to the left.
 *   plane      H x W, P = H W | cols: slot (r, i) holds pixel (y, x) = ((i mod P) div W, (i mod P) mod W) of image (r, i div P) -- cols / P images per row
 *   channels   an item is Cin ciphertexts in[J][i], the result Cout ciphertexts out[I][i], the [block][count] order of fhesi_ct_linear_grid_dev
 *   kernel     K [Cout][Cin][kh][kw] any int64 (reduced into [0, p) on the device), anchor (ah, aw), stride 1, zero padding ("same", cross-correlation):
 *              out[I](y, x) = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](y + dy - ah, x + dx - aw),  pixels outside the plane = 0
 *   offsets    t = dy kw + dx, u = dy - ah, v = dx - aw, mask mu_{u,v}[i] = [0 <= y + u < H and 0 <= x + v < W]; where the mask is 1, i + u W + v stays
 *              in the P-block of i, so the cyclic rotation of the whole row is harmless
 *   flat       out[I] = sum_J sum_t w^{IJ}_t (*) rot_{a_t}(in[J]) + b[I],  a_t = (u W + v) mod cols,  w^{IJ}_t[i] = K[I][J][dy][dx] mu_{u,v}[i]
 *   split      out[I] = sum_dy rot_{(u W) mod cols}( sum_J sum_dx w'^{IJ}_t (*) rot_{v mod cols}(in[J]) ) + b[I],  w'^{IJ}_t[i] = w^{IJ}_t[(i - u W) mod cols]
 * Key switches per item: flat Cin (kh kw - 1) over up to kh kw - 1 distinct matrices; split Cin (kw - 1) + Cout (kh - 1) over kh + kw - 2 matrices -- one
 * digit set of an input channel serves every output channel.  Two offsets may share an amount modulo cols; it is listed and run once per use.
 *
 * fhesi_conv2d_plan (host only): form 0 = the planner's (the form of fewer key switches, flat on a tie: one key-switch level less), 1 flat, 2 split.
 *   amounts in the order the run call takes its matrices -- flat: nh = kh kw, entry t; split: nh = kw + kh, the kw baby amounts v mod cols, then the kh
 *   giant amounts (u W) mod cols.  Amount 0 appears exactly at the anchor, and the matrix there is NULL.  terms = the longest plaintext sum: Cin kh kw
 *   (flat), Cin kw (split).  Any output may be NULL.  REFUSED with the condition named: a size below 1; P not dividing cols; an anchor outside the kernel;
 *   an offset whose mask is empty (|u| >= H or |v| >= W), naming the offset; more than 65535 plaintexts Cout Cin kh kw per handle; form outside 0 .. 2.
 * fhesi_conv2d_create / _create_dev: K and bias [Cout] (or NULL) contiguous int64, on the host or in HBM where they stay, as for fhesi_linear_create.  The
 *   handle owns ONE prepared plaintext of Cout Cin kh kw rows, row (I Cin + J) kh kw + t -- equal to fhesi_plain_create_slots of the w (flat) or w' (split)
 *   above with only_usable = 0 --, the biases as slot values [Cout][phi(m)] (b[I] in every slot) and the plan; the plaintexts are written, embedded and
 *   transformed in chunks of whole channel pairs, so the workspace holds a chunk and never the layer.  It counts as a live handle of the context and
 *   borrows s.  fhesi_conv2d_info: shapes, plan, whether it has a bias, the amounts (any pointer may be NULL).
 * fhesi_conv2d_masks: the same stage without a handle -- vals_host [Cout][Cin][kh kw][phi(m)] receives the slot vectors.
 * fhesi_ct_conv2d_dev: in_dev [Cin][count], out_dev [Cout][count] two-part ciphertexts; hoisted [nh]: entry t the hoisted matrix of g^amounts[t] mod m.
 *   DEFINED as, and word for word equal to -- flat: fhesi_ct_rotations_dev per input channel over the nh amounts into one pool [Cin][kh kw][count]; ONE
 *   fhesi_ct_plain_sum_dev with the groups (I, i) and the terms (J, t); fhesi_ct_add_slots_dev with b[I] per output channel.  split: the rotations per
 *   input channel over the kw baby amounts into a pool [Cin][kw][count]; ONE plaintext sum with the groups (I, dy, i) and the terms (J, dx); per output
 *   channel fhesi_ct_rotations_dev (nk = 1) of each inner sum by its giant, the first into out, the others added with fhesi_ct_add_dev; then the bias.
 *   The capacity rule of fhesi_ct_plain_sum_dev is checked with `terms` before anything is launched.  REFUSED with the condition named: nh other than
 *   the plan's; a matrix missing where the amount is not 0, present where it is 0, not hoisted, hoisted for another k or of another context; a layer of
 *   another context; out overlapping in; whatever the calls it is composed of refuse.
 * NOT HERE: stride and dilation (fhesi_conv2d_lattice_*, below); "valid" output; several channels inside one ciphertext; depthwise / grouped kernels; a form that keeps the weights as
 *   scalars against kh kw shared masks; pruning zero weights; a form of the C++ mirror; mixing the two rows of a two-row space. */
typedef struct fhesi_conv2d fhesi_conv2d; /* a convolution layer on a slot space: its masked weight plaintexts, its biases and its plan */
int fhesi_conv2d_plan(int64_t cols, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kh, int64_t kw, int64_t ah, int64_t aw,
                      int32_t form /* 0 planner, 1 flat, 2 split */, int32_t* form_out, int32_t* nh, int64_t* key_switches, int64_t* terms,
                      int64_t* amounts /* [nh] or NULL */);
int fhesi_conv2d_create(fhesi_slots* s, const int64_t* K_host /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                        int64_t ah, int64_t aw, const int64_t* bias_host /* [Cout] or NULL */, int32_t form, fhesi_conv2d** out);
int fhesi_conv2d_create_dev(fhesi_slots* s, const int64_t* K_dev /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                            int64_t ah, int64_t aw, const int64_t* bias_dev /* [Cout] or NULL */, int32_t form, fhesi_conv2d** out);
int fhesi_conv2d_free(fhesi_conv2d* conv);
int fhesi_conv2d_info(const fhesi_conv2d* conv, int64_t* Cout, int64_t* Cin, int64_t* kh, int64_t* kw, int64_t* H, int64_t* W, int64_t* ah, int64_t* aw,
                      int32_t* form, int32_t* nh, int64_t* key_switches, int64_t* terms, int32_t* has_bias, int64_t* amounts /* [nh] or NULL */);
int fhesi_conv2d_masks(fhesi_slots* s, const int64_t* K_host /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                       int64_t ah, int64_t aw, int32_t form, int64_t* vals_host /* [Cout][Cin][kh kw][phi(m)] */);
int fhesi_ct_conv2d_dev(fhesi_ctx* ctx, const fhesi_conv2d* conv, const fhesi_ksk* const* hoisted, int32_t nh, int32_t logQ, int32_t decomp_bytes,
                        const uint64_t* in_dev /* [Cin][count][2][phi(m)][nlimbs] */, int32_t nlimbs, int64_t count,
                        uint64_t* out_dev /* [Cout][count][2][phi(m)][nlimbs] */);

/* ---- strided and dilated convolutions and sum pooling: the plane carries a lattice step and is never compacted (capi_ct.hip, capi_pipeline.hip,
 * conv_plan.h, lattice_plan.h, conv_lattice_mask_kernel and lattice_columns_kernel in kernels_slots.hip; tests/lattice_model.py is the normative statement).
 *   lattice    input step (sy, sx), sy | H, sx | W: logical pixel (a, b) of the Hl x Wl = H/sy x W/sx logical plane at physical pixel (a sy, b sx); slots
 *              off the lattice are don't care on input.  A strided convolution and a pooling multiply the step; the next layer takes it as its input step
 *   geometry   six integers sy, sx, ty, tx, ey, ex: step, stride (ty | Hl, tx | Wl), dilation (at least 1); the output step is (sy ty, sx tx)
 *   definition out[I](a', b') = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](a' ty + (dy - ah) ey, b' tx + (dx - aw) ex),  logical pixels outside
 *              Hl x Wl = 0;  EVERY output slot off the output lattice is exactly 0, bias included
 *   offsets    t = dy kw + dx in physical pixels u = (dy - ah) ey sy, v = (dx - aw) ex sx, amount a_t = (u W + v) mod cols,
 *              mu_t[i] = [sy ty | y and sx tx | x and 0 <= y + u < H and 0 <= x + v < W];  flat and split as above, the split form's plaintexts moved
 *              back by (u W) mod cols, lattice factor included.  Key switches and the planner's rule do not change.
 * fhesi_conv2d_lattice_plan (host only): fhesi_conv2d_plan's outputs and the output step.  REFUSED with the condition named, in this order: cols; a size
 *   below 1; P not dividing cols; a factor of the geometry below 1; a step not dividing the plane; a stride not dividing the logical plane; the anchor; an
 *   offset whose mask is empty after step and dilation (|u| >= H or |v| >= W), naming it in physical pixels; the plaintexts of one handle; the form.  With
 *   step, stride and dilation all (1, 1): the refusals, the plan and every word of the plaintexts of fhesi_conv2d_*.
 * fhesi_conv2d_lattice_create / _create_dev / _masks: as fhesi_conv2d_create / _create_dev / _masks; the bias rows are b[I] on the output lattice and 0 off
 *   it.  The handle is a fhesi_conv2d that also records its geometry (fhesi_conv2d_lattice_info: the six integers and the output step; all 1 for a handle of
 *   fhesi_conv2d_create); fhesi_conv2d_info, fhesi_conv2d_free and the run call fhesi_ct_conv2d_dev take it as it is.
 * fhesi_pool2d_plan (host only), fhesi_ct_pool2d_dev: SUM pooling over non-overlapping windows of kh x kw logical pixels on a plane of step (sy, sx).  The
 *   windows must tile the plane (kh sy | H, kw sx | W); they then never cross a plane border, so there is no mask and NO plaintext product:
 *     out = sum_{dy < kh} rot_{(dy sy W) mod cols}( sum_{dx < kw} rot_{(dx sx) mod cols}(in) ),
 *   the window's sum at its top left pixel, output step (sy kh, sx kw); slots off the output lattice hold the cyclic sums this formula gives.  It is a
 *   sum: the caller folds 1 / (kh kw) into the next layer's weights.  Global pooling is kh = Hl, kw = Wl.  Channels and items are one `count`.
 *   form 1     per direction the k - 1 rotations hoisted from ONE digit set, summed with the running value as base in one rotated sum: (kw - 1) + (kh - 1)
 *              key switches over two key-switch levels.  amounts: dx sx for dx = 1 .. kw - 1, then dy sy W for dy = 1 .. kh - 1
 *   form 2     kw and kh powers of two: doubling folds y <- y + rot(y) by sx 2^j, then by sy W 2^j: log2 kw + log2 kh key switches and as many levels
 *   form 0     the form of fewer key switches, form 1 on a tie (fewer levels)
 *   hoisted [nh]: entry t the hoisted matrix of g^amounts[t] mod m, horizontal amounts first (nhor of them), none NULL.  out_dev may be in_dev.
 *   DEFINED as, and word for word equal to -- form 1: y = Reduce(in); per direction fhesi_ct_rotations_dev of y over the direction's amounts and
 *   fhesi_ct_add_dev of every term onto y, horizontal then vertical (sums are exact modulo 2^logQ with the centred store, so the order of terms is free);
 *   form 2: fhesi_ct_rot_fold_dev over the amounts.  REFUSED with the condition named before any launch: a size below 1; P not dividing cols; a step not
 *   dividing the plane; windows that do not tile the logical plane; a form outside 0 .. 2, form 2 on a window that is no power of two; nh other than the
 *   plan's; a matrix missing, not hoisted, hoisted for another k or of another context; out overlapping in without being in.
 *   Overlapping or padded pooling is no tiling: it stays a convolution with a constant kernel, run with Cin = Cout = 1 over `count`.
 * fhesi_slots_lattice_columns / _dev: the bridge to a dense layer.  M [R][nch Hl Wl] over logical pixels (host / HBM) -> M' [R][nch H W] over the slots of
 *   nch planes, column c P + (a sy) W + b sx = column c Hl Wl + a Wl + b, zero columns off the lattice, the words as they are;
 *   fhesi_linear_grid_create[_dev] with Cb = H W takes M' as it is.  out must not overlap M.
 * NOT HERE: compaction of a stepped plane; several channels inside one ciphertext; depthwise / grouped kernels; "valid" output; max pooling; a form of the
 *   C++ mirror. */
int fhesi_conv2d_lattice_plan(int64_t cols, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t kh, int64_t kw, int64_t ah, int64_t aw, int64_t sy, int64_t sx,
                              int64_t ty, int64_t tx, int64_t ey, int64_t ex, int32_t form /* 0 planner, 1 flat, 2 split */, int32_t* form_out, int32_t* nh,
                              int64_t* key_switches, int64_t* terms, int64_t* out_sy, int64_t* out_sx, int64_t* amounts /* [nh] or NULL */);
int fhesi_conv2d_lattice_create(fhesi_slots* s, const int64_t* K_host /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                                int64_t ah, int64_t aw, int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex,
                                const int64_t* bias_host /* [Cout] or NULL */, int32_t form, fhesi_conv2d** out);
int fhesi_conv2d_lattice_create_dev(fhesi_slots* s, const int64_t* K_dev /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                                    int64_t ah, int64_t aw, int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex,
                                    const int64_t* bias_dev /* [Cout] or NULL */, int32_t form, fhesi_conv2d** out);
int fhesi_conv2d_lattice_masks(fhesi_slots* s, const int64_t* K_host /* [Cout][Cin][kh][kw] */, int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int64_t H, int64_t W,
                               int64_t ah, int64_t aw, int64_t sy, int64_t sx, int64_t ty, int64_t tx, int64_t ey, int64_t ex, int32_t form,
                               int64_t* vals_host /* [Cout][Cin][kh kw][phi(m)] */);
int fhesi_conv2d_lattice_info(const fhesi_conv2d* conv, int64_t* sy, int64_t* sx, int64_t* ty, int64_t* tx, int64_t* ey, int64_t* ex, int64_t* out_sy, int64_t* out_sx);
int fhesi_pool2d_plan(int64_t cols, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sy, int64_t sx, int32_t form /* 0 planner, 1 hoisted sums, 2 doubling */,
                      int32_t* form_out, int32_t* nh, int32_t* nhor, int64_t* key_switches, int32_t* levels, int64_t* out_sy, int64_t* out_sx,
                      int64_t* amounts /* [nh] or NULL */);
int fhesi_ct_pool2d_dev(fhesi_slots* s, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sy, int64_t sx, int32_t form, const fhesi_ksk* const* hoisted, int32_t nh,
                        int32_t logQ, int32_t decomp_bytes, const uint64_t* in_dev /* [count][2][phi(m)][nlimbs] */, int32_t nlimbs, int64_t count,
                        uint64_t* out_dev /* [count][2][phi(m)][nlimbs]; may be in_dev */);
int fhesi_slots_lattice_columns(fhesi_slots* s, const int64_t* M_host /* [R][nch (H/sy) (W/sx)] */, int64_t R, int64_t nch, int64_t H, int64_t W, int64_t sy, int64_t sx,
                                int64_t* out_host /* [R][nch H W] */);
int fhesi_slots_lattice_columns_dev(fhesi_slots* s, const int64_t* M_dev /* [R][nch (H/sy) (W/sx)] */, int64_t R, int64_t nch, int64_t H, int64_t W, int64_t sy, int64_t sx,
                                    int64_t* out_dev /* [R][nch H W] */);

/* ---- polynomial activations on packed slots: y = f(x) = sum_{k <= d} c_k x^k slot by slot, the non-linear step between two linear layers (DESIGN.md 9a;
 * tests/poly_model.py is the normative statement of the plan and of the schedule).
 * fhesi_ct_lin_comb_dev: for every group g,  out[g] = Reduce_logQ( sum_{t in [seg[g], seg[g+1])} coef[t] * pool[a_idx[t]] + konst[g] ) on unscaled two-part
 *   ciphertexts; the constant enters by the rule of Ciphertext += ZZX (Ciphertext.cpp:147-156): floor((konst[g] << logQ) / p) is added to coefficient 0 of
 *   part 0.  DEFINED as, and bit for bit equal to: a copy of each operand, fhesi_ct_mul_long_dev(coef[t]), fhesi_ct_add_dev per term, fhesi_ct_add_const_dev
 *   with the polynomial (konst[g], 0, .., 0) -- all exact modulo 2^logQ, so the order of the terms cannot matter.  One kernel launch reads every term once and
 *   writes once; there is no bound on the terms of a group.  An empty group gives the trivial ciphertext of its constant (the zero ciphertext for konst NULL or
 *   konst[g] = 0).  coef and konst: any int64.  The host arrays are read before the call returns.
 *   REFUSED before any launch, the condition named, the context usable: out overlapping pool; an index outside the pool; seg not starting at 0 or
 *   decreasing; nlimbs outside 1 .. 32 or not holding logQ; p < 2; a null argument where terms exist.
 * fhesi_poly_eval_plan (host only): the Paterson-Stockmeyer plan of a DENSE polynomial of degree 1 .. 4096 with B baby powers x^1 .. x^B and the giants
 *   x^(gB), g = 2 .. G - 1, G = floor(degree / B) + 1.  nks key switches = (B - 1) + max(G - 2, 0) + [a group g >= 1 has terms], nprod products = the same
 *   powers + one per such group, depth = ceil(log2 B) + ceil(log2 max(G - 1, 1)) + [a group g >= 1 has terms].  baby = 0 picks the B of least nks, of
 *   equal nks the smaller depth, of equal depth the larger B (degree 15: B = 4, G = 4, 6 key switches and depth 5 where Horner takes 14 and 14).  Any
 *   output pointer may be NULL.
 * fhesi_ct_poly_eval_dev: out[i] = f(in[i]), f given by coef[0 .. degree] (any int64; reduced modulo p, scalar factors by their centred representative in
 *   (-p/2, p/2], constants by the one in [0, p)).  DEFINED as, and word for word equal to, this composition of the entry points above:
 *   powers x^j = MulRelin(x^ceil(j/2), x^floor(j/2)) for j = 2 .. B and x^(gB) = MulRelin(x^(ceil(g/2) B), x^(floor(g/2) B)) for g = 2 .. G - 1, every level
 *   ceil(log2 .) ONE fhesi_ct_mul_sum_relin_dev of single-term groups over all items (all powers, whatever the zero pattern of the coefficients);
 *   u_g = lin_comb(c_(gB+j) x^j, 1 <= j < B, non-zero terms only; konst c_(gB)) for every g >= 1 that has such a term, all of them ONE fhesi_ct_lin_comb_dev;
 *   W = ONE fhesi_ct_mul_sum_relin_dev with one group per item holding the pairs (u_g, x^(gB)) in ascending g: one key switch whatever G is;
 *   y = lin_comb(group 0's terms in ascending j, then (c_(gB), x^(gB)) of the groups g >= 1 that are a non-zero constant alone, then (1, W); konst c_0).
 *   Everything between in and out lives in the workspace, in chunks of ciphertexts.  REFUSED before any launch: what fhesi_ct_mul_sum_relin_dev refuses
 *   (a matrix of another context, of another digit count or without 3 source components, a decompSize outside 1 .. 7, nlimbs not holding logQ); a degree
 *   outside 1 .. 4096; baby outside 0 .. degree; p outside [2, 2^62); out overlapping in; null arguments.
 * NOT HERE: per-slot coefficients (a prepared plaintext per power); several polynomials of one input sharing its powers; pruning the powers a zero pattern
 *   leaves unused; a form of the C++ mirror; a C-ABI form over a slot basis (the Python binding runs one call per channel). */
int fhesi_ct_lin_comb_dev(fhesi_ctx* ctx, int32_t logQ, uint64_t p, const uint64_t* pool_dev /* [npool][2][phi(m)][nlimbs] */, int64_t npool, int32_t nlimbs,
                          const int32_t* a_idx, const int64_t* coef /* per term */, const int32_t* seg /* [ngroups + 1] */, const int64_t* konst /* [ngroups] or NULL */,
                          int64_t ngroups, uint64_t* out_dev /* [ngroups][2][phi(m)][nlimbs] */);
int fhesi_poly_eval_plan(int32_t degree, int32_t baby /* 0 = choose */, int32_t* B, int32_t* G, int32_t* nprod, int32_t* nks, int32_t* depth);
int fhesi_ct_poly_eval_dev(fhesi_ctx* ctx, const fhesi_ksk* k /* s^2 -> s, 3 source components */, int32_t logQ, uint64_t p, int32_t decomp_bytes,
                           const int64_t* coef /* [degree + 1] */, int32_t degree, int32_t baby /* 0 = the planner's */, const uint64_t* in_dev, int32_t nlimbs,
                           int64_t count, uint64_t* out_dev);

/* ---- multi-GPU: independent ciphertexts are data-parallel, every GPU holds the context tables and a replica of
 * the key-switch matrices; RCCL collectives run on the context's stream.  librccl is loaded on first use (no RCCL needed on one GPU).
 * fhesi_comm_init_all: one process, one host thread per GPU -- ncclCommInitAll over `devices`, comms_out[r] is rank r's handle.
 *   (If `devices` repeats a GPU -- RCCL refuses that -- the group is a "loopback" group that moves the same bytes with device copies
 *   and host barriers between the calling threads: for exercising N > 1 host logic on a single-GPU box, never for measurements.)
 * fhesi_comm_from_rccl: wraps a caller-owned ncclComm_t (process-per-GPU launchers: ncclCommInitRank); not destroyed by us.
 * Collective calls must be made by every rank of the group (from its own thread or process), like the RCCL calls they are. */
int fhesi_comm_init_all(int32_t ndev, const int32_t* devices, fhesi_comm** comms_out);
int fhesi_comm_from_rccl(void* nccl_comm, fhesi_comm** out);
int fhesi_comm_destroy(fhesi_comm* comm);
int32_t fhesi_comm_rank(const fhesi_comm* comm);
int32_t fhesi_comm_size(const fhesi_comm* comm);
/* the set-up collective of the data-parallel model: rank `root`'s key-switch matrix (KeySwitchSI::keySwitchMatrix, FHE-SI.cpp:206-208;
 * 297 MiB at the metric ring) into every rank's replica `k` (same shape on every rank); derived tables are rebuilt on the receivers */
int fhesi_ksk_broadcast(fhesi_ksk* k, fhesi_comm* comm, int32_t root);
int fhesi_comm_broadcast_dev(fhesi_ctx* ctx, fhesi_comm* comm, void* buf_dev, size_t bytes, int32_t root);   /* any HBM buffer (bytes % 8 == 0) */
/* exchange of sharded wave outputs (Matrix<Ciphertext> waves, Matrix.cpp:150-174): rank r produced the words
 * [offsets_words[r], offsets_words[r+1]) of base_dev; afterwards every rank holds all of them (one grouped broadcast per producer) */
int fhesi_comm_exchange(fhesi_ctx* ctx, fhesi_comm* comm, uint64_t* base_dev, const int64_t* offsets_words);
/* the same exchange split for overlap with compute (the waves of Regression::Regress, Regression.h:102-149 over Matrix.cpp:182-263: a
 * wave's outputs are read by the NEXT wave only).  _begin enqueues the exchange on the communicator's own stream behind everything already
 * on the context's stream and returns without waiting for the GPU -- the context's stream goes on with the next chunk of the wave;
 * _end returns when every exchange begun since the last _end has landed.  All ranks call _begin for the same exchanges in the same order. */
int fhesi_comm_exchange_begin(fhesi_ctx* ctx, fhesi_comm* comm, uint64_t* base_dev, const int64_t* offsets_words);
int fhesi_comm_exchange_end(fhesi_ctx* ctx, fhesi_comm* comm);
/* exact all-reduce of partial scaled-up sums held by the ranks (Ciphertext::operator+= on scaled-up ciphertexts is linear,
 * Ciphertext.cpp:135-142): rows_dev [count][L][phi(m)] <- (sum over ranks) mod q_i; at most 16 ranks (64-bit partial sums of 60-bit residues) */
int fhesi_comm_allreduce_rows(fhesi_ctx* ctx, fhesi_comm* comm, uint64_t* rows_dev, int64_t count);

/* plain device-memory helpers so C callers need no HIP headers */
int fhesi_dev_alloc(fhesi_ctx* ctx, size_t bytes, void** out_dev);
int fhesi_dev_free(fhesi_ctx* ctx, void* dev);
int fhesi_dev_upload(fhesi_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int fhesi_dev_download(fhesi_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int fhesi_dev_copy(fhesi_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);    /* e.g. RCCL receive buffer -> key matrix */

#ifdef __cplusplus
}
#endif
#endif /* FHESI_HIP_H_ */
