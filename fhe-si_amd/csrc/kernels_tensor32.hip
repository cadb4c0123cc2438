// kernels_tensor32.hip -- the tensor half of the fused multiplication (Ciphertext::operator*=, Ciphertext.cpp:167-218) over primes below 2^30.
//
// tProd = (p a) (x) b is an INTEGER polynomial triple: its coefficients are bounded by 2 n (p 2^(64 nl - 1)) 2^(64 nl - 1), far below half the
// chain product, and ScaleDown only keeps round(x / 2^logQ) mod 2^logQ of every coefficient x.  Inside fhesi_ct_mul_relin_batch_dev the
// DoubleCRT of tProd is never visible, so the integers may be computed modulo ANY product of primes that exceeds the bound: here the NP
// largest primes below 2^30 that are 1 mod 2^15 (35 of them at the metric shape, 1050 bits, where the chain has 18 primes of 60 bits).
// Same bytes per row set, a quarter of the multiplier work per butterfly, and the residues are 30-bit numbers, which lets the two
// conversions run on single v_mad_u64_u32 chains:
//   rns32_reduce_kernel   coefficient (two's complement, 2 nl words of 32 bits) -> residues below 4p: 4 + 3 + 3 + ... products of
//                         x_k (2^(32k) s mod p) per 64-bit accumulator, folded through 2^32 mod p, one Barrett step at the end
//   ntt32_fwd_kernel3     the rows' forward transforms (ntt32_core.inc)
//   ntt32_inv_kernel3<.., TENSOR>   element-wise products formed in the loader of the inverse transform (no tensor kernel, no rows
//                         written in between)
//   crt32_scale_kernel    x = sum_i y_i M_i - kappa M with y_i = r_i (M/p_i)^-1 mod p_i and M_i = M/p_i cut into words of 28 bits: y_i M_i[l] < 2^58,
//                         so the NP + 1 terms of a word accumulate in 64 bits without carries; kappa from a 26-bit fixed-point sum.  Rows of
//                         2^14 arrive as y_i (T32_ROWS_CRT): the inverse transform's closing constants are (M/p_i)^-1 / n and that times the last
//                         twiddle (T32Primes, per configuration), so the kernel starts at the multiply-adds.  Only the words from
//                         28 * 16 = 448 bits upwards are formed -- the dropped part is below 64 * 2^30 * 2^448 = 2^484 and can change
//                         round(x / 2^512) only when bits 484..511 of x + 2^511 are all ones (2^-27 per coefficient: about one workgroup in
//                         three launches of 1024 products): those workgroups are flagged, listed and redone with every word (EXACT on a small
//                         grid that walks the list), the pattern of crt_sum_kernel.
//   crt32_mfma_kernel     the same fast pass at rows of 2^14, logQ = 512 as an int8 matrix product (option crt32_mfma): the window of the constants
//                         in balanced bytes is operand A, the residues' bytes operand B, fifteen v_mfma_i32_32x32x32_i8 per 32 coefficients and a
//                         carry pass over nine words per lane -- the same integer, the same limbs, the same flags (crt32_bytes.h).
// Rows of 2^15 (n = 2^15, the stress shape: 70 primes for logQ = 1024): the head stage of the forward transform is taken inside
// rns32_reduce_kernel<NL, true> (a thread converts coefficients j and j + 2^14 and stores the two butterfly outputs into the two sub-rows),
// the tail of the inverse inside crt32_scale_kernel (its first multiplication takes (A + B) or (A - B) with the tail constant folded into
// the CRT constant), so a row still passes through exactly one forward and one inverse kernel.  With more than 62 primes the CRT words
// are 26 bits wide (71 terms below 2^56 per 64-bit accumulator).
// The reference's safe-prime rings (m = 2q', Bluestein rows in the reference and in the chain path) take the same route as LINEAR
// convolutions: phi(m) coefficients zero-padded into rows of 2^14, products of degree < 2 phi(m) - 1, and the reduction modulo
// X^q' + 1 and Phi_m -- out_j = S_j - S_(j+q') - (-1)^j S_(q'-1), linear, so it is applied to the residues in the loader of the CRT
// kernel (crt32_scale_generic_kernel: any logQ, words at run-time positions through LDS).  Sums of products per group
// (fhesi_ct_mul_sum_relin_dev: Matrix products inside Regression) are formed in evaluation form by tensor_sum32_kernel.
// Padded rows of 2^16 take their second head stage in rns32_reduce_kernel<NL, 2> and their tails as a pass of their own; rows of 2^17 .. 2^20
// (round 6: every m = p - 1 below 2^20) are converted as plain zero-padded rows and take head AND tail stages as passes of their own
// (ntt32_headS_kernel / ntt32_tailS_kernel, ntt32_core.inc); the CRT kernel then folds from whole rows.
// fhesi_ct_mul_dev keeps the reference chain (its rows ARE visible).  Option tensor32 = 0 keeps the chain in the fused pipeline too; option
// tensor_bits = 29 takes the primes below 2^29 (fewer range steps in the row transforms, one or two primes more: measured a tie).
// Host tables: ring32_tables.h builds them all -- hm::ring32_build the transform tables (t32_ring; the key switch's four primes go through the
// same builder), hm::conv32_build the conversion tables of a configuration (t32_config) -- and tests/test_ring32_tables.py checks them on the CPU.
#include "fhesi_internal.h"
#include "lin_fold.h"
#include "ntt32_core.inc"
#include "crt32_bytes.h"
#include <cmath>

// one (lift, limb count, logQ, prime count) configuration: the conversion tables
struct T32Config {
  u64 lift = 0;
  int nl = 0, logQ = 0, NP = 0, R = 28, WT = 0;
  bool generic = false;              // crt32_scale_generic_kernel (any logQ, fold) instead of the compiled shapes
  T32Primes pr;                      // pr.closing: the form this configuration's inverse leaves its rows in, and the only one its CRT kernels take (t32_crt)
  u32* d_rns = nullptr;              // [2][NP][2 nl + 6]: (s 2^(32k) mod p) k < 2 nl, -(s 2^(64 nl)) mod p, 2^32 mod p, floor(2^61 / p), p, head twiddle (w, w');  s = lift (class 0) or 1
  Tw32* d_cinv = nullptr;            // [NP][2] (M / p_i)^-1 mod p_i  [times 1/2 | times psi^-brv(1) / 2: the tail of a 2^15-point inverse]   (rows of 2^14: not read, pr.ninv carries it)
  u32* d_inv57 = nullptr;            // [NP] floor(2^57 / p_i)
  u32* d_Mw = nullptr;               // [NP + 1][WT]: M_i in words of R bits; row NP = 2^(R WT) - M
  u32* d_bytes = nullptr;            // crt32_mfma_kernel's operand A (crt32_bytes.h): [3][5][64][4]; null where the shape does not qualify
  ~T32Config() { hipFree(d_rns); hipFree(d_cinv); hipFree(d_inv57); hipFree(d_Mw); hipFree(d_bytes); }
};
struct fhesi_tensor32 {
  int S = 0;                         // rows of 2^14 << S
  int bits = 30;                     // 30: the largest primes below 2^30; 29: below 2^29 (option tensor_bits: one or two primes more, 6 of 14 / 7 of 13 range steps per row transform)
  // what the device tables were built for, committed after them (t32_ring): k.primes, largest first, and per prime the values the configurations
  // derive their constants from -- head (psi^brv(1): S = 1), head1 (psi^brv(2), psi^brv(3): S = 2), tail (psi^-brv(1)), last (S = 0: the twiddle of
  // the inverse's last stage before the 1/n went in)
  hm::Ring32Consts k;
  Ring32Dev tab;                     // [primes][2^S][2^14] forward and inverse tables, and the constants of the stand-alone passes (S >= 2)
  std::vector<T32Config*> cfgs;
  T32Config* cur = nullptr;          // the configuration of the running sum (tensor32_sum_begin)
};

void tensor32_free(fhesi_ctx* ctx) {
  fhesi_tensor32* x = ctx->tensor32;
  if (!x) return;
  for (T32Config* c : x->cfgs) delete c;
  x->tab.release();
  delete x;
  ctx->tensor32 = nullptr;
}

// the two compiled shapes of crt32_scale_kernel, and the run-time form
static constexpr int T32_WT_512 = 38, T32_R_512 = 28;        // logQ = 512: words of 28 bits (up to 62 primes), 1064 bits per table row
static constexpr int T32_WT_1024 = 82, T32_R_1024 = 26;      // logQ = 1024: words of 26 bits (up to 72 primes), 2132 bits per table row
static constexpr int T32_GEN_NW = 24, T32_GEN_NWX = 40;      // generic kernel: words formed in the first pass / in the exact pass (logQ <= 512)
static constexpr int T32_NP_28 = 62, T32_NP_26 = T32_MAXP;   // the most primes a table of 28-bit / 26-bit words is built for (t32_plan_search)
// The first word the non-exact CRT pass forms.  A dropped word position l < J0 holds NP + 1 terms y_i M_i[l] (and kappa N[l]) with y_i, kappa
// < 2^30 and the table word < 2^R, so everything below word J0 is less than (np_max + 1) 2^30 2^(R J0) <= 2^(tb + 30 + R J0), tb = bits of np_max + 1.
// J0 is the largest value that keeps this at or below 2^(logQ - T32_WIN): the formed value F <= x < F + 2^(logQ - T32_WIN) then rounds like x unless
// one carry into bit logQ - T32_WIN runs through to bit logQ - 1, i.e. unless bits logQ-28 .. logQ-1 of F + 2^(logQ-1) are all ones (the undecided test).
// (tb >= 6 at both bounds, so R J0 <= logQ - 64 follows and the rounding limb of bits logQ-64 .. logQ-1 is always formed: asserted in the kernel.)
static constexpr int T32_WIN = 28;
__host__ __device__ constexpr int t32_j0(int LQ, int R, int np_max) {
  int tb = 0;
  while ((1 << tb) < np_max + 1) ++tb;
  return LQ < T32_WIN + 30 + tb ? 0 : (LQ - T32_WIN - 30 - tb) / R;
}
static_assert(t32_j0(512, T32_R_512, T32_NP_28) == 16 && t32_j0(1024, T32_R_1024, T32_NP_26) == 36, "the compiled windows: words from bit 448 / 936");
// undecided: bits logQ-28 .. logQ-1 of the rounding limb G (bits logQ-64 .. logQ-1 of F) read 0111...1, i.e. all ones once the rounding bit is added
__device__ __forceinline__ int t32_undecided(u64 G) { return (G >> (64 - T32_WIN)) == (((u64)1 << (T32_WIN - 1)) - 1) ? 1 : 0; }

// The matrix-core form of the fast pass (crt32_mfma_kernel): rows of 2^14, logQ = 512, the 21 words of 28 bits from bit 448 -- the window
// crt32_scale_kernel<512, false, 28, 38, 0> forms.  Its depth holds 40 slots of four bytes; the first four depth steps
// hold primes only, so at least 32 primes, and kappa and the constant need two slots (35 primes below 2^30 and 36 below 2^29 at the metric ring;
// sums of products take one or two more).
static constexpr int T32_MFMA_NW = (2 * 512 + T32_R_512 - 1) / T32_R_512 - t32_j0(512, T32_R_512, T32_NP_28);
static_assert(T32_MFMA_NW == 21 && T32_R_512 * t32_j0(512, T32_R_512, T32_NP_28) + 8 * hm::C32B_COLS == 2 * 512, "72 byte columns from bit 448 reach bit 1024");
static constexpr size_t T32_MFMA_MIN_WG = 8 * 2048;
static bool t32_mfma_shape(bool generic, int logQ, int S, int NP) { return !generic && logQ == 512 && S == 0 && NP >= 32 && NP + 2 <= hm::C32B_SLOTS; }
// The redo list of a fast pass, behind the flags in workspace slot 6: word 0 counts the flagged workgroups, their indices follow from word
// T32_LIST_HDR.  More than T32_LIST_CAP flagged workgroups (crafted inputs only: about one in three launches of 1024 products flags one) are
// counted but not listed, and the redo pass then walks the flags instead.
static constexpr u32 T32_LIST_HDR = 4, T32_LIST_CAP = 4092, T32_REDO_GRID = 256;
__device__ __forceinline__ void t32_flag(unsigned char* __restrict__ flags, u32* __restrict__ list, u32 wg, int any) {
  flags[wg] = any ? 1 : 0;
  if (any) {
    const u32 at = atomicAdd(list, 1u);
    if (at < T32_LIST_CAP) list[T32_LIST_HDR + at] = wg;
  }
}
__global__ void t32_list_clear_kernel(u32* __restrict__ list) { if (threadIdx.x == 0) list[0] = 0; }

struct T32Plan { int NP = 0; bool generic = false; };
// The number of primes the tensor half needs (0: this shape does not run through it).
//   |x| < 2^TB with TB = 2 (logQ - 1) + bits(p) + log2(coefficients) + 1 [+ log2(terms per sum)] [+ 2: the three-term fold of the
//   safe-prime rings];  M > 2^(TB + 3) keeps x/M below 1/8 (kappa is then decided by a coarse fixed-point sum), and the chain product must
//   exceed 2^(TB + 1) so that the reference's own centred integers are these same integers.
static T32Plan t32_plan_search(const fhesi_ctx* ctx, u64 p, int nlimbs, int logQ, i64 gmax, std::vector<u32>* primes);
// (the search tests a few hundred candidates for primality: a tenth of a millisecond, which a caller of single multiplications would pay
// twice per call -- so the answer is kept per (lift, limbs, logQ, bits of the group size, option tensor32))
static T32Plan t32_plan(const fhesi_ctx* ctx, u64 p, int nlimbs, int logQ, i64 gmax, std::vector<u32>* primes) {
  int gbits = 0;
  while (((i64)1 << gbits) < gmax) ++gbits;
  auto& memo = const_cast<fhesi_ctx*>(ctx)->t32_memo;          // (a context serves one host thread at a time)
  const std::vector<long long> key{(long long)p, nlimbs, logQ, gbits, ctx->opt.tensor32, ctx->opt.tensor_bits};
  auto it = memo.find(key);
  if (it == memo.end()) {
    std::vector<u32> pr;
    const T32Plan pl = t32_plan_search(ctx, p, nlimbs, logQ, gmax, &pr);
    it = memo.emplace(key, std::make_pair(pl.NP * 2 + (pl.generic ? 1 : 0), std::move(pr))).first;
  }
  if (primes) *primes = it->second.second;
  T32Plan pl;
  pl.NP = it->second.first >> 1; pl.generic = it->second.first & 1;
  return pl;
}
static T32Plan t32_plan_search(const fhesi_ctx* ctx, u64 p, int nlimbs, int logQ, i64 gmax, std::vector<u32>* primes) {
  T32Plan pl;
  if (!ctx->opt.tensor32 || p < 2 || nlimbs < 1 || nlimbs > 16 || 64 * nlimbs < logQ || gmax < 1) return pl;
  const bool lin = ctx->lin_q != 0;
  if (!lin && !(ctx->pow2 && (ctx->logn == A32_LOGN || ctx->logn == A32_LOGN + 1))) return pl;
  const int lg = lin ? ctx->lin_lg : ctx->logn;              // rows of 2^lg
  const bool compiled = !lin && (logQ == 512 || logQ == 1024);
  if (!compiled && (logQ < 64 || logQ > 512)) return pl;     // the generic CRT kernel: logQ <= 512 (rows of 2^14, or two sub-rows of a 2^15-point row)
  int pbits = 0, gbits = 0, cbits = 0;
  while (pbits < 64 && (p >> pbits)) ++pbits;
  while (((i64)1 << gbits) < gmax) ++gbits;
  while (((i64)1 << cbits) < ctx->phim) ++cbits;
  // (operands are centred residues modulo 2^logQ, as every reference Ciphertext holds them: Ciphertext.cpp reduces after each operation)
  const double TB = 2.0 * (logQ - 1) + pbits + cbits + 1 + gbits + (lin ? 2 : 0);
  double chain = 0;
  for (int i = 0; i < ctx->L; ++i) chain += std::log2((double)ctx->q[i]);
  if (chain < TB + 1.5) return pl;
  const int maxp = (compiled && logQ == 1024) ? T32_NP_26 : T32_NP_28;
  // Primes of 30 bits keep M above 2^(TB + 3.5) (rounds 2-5).  Primes below 2^29 (option tensor_bits = 29) make do with 2^(TB + 1.5): |x / M| < 0.36
  // and the fixed-point sum behind kappa is short by less than NP 2^-25, so round(sum y_i / p_i) is still kappa -- 36 primes at the metric ring
  // (1043.5 bits for TB = 1042), 72 at the stress ring.
  const int pb = ctx->opt.tensor_bits == 29 ? 29 : 30;
  const double margin = pb == 29 ? 1.5 : 3.5;
  double have = 0;
  int np = 0;
  for (u64 k = ((u64)1 << (pb - 1 - lg)) - 1; k > ((u64)1 << (pb - 2 - lg)) && have < TB + margin; --k) {
    const u64 cand = (k << (lg + 1)) + 1;
    if (cand > ((u64)1 << pb) - ((u64)1 << 15) + 1 || !hm::is_prime(cand)) continue;
    if (np == maxp) return pl;
    if (primes) primes->push_back((u32)cand);
    have += std::log2((double)cand);
    ++np;
  }
  if (have < TB + margin) return pl;
  // all of M inside the table row
  const double room = compiled ? (logQ == 512 ? (double)T32_R_512 * T32_WT_512 : (double)T32_R_1024 * T32_WT_1024) : 28.0 * ((have + 8) / 28 + 2);
  if (have > room - 8) return pl;
  pl.NP = np;
  pl.generic = !compiled;
  return pl;
}
bool tensor32_applies(const fhesi_ctx* ctx, u64 p, int nlimbs, int logQ) { return t32_plan(ctx, p, nlimbs, logQ, 1, nullptr).NP > 0; }
bool tensor32_sum_applies(const fhesi_ctx* ctx, u64 p, int nlimbs, int logQ, i64 gmax) {
  return t32_plan(ctx, p, nlimbs, logQ, gmax, nullptr).NP > 0;
}

// transform tables of the first `want` primes (grown on demand; a growth waits for the streams)
static int t32_ring(fhesi_ctx* ctx, const std::vector<u32>& primes) {
  fhesi_tensor32* x = ctx->tensor32;
  const int pb = !primes.empty() && primes[0] < (1u << 29) ? 29 : 30;
  if (x && x->bits != pb) {              // (option tensor_bits toggled on a live context: other primes, other tables)
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->lane_stream) HIP_TRY(hipStreamSynchronize(ctx->lane_stream));
    tensor32_free(ctx);
    x = nullptr;
  }
  if (!x) { x = new fhesi_tensor32(); x->S = (ctx->lin_q ? ctx->lin_lg : ctx->logn) - A32_LOGN; x->bits = pb; ctx->tensor32 = x; }
  if (x->k.primes.size() >= primes.size()) return 0;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (ctx->lane_stream) HIP_TRY(hipStreamSynchronize(ctx->lane_stream));
  if (x->S < 0 || x->S > 6) FHESI_FAIL("tensor32: rows of 2^%d", A32_LOGN + x->S);
  hm::Ring32Tables t;                    // (ring32_tables.h: the builder the key switch's four primes go through as well)
  if (!hm::ring32_build(primes, x->S, t)) FHESI_FAIL("tensor32: no 2n-th root");
  FHESI_TRY(x->tab.upload(t));           // (a failure leaves the old tables AND the old prime list in force)
  x->k = std::move(t.k);
  return 0;
}

static int t32_config(fhesi_ctx* ctx, u64 lift, int nlimbs, int logQ, i64 gmax, T32Config** out) {
  std::vector<u32> primes;
  const T32Plan pl = t32_plan(ctx, lift, nlimbs, logQ, gmax, &primes);
  if (!pl.NP) FHESI_FAIL("tensor32: shape not supported");
  FHESI_TRY(t32_ring(ctx, primes));
  fhesi_tensor32* x = ctx->tensor32;
  for (T32Config* c : x->cfgs)
    if (c->lift == lift && c->nl == nlimbs && c->logQ == logQ && c->NP == pl.NP && c->generic == pl.generic) { *out = c; return 0; }
  const int NP = pl.NP, S = x->S;
  double have = 0;
  for (int a = 0; a < NP; ++a) have += std::log2((double)primes[a]);
  const int R = pl.generic ? 28 : (logQ == 512 ? T32_R_512 : T32_R_1024);
  const int WT = pl.generic ? (int)((have + 8) / 28) + 2 : (logQ == 512 ? T32_WT_512 : T32_WT_1024);
  const hm::Conv32Tables h = hm::conv32_build(x->k, NP, lift, nlimbs, R, WT);      // (ring32_tables.h)
  T32Config* c = new T32Config();
  c->lift = lift; c->nl = nlimbs; c->logQ = logQ; c->NP = NP; c->generic = pl.generic; c->R = R; c->WT = WT;
  for (int a = 0; a < NP; ++a) {
    const Tw32 cn = h.closing[2 * a], cw = h.closing[2 * a + 1];
    c->pr.p[a] = primes[a]; c->pr.mu61[a] = h.mu61[a]; c->pr.ninv[a] = cn.w; c->pr.ninv_p[a] = cn.wp; c->pr.ninv_w[a] = cw.w; c->pr.ninv_w_p[a] = cw.wp;
  }
  c->pr.closing = S ? T32_ROWS_PLAIN : T32_ROWS_CRT;
  bool ok = a32_upload(&c->d_rns, h.rns) && a32_upload(&c->d_cinv, h.cinv) && a32_upload(&c->d_inv57, h.inv57) && a32_upload(&c->d_Mw, h.Mw);
  // the same window of the same table rows as balanced bytes (crt32_bytes.h): the matrix-core form of the fast pass
  if (ok && t32_mfma_shape(pl.generic, logQ, S, NP)) ok = a32_upload(&c->d_bytes, hm::crt32_bytes_build(h.Mw.data(), NP, WT, R, t32_j0(512, T32_R_512, T32_NP_28), T32_MFMA_NW).aop);
  if (!ok) { delete c; FHESI_FAIL("tensor32: table upload failed"); }
  x->cfgs.push_back(c);
  *out = c;
  return 0;
}

// ---------------------------------------------------------------------------------------------- big integer -> residues
// PAIRED: a, b: [count][2][n_src][NL] two's complement coefficients; rows [count][4][NP][nrow] (a0, a1, b0, b1).
// otherwise: na2 polynomials of a (class 0: lifted by p), then those of b; rows [polys][NP][nrow].  Values below 4p; positions from
// n_src upwards (linear-convolution rings) are zero.
// HEAD (rows of 2^15): a thread takes coefficients j and j + 2^14 and stores  x + w y  and  x + 2p - w y  into sub-rows 0 and 1 of the row
// (the head stage of the 2^15-point transform, w = psi^brv(1)).
// a * b_uniform + c in one v_mad_u64_u32, the wave-uniform factor taken from its scalar register
__device__ __forceinline__ u64 mad64s(u32 a, u32 b_uniform, u64 c) {
  u64 r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "s"(b_uniform), "v"(c));
  return r;
}
template <int NL>
__device__ __forceinline__ u32 rns32_one(const u32 (&x)[2 * NL], u32 neg, const u32* __restrict__ t) {
  const u32 r32 = t[2 * NL + 1], mu = t[2 * NL + 2], p = t[2 * NL + 3];
  // products below 2^62 - 2^47: four fit a 64-bit accumulator, three on top of a folded value (below 2^62 + 2^32)
  u64 acc = 0;
  int room = 4;
  // ONE dependency chain of v_mad_u64_u32 (the table words from their scalar registers): written as plain C++ the compiler splits the sum into
  // five independent groups and joins them with 64-bit adds and moves -- 38 instructions per prime where the chain needs 32; the latency
  // of the chain is covered by the other waves (34 registers: full occupancy)
#pragma unroll
  for (int k = 0; k < 2 * NL; ++k) {
    if (room == 0) { acc = mad64s((u32)(acc >> 32), r32, (u64)(u32)acc); room = 3; }
    acc = mad64s(x[k], t[k], acc);
    --room;
  }
  acc = mad64s(neg, t[2 * NL], acc);                          // (neg is 0 or 1: the two's complement correction without a branch)
  acc = mad64s((u32)(acc >> 32), r32, (u64)(u32)acc);       // below 2^32 r32 + 2^32
  // The primes of the tensor half are the largest below 2^30, so 2^32 mod p = 4 (2^30 - p) is a small number (below 2^26 for the 72 largest
  // primes that are 1 mod 2^16): one fold already leaves the total below 2^61.  Any other prime takes the second fold (a wave-uniform branch).
  // (primes of 29 bits: sh = 28 -- one fold leaves the total below 2^60 when 2^32 mod p = 8 (2^29 - p) is below 2^27, the second fold otherwise)
  const u32 sh = t32_shift(p);
  if (r32 >= (1u << (sh - 1))) acc = mad64s((u32)(acc >> 32), r32, (u64)(u32)acc);       // below 2^(32 + sh)
  const u32 q = __umulhi((u32)(acc >> sh), mu);        // at most 2 below floor(acc / p)
  return (u32)acc - q * p;                             // below 3p
}
// HEAD: 0 = plain rows (or, dup, padded rows of 2^15: the value goes to both sub-rows); 1 = rows of 2^15 with the head stage x +- w y of
// coefficients j, j + 2^14; 2 = PADDED rows of 2^16 (fewer than 2^15 coefficients): the first head stage is a duplication, the second the same
// x +- w y with the half's twiddle -- sub-rows 0, 1: psi^brv(2), sub-rows 2, 3: psi^brv(3); coefficients from n_src upwards are zero
template <int NL, int HEAD, bool PAIRED>
__global__ void __launch_bounds__(256) rns32_reduce_kernel(const u64* __restrict__ a, const u64* __restrict__ b, i64 na2, i64 n_src, i64 nrow, u32* __restrict__ rows, int NP,
                                                            const u32* __restrict__ tab, const int* __restrict__ idx_a = nullptr, const int* __restrict__ idx_b = nullptr, int dup = 0) {
  __shared__ __attribute__((aligned(16))) u64 sl[NL * 256];       // [NL][256]
  const i64 poly = blockIdx.y;
  int cls;
  const u64* __restrict__ src;
  if (PAIRED) {      // (idx_a / idx_b: operand ct of the a's / b's is ciphertext idx[ct] of the buffer -- pool indices of a wave of single products)
    const i64 ct = poly >> 2; const int jp = (int)(poly & 3); cls = jp >> 1;
    const i64 cs = idx_a ? (i64)(cls ? idx_b : idx_a)[ct] : ct;
    src = (cls ? b : a) + (cs * 2 + (jp & 1)) * n_src * NL;
  }
  else { cls = poly >= na2; src = cls ? b + (poly - na2) * n_src * NL : a + poly * n_src * NL; }
  const i64 j0 = (i64)blockIdx.x * 256;
  const int tid = threadIdx.x;
  u32* __restrict__ o = rows + poly * NP * nrow + j0 + tid;
  // dup (padded rows of 2^15 on a linear-convolution ring: the polynomial's upper half is zero, so the head stage x +- w 0 leaves x in both
  // sub-rows): every value is written to sub-row 1 as well
  // few polynomials (small batches): the primes are split over gridDim.z so that the launch fills the chip -- with one workgroup per CU
  // every thread walked the 35 primes behind 35 exposed scalar-load latencies (21 us for one ciphertext)
  const int i_first = (int)((i64)blockIdx.z * NP / gridDim.z), i_last = (int)((i64)(blockIdx.z + 1) * NP / gridDim.z);
  if (j0 >= n_src) {                                             // (whole block in the zero padding)
    // (every sub-row this block owns: a ring needing rows of 2^16 has more than 2^14 coefficients and never comes here with HEAD = 2, the
    // FHESI_LIN_LG test hook on a small ring does)
    for (int i = i_first; i < i_last; ++i) {
      o[(i64)i * nrow] = 0;
      if (dup || HEAD != 0) o[(i64)i * nrow + A32_N] = 0;
      if constexpr (HEAD == 2) { o[(i64)i * nrow + 2 * A32_N] = 0; o[(i64)i * nrow + 3 * A32_N] = 0; }
    }
    return;
  }
  const i64 avail = (n_src - j0) * NL;                           // words of this block's 256 coefficients that exist
  u32 x[2 * NL], x1[HEAD != 0 ? 2 * NL : 1];
  const u64* __restrict__ sblk = src + j0 * NL;
  if (avail >= 256 * NL) {                                       // (uniform: every block but the last one of a padded row)
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int e = it * 256 + tid;
      sl[(e % NL) * 256 + e / NL] = sblk[e];
    }
  } else {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int e = it * 256 + tid;
      sl[(e % NL) * 256 + e / NL] = e < avail ? sblk[e] : 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NL; ++k) { const u64 v = sl[k * 256 + tid]; x[2 * k] = (u32)v; x[2 * k + 1] = (u32)(v >> 32); }
  if constexpr (HEAD != 0) {
    __syncthreads();
    const i64 avail1 = HEAD == 2 ? (n_src - (j0 + A32_N)) * NL : (i64)256 * NL;      // (padded rows: the second block may lie partly or wholly in the padding)
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int e = it * 256 + tid;
      sl[(e % NL) * 256 + e / NL] = e < avail1 ? src[(j0 + A32_N) * NL + e] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NL; ++k) { const u64 v = sl[k * 256 + tid]; x1[2 * k] = (u32)v; x1[2 * k + 1] = (u32)(v >> 32); }
  }
  const u32 neg = x[2 * NL - 1] >> 31;
  u32 neg1 = 0;
  if constexpr (HEAD != 0) neg1 = x1[2 * NL - 1] >> 31;
  constexpr int STRIDE = (2 * NL + 8 + 7) & ~7;
#pragma unroll 2
  for (int i = i_first; i < i_last; ++i) {
    const u32* __restrict__ t = tab + ((i64)cls * NP + i) * STRIDE;
    const u32 r0 = rns32_one<NL>(x, neg, t);
    if constexpr (HEAD == 0) {
      __builtin_nontemporal_store(r0, &o[(i64)i * nrow]);                  // (a zero coefficient gives 0: the padding inside a partial block)
      if (dup) __builtin_nontemporal_store(r0, &o[(i64)i * nrow + A32_N]);
    }
    else {
      const u32 p = t[2 * NL + 3], twop = 2 * p;
      const u32 r1 = rns32_one<NL>(x1, neg1, t);
      const u32 X = r0 >= twop ? r0 - twop : r0;
      const u32 T = mul_lazy32(r1, Tw32{t[2 * NL + 4], t[2 * NL + 5]}, p);
      o[(i64)i * nrow] = X + T;
      o[(i64)i * nrow + A32_N] = X + twop - T;
      if constexpr (HEAD == 2) {
        const u32 Tb = mul_lazy32(r1, Tw32{t[2 * NL + 6], t[2 * NL + 7]}, p);
        o[(i64)i * nrow + 2 * A32_N] = X + Tb;
        o[(i64)i * nrow + 3 * A32_N] = X + twop - Tb;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- sums of tensor products, evaluation form
//   out[g][0..2][prime][:] = sum_{t in [seg[g], seg[g+1])} (a0 b0, a0 b1 + a1 b0, a1 b1)  mod p   with a = ra[slot_a[t]], b = rb[slot_b[t]]
// ra [nua][2][NP][nrow], rb [nub][2][NP][nrow]: forward transforms (below p); out below 2p (what the inverse transform takes)
__global__ void __launch_bounds__(256) tensor_sum32_kernel(const u32* __restrict__ ra, const u32* __restrict__ rb, const int* __restrict__ slot_a,
                                                           const int* __restrict__ slot_b, const int* __restrict__ seg, int accumulate, u32* __restrict__ out,
                                                           i64 nrow, int NP, T32Primes pr) {
  const int g = blockIdx.z, l = blockIdx.y;
  const u32 p = pr.p[l], mu = pr.mu61[l], twop = 2 * p, sh = t32_shift(p);
  const u32 r32 = (u32)((((u64)1) << 32) % p);
  const i64 rs = (i64)NP * nrow;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  u32* o0 = out + (((i64)g * 3 + 0) * NP + l) * nrow + j;
  const int t0 = seg[g], t1 = seg[g + 1];
  // a 64-bit total takes 8 products below 2^60; reduced to below 2p every 4 terms (t1 adds two products per term)
  auto red = [&](u64 v) -> u32 {
    v = (u64)(u32)(v >> 32) * r32 + (u32)v;          // below 2^62 + 2^32
    v = (u64)(u32)(v >> 32) * r32 + (u32)v;          // below 2^61 (primes of 29 bits: below 2^59)
    const u32 q = __umulhi((u32)(v >> sh), mu);
    const u32 r = (u32)v - q * p;                     // below 3p
    return r >= twop ? r - twop : r;
  };
  u64 r0 = 0, r1 = 0, r2 = 0;
  if (accumulate) { r0 = o0[0]; r1 = o0[rs]; r2 = o0[2 * rs]; }
  // four terms per round: their sixteen loads are issued together (the kernel waits on its loads), then one reduction
  int t = t0;
  for (; t + 4 <= t1; t += 4) {
    u32 a0[4], a1[4], b0[4], b1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u32* a = ra + (((i64)slot_a[t + u] * 2) * NP + l) * nrow + j;
      const u32* b = rb + (((i64)slot_b[t + u] * 2) * NP + l) * nrow + j;
      a0[u] = a[0]; a1[u] = a[rs]; b0[u] = b[0]; b1[u] = b[rs];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      r0 += (u64)a0[u] * b0[u];
      r1 += (u64)a0[u] * b1[u] + (u64)a1[u] * b0[u];
      r2 += (u64)a1[u] * b1[u];
    }
    r0 = red(r0); r1 = red(r1); r2 = red(r2);
  }
  for (; t < t1; ++t) {                               // at most three more
    const u32* a = ra + (((i64)slot_a[t] * 2) * NP + l) * nrow + j;
    const u32* b = rb + (((i64)slot_b[t] * 2) * NP + l) * nrow + j;
    const u32 a0 = a[0], a1 = a[rs], b0 = b[0], b1 = b[rs];
    r0 += (u64)a0 * b0;
    r1 += (u64)a0 * b1 + (u64)a1 * b0;
    r2 += (u64)a1 * b1;
  }
  o0[0] = red(r0);
  o0[rs] = red(r1);
  o0[2 * rs] = red(r2);
}

// ---------------------------------------------------------------------------------------------- residues -> round(x / 2^logQ) mod 2^logQ
// rows [npolys][NP][n] (below p) -> out [npolys][LQ/64][n] limb-major positive residues (crt mode 1, kernels_crt.hip).
// S = 0: the rows are y_i = x (M / p_i)^-1 mod p_i already (T32_ROWS_CRT, below p: the inverse transform's closing constants), cinv is not read.
// S = 1: the rows are the two sub-inverses of 2^15-point rows; coefficient j < 2^14 is (A_j + B_j) / 2, coefficient j + 2^14 is
// (A_j - B_j) psi^-brv(1) / 2 -- the constants are folded into the CRT constant of the first multiplication.
// crt32_scale_block: the 128 coefficients from 128 bx of polynomial poly, one per thread; returns the thread's undecided bit (fast pass).
template <int LQ, bool EXACT, int R, int WT, int S>
__device__ __forceinline__ int crt32_scale_block(const u32* __restrict__ rows, i64 n, int NP, const T32Primes& pr, const Tw32* __restrict__ cinv,
                                                 const u32* __restrict__ inv57, const u32* __restrict__ Mw, u64* __restrict__ out, int wm, i64 poly, u32 bx) {
  static_assert((LQ & 63) == 0, "logQ a multiple of 64");
  constexpr int WU = (2 * LQ + R - 1) / R;            // words that reach below bit 2 logQ
  constexpr int NPMAX = R == 28 ? T32_NP_28 : T32_NP_26;
  constexpr int J0 = EXACT ? 0 : t32_j0(LQ, R, NPMAX);       // first word formed: the dropped part stays below bit logQ - 28 (t32_j0)
  constexpr int NW = WU - J0;
  static_assert(WU <= WT && J0 >= 0, "window");
  static_assert(R == 28 || R == 26, "word widths the tables are built in");
  static_assert(EXACT || ((u64)(NPMAX + 1) << 30) <= ((u64)1 << (LQ - T32_WIN - R * J0)), "dropped words stay below bit logQ - 28");
  static_assert(EXACT || ((u64)(NPMAX + 1) << 30) > ((u64)1 << (LQ - T32_WIN - R * (J0 + 1) < 0 ? 0 : LQ - T32_WIN - R * (J0 + 1))), "... and J0 is the largest such");
  static_assert(R * J0 <= LQ - 64, "the rounding limb is formed");
  const i64 j = (i64)bx * blockDim.x + threadIdx.x;
  const int hi = S ? (int)(j >> A32_LOGN) : 0;        // (uniform per workgroup)
  const u32* __restrict__ src = rows + poly * NP * n + (S ? (j & (A32_N - 1)) : j);
  u64 acc[NW];
#pragma unroll
  for (int l = 0; l < NW; ++l) acc[l] = 0;
  u32 fsum = 0;
#pragma unroll 2
  for (int i = 0; i < NP; ++i) {
    u32 y = src[(i64)i * n];
    if (S) {
      const u32 p = pr.p[i], B = src[(i64)i * n + A32_N];
      y = mul_lazy32(hi ? y + p - B : y + B, cinv[2 * i + hi], p);
      y = y >= p ? y - p : y;
    }
    fsum += __umulhi(y, inv57[i]);                    // (y / p) 2^25, low by less than one unit
    const u32* __restrict__ Mi = Mw + (i64)i * WT + J0;
#pragma unroll
    for (int l = 0; l < NW; ++l) acc[l] += (u64)y * Mi[l];
  }
  // x/M is within 1/8 of an integer: kappa = round(sum y_i / p_i); x = sum - kappa M = sum + kappa (2^(R WT) - M)  (mod 2^(R WT))
  const u32 kappa = (fsum + (1u << 24)) >> 25;
  {
    const u32* __restrict__ Nm = Mw + (i64)NP * WT + J0;
#pragma unroll
    for (int l = 0; l < NW; ++l) acc[l] += (u64)kappa * Nm[l];
  }
  // carries: words of R bits
  u64 carry = 0;
#pragma unroll
  for (int l = 0; l < NW; ++l) { const u64 v = acc[l] + carry; acc[l] = v & (((u64)1 << R) - 1); carry = v >> R; }
  // 64 bits from bit B of x (two's complement, bits above R WU dropped)
  auto limb = [&](int B) -> u64 {
    const int l0 = B / R - J0, o = B % R;
    u64 v = acc[l0] >> o;
    if (l0 + 1 < NW) v |= acc[l0 + 1] << (R - o);
    if (l0 + 2 < NW) v |= acc[l0 + 2] << (2 * R - o);
    if (l0 + 3 < NW && 3 * R - o < 64) v |= acc[l0 + 3] << (3 * R - o);
    return v;
  };
  const u64 G = limb(LQ - 64);                         // bits logQ-64 .. logQ-1
  int undecided = 0;
  if (!EXACT) undecided = t32_undecided(G);
  u64 c = G >> 63;                                     // round half up: + bit logQ-1
  u64* __restrict__ o = out + poly * (LQ / 64) * n + j;
  u32* __restrict__ o32 = reinterpret_cast<u32*>(out) + poly * (LQ / 32) * n + j;
#pragma unroll
  for (int i = 0; i < LQ / 64; ++i) {
    u64 v = limb(LQ + 64 * i);
    v += c;
    c = (c && v == 0) ? 1 : 0;
    if (wm) { o32[(i64)(2 * i) * n] = (u32)v; o32[(i64)(2 * i + 1) * n] = (u32)(v >> 32); }
    else o[(i64)i * n] = v;
  }
  return undecided;
}
// The fast pass (EXACT = false): grid (n / 128, npolys), one block per workgroup; a workgroup with an undecided coefficient sets its flag and
// appends itself to the redo list (t32_flag).  The redo pass (EXACT = true): T32_REDO_GRID workgroups walk that list -- or, had it overflowed,
// the flags of all npolys n / 128 blocks -- and form every word of the flagged blocks again.  (Until the list the redo pass was launched over
// the fast pass's grid, 393 216 workgroups per 1024 products that read one flag byte each: 0.09 ms of a 30.4 ms step.)
template <int LQ, bool EXACT, int R, int WT, int S>
__global__ void __launch_bounds__(128) crt32_scale_kernel(const u32* __restrict__ rows, i64 n, int NP, T32Primes pr, const Tw32* __restrict__ cinv,
                                                           const u32* __restrict__ inv57, const u32* __restrict__ Mw, u64* __restrict__ out,
                                                           unsigned char* __restrict__ flags, u32* __restrict__ list, u32 npolys,
                                                           int wm /* 1: out as 32-bit WORD rows [npolys][LQ/32][n] (what the 32-bit digit loader reads whole lines of) */) {
  if constexpr (!EXACT) {
    const u32 wg = blockIdx.y * gridDim.x + blockIdx.x;
    const int undecided = crt32_scale_block<LQ, false, R, WT, S>(rows, n, NP, pr, cinv, inv57, Mw, out, wm, blockIdx.y, blockIdx.x);
    const int any = __syncthreads_or(undecided);
    if (threadIdx.x == 0) t32_flag(flags, list, wg, any);
  } else {
    const u32 gx = (u32)(n / 128), total = gx * npolys, cnt = list[0];
    if (cnt <= T32_LIST_CAP) {
      for (u32 k = blockIdx.x; k < cnt; k += gridDim.x) {
        const u32 wg = list[T32_LIST_HDR + k];
        crt32_scale_block<LQ, true, R, WT, S>(rows, n, NP, pr, cinv, inv57, Mw, out, wm, wg / gx, wg % gx);
      }
    } else {
      for (u32 wg = blockIdx.x; wg < total; wg += gridDim.x)
        if (flags[wg]) crt32_scale_block<LQ, true, R, WT, S>(rows, n, NP, pr, cinv, inv57, Mw, out, wm, wg / gx, wg % gx);
    }
  }
}

// The fast pass of crt32_scale_kernel<512, false, 28, 38, 0> on the int8 matrix cores (option crt32_mfma; tables and arithmetic: crt32_bytes.h).
// Per coefficient the window F = sum_i y_i C_i + kappa C_kappa is a product of the residues' bytes with a constant matrix, 160 deep and 72 byte
// columns wide: operand A holds the constants (rows = byte columns), operand B the residues (column = coefficient), fifteen
// v_mfma_i32_32x32x32_i8 per 32 coefficients -- three row tiles by five depth steps -- instead of 770 64-bit multiply-adds per coefficient.
//   * A wave takes 32 coefficients.  Lane l of half h = l / 32 loads, for coefficient l % 32, the residue words of primes 8 ks + 4 h + (0 .. 3)
//     per depth step ks: each load instruction reads 128 contiguous bytes of two rows.  y ^ 0x80808080 are the signed bytes yb - 128; the
//     constant slot NP + 1 (operand bytes 1, 0, 0, 0) makes up for the offset and for the bias the accumulators start at (crt32_bytes.h).
//   * kappa is crt32_scale_kernel's value, bit for bit: the same sum of floors umulhi(y_i, inv57_i) over the primes (a u32 sum in any order),
//     twenty per lane and one exchange between the half waves.  It then takes slot NP of the depth, a "residue" like the others.
//   * The rows are mapped so that lanes 0-31 end with columns 0 .. 35 (bits 448 .. 735) of their coefficient in 36 accumulator registers and
//     lanes 32-63 with columns 36 .. 71 (bits 736 .. 1023).  Every column sum is a positive number below 2^23, so two columns join in 32 bits,
//     two such pairs in a (word, carry) pair, and one add-with-carry per word runs the carries through a lane's nine words.  The low half
//     holds the rounding limb G (words 0, 1: bits 448 .. 511), decides `undecided` exactly as t32_undecided does, and hands its carry -- with
//     the rounding carry, which runs through only when its seven output words are all ones -- to the high half: one more exchange and one
//     more run of add-with-carry.  Each half stores whole 128-byte pieces of its 7 / 9 output word rows.
//   * The same integer F mod 2^576 as the VALU kernel (the balanced bytes represent 256^a C_i exactly), so the same limbs, the same rounding and
//     the same flags: the EXACT pass behind it is the unchanged one.
// A workgroup is four waves = the 128 coefficients one flag stands for, and walks nblk consecutive blocks with the 60 registers of A loaded once.
typedef int t32_v16i __attribute__((ext_vector_type(16)));
typedef int t32_v4i __attribute__((ext_vector_type(4)));
template <int LQ>
__global__ void __launch_bounds__(256, 2) crt32_mfma_kernel(const u32* __restrict__ rows, int NP, const u32* __restrict__ inv57, const u32* __restrict__ bytes,
                                                             u32* __restrict__ out32, unsigned char* __restrict__ flags, u32* __restrict__ list, u32 nwg, u32 nblk, int wm) {
  static_assert(LQ == 512, "the compiled window: 72 byte columns from bit 448");
  constexpr u32 n = A32_N;
  constexpr int KS = hm::C32B_KSTEPS, NT = hm::C32B_TILES, NWD = hm::C32B_HALF / 4;      // 9 words per lane
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const u32 jw = (threadIdx.x >> 6) * 32 + (lane & 31);          // coefficient within the block
  t32_v4i A[NT * KS];
  {
    const t32_v4i* __restrict__ ap = reinterpret_cast<const t32_v4i*>(bytes);
#pragma unroll
    for (int i = 0; i < NT * KS; ++i) A[i] = ap[i * 64 + lane];
  }
  t32_v16i bias;
#pragma unroll
  for (int r = 0; r < 16; ++r) bias[r] = hm::C32B_BIAS;
  asm volatile("" : "+v"(bias));                                  // (sixteen registers for the whole loop, not sixteen moves per tile)
  u32 iv[KS][4];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int s = ks * 8 + h * 4 + t; iv[ks][t] = s < NP ? inv57[s] : 0u; }
  // lane offsets of the loads: the half wave's share of the row index goes into the offset, the rest is wave-uniform.  The last depth step holds
  // the slots from 32: beyond the primes a lane reads row NP - 1 (a valid address) and drops the value.
  // (buffer loads and stores: a descriptor per block -- the polynomial's rows from the block's first coefficient, range-checked -- with the row as
  // the scalar offset and ONE 32-bit register per lane; as pointers the compiler forms a 64-bit address per row in vector registers)
  const u32 loff = ((u32)h * (4 * n) + jw) * 4;
  u32 loff4[4];
  bool prime4[4], kappa4[4], const4[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int s = 32 + h * 4 + t;
    prime4[t] = s < NP; kappa4[t] = s == NP; const4[t] = s == NP + 1;
    loff4[t] = ((u32)(s < NP ? s : NP - 1) * n + jw) * 4;
  }
  // the residues of block wg: twenty loads per lane, all in flight together
  u32 y[KS][4];
  auto load_block = [&](u32 wg) {
    const i64 poly = wg / (n / 128);
    const u32 j0 = (wg % (n / 128)) * 128;
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(rows + poly * NP * n + j0), 0, (int)(((u32)NP * n - j0) * 4), 0x00020000);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)                                // (NP >= 32: the first four steps hold primes only)
#pragma unroll
      for (int t = 0; t < 4; ++t) y[ks][t] = __builtin_amdgcn_raw_buffer_load_b32(src, loff, (ks * 8 + t) * n * 4, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) y[4][t] = __builtin_amdgcn_raw_buffer_load_b32(src, loff4[t], 0, 0);
  };
  // the workgroup's flag: one LDS word per block, three in rotation, so that one barrier per block is enough -- word (b + 2) % 3 is cleared by
  // thread 0 behind barrier b (it last read it behind barrier b - 1) and written by the waves of block b + 2, which thread 0 lets through
  // barrier b + 1 only after that.  (The barrier is a bare s_barrier behind the LDS write: nothing here waits for the block's stores.)
  __shared__ u32 s_any[3];
  if (threadIdx.x < 3) s_any[threadIdx.x] = 0;
  __syncthreads();
  const u32 wg0 = blockIdx.x * nblk;
  const u32 nb = wg0 < nwg ? (nwg - wg0 < nblk ? nwg - wg0 : nblk) : 0u;
  if (nb) load_block(wg0);
  for (u32 b = 0; b < nb; ++b) {
    const u32 wg = wg0 + b;
    const i64 poly = wg / (n / 128);
    const u32 j0 = (wg % (n / 128)) * 128;
#pragma unroll
    for (int t = 0; t < 4; ++t) y[4][t] = prime4[t] ? y[4][t] : 0u;
    u32 fsum = 0;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) fsum += __umulhi(y[ks][t], iv[ks][t]);      // (y / p) 2^25, low by less than one unit; 0 beyond the primes
    fsum += (u32)__shfl_xor((int)fsum, 32);
    const u32 kappa = (fsum + (1u << 24)) >> 25;
    t32_v4i B[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) B[ks][t] = (int)(y[ks][t] ^ 0x80808080u);
#pragma unroll
    for (int t = 0; t < 4; ++t) B[4][t] = const4[t] ? 1 : (kappa4[t] ? (int)(kappa ^ 0x80808080u) : B[4][t]);
    if (b + 1 < nb) load_block(wg + 1);                  // (the next block's residues travel while this one is worked on: y is dead from here)
    t32_v16i acc[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
      acc[tl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[tl * KS], B[0], bias, 0, 0, 0);
#pragma unroll
      for (int ks = 1; ks < KS; ++ks) acc[tl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[tl * KS + ks], B[ks], acc[tl], 0, 0, 0);
    }
    // word w = columns 4 w .. 4 w + 3 of this half: T[w] + 2^32 H[w] with H below 2^16; then W[w] = T[w] + H[w - 1] + carry
    u32 W[NWD];
    u32 Hp = 0, cy = 0;
#pragma unroll
    for (int w = 0; w < NWD; ++w) {
      const int q = 4 * w;
      const u32 lo = (u32)acc[q >> 4][q & 15] + ((u32)acc[(q + 1) >> 4][(q + 1) & 15] << 8);          // below 2^23 * 257 < 2^32
      const u32 hi2 = (u32)acc[(q + 2) >> 4][(q + 2) & 15] + ((u32)acc[(q + 3) >> 4][(q + 3) & 15] << 8);
      const u64 v = (u64)lo + ((u64)hi2 << 16);
      W[w] = __builtin_addc((u32)v, Hp, cy, &cy);
      Hp = (u32)(v >> 32);
    }
    const u64 G = ((u64)W[1] << 32) | W[0];              // bits 448 .. 511 (the low half's; the high half's value is not used)
    const int undecided = h ? 0 : t32_undecided(G);
    const u32 rnd = h ? 0u : W[1] >> 31;                  // round half up: + bit 511
    const u32 ones = W[2] & W[3] & W[4] & W[5] & W[6] & W[7] & W[8];
    const u32 cout = Hp + cy + ((rnd && ones == 0xffffffffu) ? 1u : 0u);
    const u32 cswap = (u32)__shfl_xor((int)cout, 32);    // (every lane takes part: an exchange inside `h ? ... : 0` would run with the low half switched off and read nothing from it)
    const u32 cin = h ? cswap : 0u;
    cy = 0;
#pragma unroll
    for (int w = 0; w < NWD; ++w) W[w] = __builtin_addc(W[w], w == 0 ? cin : (w == 2 ? rnd : 0u), cy, &cy);
    // output word ow of the coefficient: the low half's words 2 .. 8 are 0 .. 6, the high half's 0 .. 8 are 7 .. 15
    if (wm) {
      const __amdgpu_buffer_rsrc_t o = __builtin_amdgcn_make_buffer_rsrc(out32 + poly * (LQ / 32) * n + j0, 0, (int)(((LQ / 32) * n - j0) * 4), 0x00020000);
      const u32 soff = ((u32)h * (9 * n) + jw) * 4;
#pragma unroll
      for (int w = 2; w < NWD; ++w) __builtin_amdgcn_raw_buffer_store_b32(W[w], o, soff, (w - 2) * n * 4, 0);
      if (h) { __builtin_amdgcn_raw_buffer_store_b32(W[0], o, jw * 4, 7 * n * 4, 0); __builtin_amdgcn_raw_buffer_store_b32(W[1], o, jw * 4, 8 * n * 4, 0); }
    } else {
#pragma unroll
      for (int w = 0; w < NWD; ++w) {
        const int ow = h ? 7 + w : w - 2;
        if (ow >= 0) out32[((poly * (LQ / 64) + (ow >> 1)) * n + j0 + jw) * 2 + (ow & 1)] = W[w];
      }
    }
    if (undecided) atomicOr(&s_any[b % 3], 1u);                  // (LDS atomics: the words are read and cleared the same way, behind the barrier)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (threadIdx.x == 0) {
      t32_flag(flags, list, wg, (int)atomicOr(&s_any[b % 3], 0u));
      atomicAnd(&s_any[(b + 2) % 3], 0u);
    }
  }
}

// The same conversion for any logQ <= 512 (words of 28 bits, rows of 2^14) and for the linear-convolution rings: the window [J0, J0 + NW)
// of words and the bit positions are run-time values, so after the (compile-time indexed) accumulation and the carry pass the words go
// through LDS, one column per thread, and the 64-bit limbs are cut from there.  The fold (fold_off = lin_fold_pack: the offset Q or m and the stride
// s = q^(k-1) of a ring m = 2Q or Q, Q = q^k; phi = (q - 1) s = n_out): the residue of output coefficient j is
//   r_j - r_(j+Q) - (-1)^floor(j/s) r_(phi + j mod s)   (m = 2Q: modulo X^Q + 1, then modulo Phi_m = sum_{i<q} (-X^s)^i)
//   r_j + r_(j+m) - r_(phi + j mod s)                   (m odd:  modulo X^m - 1, then modulo Phi_m = sum_{i<q} X^(i s))
// of the linear product's residues; s = 1 is the fixed top phi and the sign (-1)^j of the prime and 2 x prime rings.
// NWMAX = T32_GEN_NW with J0 from the host, or T32_GEN_NWX with J0 = 0 for the exact pass over flagged workgroups.
// S = 1 (rows of 2^15 = the two sub-inverses A, B of ntt32_inv_kernel3): the coefficient at position e < 2^14 is (A_e + B_e) / 2, at e + 2^14
// (A_e - B_e) psi^-brv(1) / 2; the two constants sit in cinv[2i], cinv[2i + 1] (times the CRT constant), so the positions of the lower and of
// the upper half are summed separately and the residue is  lo c_lo + hi c_hi.
// S and FOLD (0: none, 1: m = 2Q, 2: m odd) are compile-time: the (up to) three positions a coefficient is folded from do not depend on the
// prime, so their offsets, halves and signs are worked out once, the loads of a prime are unconditional (clamped index, masked value) and
// independent of each other, and the multiply-adds run over all NWMAX words without a branch (words from NW upwards are never looked at; the
// table is padded so that the reads stay inside it).  With the positions behind run-time branches and `if (l < NW)` around every word the
// kernel waited on one scalar and one vector load after the other: 13.5 ms per 1024 multiplications on the reference's ring at the metric's
// size against 2.5 ms for the compiled shape on half as long rows.
template <int NWMAX, bool EXACT, int S, int FOLD>
__global__ void __launch_bounds__(128) crt32_scale_generic_kernel(const u32* __restrict__ rows, i64 nrow, i64 n_out, i64 fold_off, int NP, int LQ, int J0, int NW, int WT,
                                                                   T32Primes pr, const Tw32* __restrict__ cinv, const u32* __restrict__ inv57, const u32* __restrict__ Mw,
                                                                   u64* __restrict__ out, unsigned char* __restrict__ flags, int wm) {
  constexpr int R = 28;
  __shared__ u32 xs[NWMAX * 128];
  const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (EXACT && !flags[wg]) return;
  const i64 poly = blockIdx.y;
  const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = j < n_out;
  const u32* __restrict__ src = rows + poly * NP * nrow;
  u64 acc[NWMAX];
#pragma unroll
  for (int l = 0; l < NWMAX; ++l) acc[l] = 0;
  u32 fsum = 0;
  if (active) {
    // term 0: position j, +;  term 1: position j + off, - (m = 2Q) or + (m odd);  term 2: position phi + j mod s, -(-1)^floor(j/s) (m = 2Q) or - (m odd)
    constexpr int NT = FOLD ? 3 : 1;
    u32 eb[NT];
    bool up[NT], ok[NT], neg[NT];
    {
      u32 f_off = 0, f_top = 0;
      bool f_odd = false;
      if (FOLD) lin_fold_pos(fold_off, j, n_out, f_off, f_top, f_odd);      // (j / s and j mod s once per thread, in 32 bits)
      const i64 e[3] = {j, j + f_off, f_top};
      const bool ng[3] = {false, FOLD == 1, FOLD == 2 || !f_odd};
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        ok[k] = e[k] < nrow;
        const u32 idx = ok[k] ? (u32)e[k] : 0u;
        up[k] = S && idx >= (u32)A32_N;
        eb[k] = S ? (idx & (u32)(A32_N - 1)) : idx;
        neg[k] = ng[k];
      }
    }
#pragma unroll 2
    for (int i = 0; i < NP; ++i) {
      const u32 p = pr.p[i], twop = 2 * p;
      const u32* __restrict__ ri = src + (i64)i * nrow;
      u32 y;
      if (S) {
        // position e of the row: lower half (A_e + B_e), upper half (A - B)(e - 2^14), each below 2p, summed per half with its sign
        u32 A[NT], B[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) { A[k] = ri[eb[k]]; B[k] = ri[eb[k] + A32_N]; }
        auto red2 = [&](u32 v) -> u32 { return min(v, v - twop); };                 // [0, 4p) -> [0, 2p)
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          const u32 t = up[k] ? A[k] + p - B[k] : A[k] + B[k];                       // at most 2p
          const u32 v = ok[k] ? (neg[k] ? twop - t : t) : 0u;
          if (k == 0) { lo = up[0] ? 0u : v; hi = up[0] ? v : 0u; }
          else { lo = red2(lo + (up[k] ? 0u : v)); hi = red2(hi + (up[k] ? v : 0u)); }
        }
        if (NT == 1) { lo = red2(lo); hi = red2(hi); }
        y = mul_lazy32(lo, cinv[2 * i], p) + mul_lazy32(hi, cinv[2 * i + 1], p);    // below 4p
        y = min(y, y - twop);
        y = min(y, y - p);
      } else {
        // Whole rows, every value in [0, p), p < 2^30.  The fold adds three of them -- the row's own, p - b or b, and c or p - c (a position
        // beyond the row gives b = 0, and p - 0 = p is still congruent to 0): at most 3p < 2^32, no wrap-around.
        u32 r = ri[eb[0]];
        if (FOLD) {
          const u32 b = ok[1] ? ri[eb[1]] : 0u, c = ri[eb[2]];
          if (FOLD == 1) r = r + (p - b) + (neg[2] ? p - c : c);                    // r_j - r_(j+Q) - (-1)^floor(j/s) r_(phi + j mod s): in [0, 3p]
          else r = r + b + (p - c);                                                  // r_j + r_(j+m) - r_(phi + j mod s): in [0, 3p)
        }
        if (pr.closing) {
          // T32_ROWS_CRT (rows of 2^14): the values are y = x (M / p_i)^-1 mod p_i already, and the fold is linear, so the folded value IS the
          // folded y modulo p.  It must be canonical: the multiply-adds need y < 2^30 (NP + 1 terms below 2^58 per 64-bit word) and kappa's sum
          // takes y / p below 1.  [0, 3p] lies inside [0, 4p): one step to [0, 2p), one to [0, p).
          if (FOLD) { r = min(r, r - twop); r = min(r, r - p); }
          y = r;
        } else {
          // T32_ROWS_PLAIN (rows of 2^16 and longer, finished by their tail pass): the product by (M / p_i)^-1 (mul_lazy32 takes any u32)
          y = mul_lazy32(r, cinv[2 * i], p);
          y = y >= p ? y - p : y;
        }
      }
      fsum += __umulhi(y, inv57[i]);
      const u32* __restrict__ Mi = Mw + (i64)i * WT + J0;
#pragma unroll
      for (int l = 0; l < NWMAX; ++l) acc[l] += (u64)y * Mi[l];
    }
    const u32 kappa = (fsum + (1u << 24)) >> 25;
    const u32* __restrict__ Nm = Mw + (i64)NP * WT + J0;
    u64 carry = 0;
#pragma unroll
    for (int l = 0; l < NWMAX; ++l)
      if (l < NW) {
        const u64 v = acc[l] + (u64)kappa * Nm[l] + carry;
        xs[l * 128 + threadIdx.x] = (u32)(v & 0xfffffffull);
        carry = v >> R;
      }
  }
  int undecided = 0;
  if (active) {
    // 64 bits from bit B of x (each thread reads back its own column)
    auto word = [&](int l) -> u64 { return (l >= 0 && l < NW) ? (u64)xs[l * 128 + threadIdx.x] : 0ull; };
    auto limb = [&](int B) -> u64 {
      const int l0 = B / R - J0, o = B % R;
      u64 v = word(l0) >> o;
      v |= word(l0 + 1) << (R - o);
      v |= word(l0 + 2) << (2 * R - o);
      if (3 * R - o < 64) v |= word(l0 + 3) << (3 * R - o);
      return v;
    };
    const u64 G = limb(LQ - 64);                         // bits logQ-64 .. logQ-1
    if (!EXACT) undecided = t32_undecided(G);
    u64 c = G >> 63;                                     // round half up: + bit logQ-1
    const int nlq = (LQ + 63) >> 6;
    u64* __restrict__ o = out + poly * nlq * n_out + j;
    u32* __restrict__ o32 = reinterpret_cast<u32*>(out) + poly * (2 * nlq) * n_out + j;
    for (int i = 0; i < nlq; ++i) {
      u64 v = limb(LQ + 64 * i);
      v += c;
      c = (c && v == 0) ? 1 : 0;
      const int bits_left = LQ - 64 * i;
      if (bits_left < 64) v &= ((u64)1 << bits_left) - 1;
      if (wm) { o32[(i64)(2 * i) * n_out] = (u32)v; o32[(i64)(2 * i + 1) * n_out] = (u32)(v >> 32); }
      else o[(i64)i * n_out] = v;
    }
  }
  if (!EXACT) {
    const int any = __syncthreads_or(undecided);
    if (threadIdx.x == 0) flags[wg] = any ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------- launchers
static i64 t32_nrow(const fhesi_ctx* ctx) { return (i64)A32_N << ctx->tensor32->S; }
template <int NL>
static int t32_launch_rns(fhesi_ctx* ctx, const T32Config* c, const u64* d_a, const u64* d_b, i64 npolys, i64 na2, bool paired, u32* d_r) {
  const int S = ctx->tensor32->S;
  const i64 nrow = t32_nrow(ctx), n_src = ctx->phim;
  const unsigned zs = npolys * (A32_N / 256) >= 2048 ? 1u : (npolys * (A32_N / 256) >= 1024 ? 2u : 5u);      // (primes split over z for small launches)
  // (rows of 2^17 and longer -- S >= 3, the simple path -- are converted as plain zero-padded rows, one block per 256 positions of the whole row;
  // their head stages are a pass of their own in t32_fwd)
  const dim3 grid((unsigned)((S >= 3 ? nrow : (i64)A32_N) / 256), (unsigned)npolys, zs);
  const int* ia = paired && ctx->op_idx ? ctx->op_idx + ctx->op_idx_done : nullptr;
  const int* ib = ia ? ia + ctx->op_idx_n : nullptr;
  const int dup = S == 1 && ctx->lin_q ? 1 : 0;
  if (S >= 2 && !ctx->lin_q) FHESI_FAIL("tensor32: rows of 2^16 and longer exist for the padded linear-convolution rings only");
#define T32_GO(HEAD, PAIRED) do { PROF_KERNEL(ctx, PROF_RNS, rns32_reduce_kernel<NL, HEAD, PAIRED>); \
    rns32_reduce_kernel<NL, HEAD, PAIRED><<<grid, 256, 0, ctx->stream>>>(d_a, d_b, na2, n_src, nrow, d_r, c->NP, c->d_rns, ia, ib, dup); } while (0)
  if (S >= 3) { if (paired) T32_GO(0, true); else T32_GO(0, false); }
  else if (S == 2) { if (paired) T32_GO(2, true); else T32_GO(2, false); }
  else if (S && !dup) { if (paired) T32_GO(1, true); else T32_GO(1, false); }
  else { if (paired) T32_GO(0, true); else T32_GO(0, false); }
#undef T32_GO
  HIP_TRY(hipGetLastError());
  return 0;
}
static int t32_rns(fhesi_ctx* ctx, const T32Config* c, const u64* d_a, const u64* d_b, i64 npolys, i64 na2, bool paired, u32* d_r) {
  ProfScope prof(ctx, PROF_RNS, (double)npolys);
#define T32_RNS(NL) case NL: return t32_launch_rns<NL>(ctx, c, d_a, d_b, npolys, na2, paired, d_r);
  switch (c->nl) {
    T32_RNS(1) T32_RNS(2) T32_RNS(3) T32_RNS(4) T32_RNS(5) T32_RNS(6) T32_RNS(7) T32_RNS(8) T32_RNS(9) T32_RNS(10) T32_RNS(11) T32_RNS(12)
    T32_RNS(13) T32_RNS(14) T32_RNS(15) T32_RNS(16)
    default: break;
  }
#undef T32_RNS
  FHESI_FAIL("tensor32: %d limbs", c->nl);
}
// f(std::integral_constant<int, PB>) for the size of the context's primes, 29 or 30 bits; f reads it as decltype(pb)::value (a32_with_S's pattern)
template <class F>
static inline void t32_with_bits(const fhesi_tensor32* x, F&& f) {
  if (x->bits == 29) f(std::integral_constant<int, 29>{}); else f(std::integral_constant<int, 30>{});
}
static int t32_fwd(fhesi_ctx* ctx, const T32Config* c, u32* d_r, i64 npolys) {
  const fhesi_tensor32* x = ctx->tensor32;
  ProfScope prof(ctx, PROF_NTT_FWD, (double)(npolys * c->NP));
  if (npolys > 0x7fffffff) FHESI_FAIL("tensor32: too many rows per launch");
  const dim3 grid((unsigned)npolys, (unsigned)(c->NP << x->S));
  // head stages of the plain rows as a pass of their own (rows of 2^16 take them in rns32_reduce)
  if (x->S >= 3) {
    if (!launch_ntt32_head_pass(ctx->stream, x->S, d_r, npolys * c->NP, c->NP, 0, x->tab)) FHESI_FAIL("tensor32: no kernel for rows of 2^%d", A32_LOGN + x->S);
    HIP_TRY(hipGetLastError());
  }
  if (!a32_with_S<0, 6>(x->S, [&](auto s) {
    constexpr int SS = decltype(s)::value;
    t32_with_bits(x, [&](auto pb) {
      constexpr int PB = decltype(pb)::value;
      PROF_KERNEL(ctx, PROF_NTT_FWD, (ntt32_fwd_kernel3<false, SS, false, T32Primes, true, false, PB>));
      ntt32_fwd_kernel3<false, SS, false, T32Primes, true, false, PB><<<grid, A32_T, 0, ctx->stream>>>(d_r, npolys, c->NP, 0, c->pr, x->tab.d_fwd, Dig32Src{}, Aux32Head{});
    });
  })) FHESI_FAIL("tensor32: no kernel for rows of 2^%d", A32_LOGN + x->S);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the inverse transforms of nrows rows, in place; TENSOR: the rows are formed in the loader, as the tensor products of src's forward rows
template <bool TENSOR>
static int t32_inv(fhesi_ctx* ctx, const T32Config* c, u32* rows, i64 nrows, dim3 grid, const u32* src) {
  const fhesi_tensor32* x = ctx->tensor32;
  ProfScope prof(ctx, PROF_NTT_INV, (double)(nrows * c->NP));
  t32_with_bits(x, [&](auto pb) {
    constexpr int PB = decltype(pb)::value;
    PROF_KERNEL(ctx, PROF_NTT_INV, (ntt32_inv_kernel3<false, TENSOR, T32Primes, PB>));
    ntt32_inv_kernel3<false, TENSOR, T32Primes, PB><<<grid, A32_T, 0, ctx->stream>>>(rows, nrows, c->NP, 0, c->pr, x->tab.d_inv, x->S, src);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
template <int LQ, int R, int WT, int S>
static int t32_launch_crt(fhesi_ctx* ctx, const T32Config* c, const u32* d_t, i64 npolys, u64* d_parts, bool wm) {
  if (c->NP > (R == 28 ? T32_NP_28 : T32_NP_26)) FHESI_FAIL("tensor32: %d primes exceed the bound the CRT window is derived from", c->NP);
  const i64 n = (i64)A32_N << S;
  const dim3 grid((unsigned)(n / 128), (unsigned)npolys);
  void* d_fl;
  // flags, then the redo list (t32_flag): per lane, like every workspace slot, so two lanes keep separate flags and separate lists
  const size_t nwg = (size_t)grid.x * grid.y, fl_bytes = (nwg + 15) & ~(size_t)15;
  if (nwg > 0x7fffffff) FHESI_FAIL("tensor32: too many rows per launch");
  FHESI_TRY(ws_reserve(ctx, 6, fl_bytes + (size_t)(T32_LIST_HDR + T32_LIST_CAP) * 4, &d_fl));
  unsigned char* fl = (unsigned char*)d_fl;
  u32* list = reinterpret_cast<u32*>(fl + fl_bytes);
  t32_list_clear_kernel<<<1, 64, 0, ctx->stream>>>(list);          // (a kernel, not a memset: nothing here may stop the stream)
  // The matrix-core form pays 60 KB of operand loads per workgroup before its first coefficient, so a workgroup walks up to 32 blocks -- as many
  // as leave 2048 workgroups -- and launches below T32_MFMA_MIN_WG blocks (128 polynomials: 43 products) keep the VALU kernel, whose
  // workgroups start at once.  crt32_mfma = 2 takes the matrix cores at any size (tests, A/B).
  bool mfma = false;
  if constexpr (LQ == 512 && S == 0) mfma = c->d_bytes != nullptr && (ctx->opt.crt32_mfma >= 2 || (ctx->opt.crt32_mfma == 1 && nwg >= T32_MFMA_MIN_WG));
  if (mfma) {
    if constexpr (LQ == 512 && S == 0) {
      const u32 nblk = nwg >= 32 * 2048 ? 32u : (nwg >= 2 * 2048 ? (u32)(nwg / 2048) : 1u);
      PROF_KERNEL(ctx, PROF_CRT, (crt32_mfma_kernel<LQ>));
      crt32_mfma_kernel<LQ><<<(unsigned)((nwg + nblk - 1) / nblk), 256, 0, ctx->stream>>>(d_t, c->NP, c->d_inv57, c->d_bytes, reinterpret_cast<u32*>(d_parts), fl, list, (u32)nwg, nblk, wm ? 1 : 0);
    }
  } else {
    PROF_KERNEL(ctx, PROF_CRT, (crt32_scale_kernel<LQ, false, R, WT, S>));
    crt32_scale_kernel<LQ, false, R, WT, S><<<grid, 128, 0, ctx->stream>>>(d_t, n, c->NP, c->pr, c->d_cinv, c->d_inv57, c->d_Mw, d_parts, fl, list, (u32)npolys, wm ? 1 : 0);
  }
  HIP_TRY(hipGetLastError());
  if (!ctx->opt.crt_skip_cleanup) {
    crt32_scale_kernel<LQ, true, R, WT, S><<<T32_REDO_GRID, 128, 0, ctx->stream>>>(d_t, n, c->NP, c->pr, c->d_cinv, c->d_inv57, c->d_Mw, d_parts, fl, list, (u32)npolys, wm ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// d_t [npolys][NP][nrow] coefficient-form residues -> d_parts [npolys][ceil(logQ/64)][phi(m)]
// form: what the caller's inverse transform left in d_t (the closing word of the T32Primes it was launched with).  The CRT kernels take one form
// per row length -- T32_ROWS_CRT from rows of 2^14 (they multiply by nothing), T32_ROWS_PLAIN from longer rows (cinv carries the constant with
// the tail's) -- and the other one would come out as a wrong ciphertext, silently: refused here.
static int t32_crt(fhesi_ctx* ctx, const T32Config* c, const u32* d_t, i64 npolys, u32 form, u64* d_parts, bool wm) {
  const int S = ctx->tensor32->S, logQ = c->logQ;
  const u32 takes = S ? T32_ROWS_PLAIN : T32_ROWS_CRT;
  if (form != takes || c->pr.closing != takes) FHESI_FAIL("tensor32: rows in form %u (configuration: %u) handed to the CRT of rows of 2^%d, which takes form %u", form, c->pr.closing, A32_LOGN + S, takes);
  ProfScope prof(ctx, PROF_CRT, (double)npolys);
  if (!c->generic) {
    if (logQ == 512 && !S) return t32_launch_crt<512, T32_R_512, T32_WT_512, 0>(ctx, c, d_t, npolys, d_parts, wm);
    if (logQ == 512 && S) return t32_launch_crt<512, T32_R_512, T32_WT_512, 1>(ctx, c, d_t, npolys, d_parts, wm);
    if (logQ == 1024 && !S) return t32_launch_crt<1024, T32_R_1024, T32_WT_1024, 0>(ctx, c, d_t, npolys, d_parts, wm);
    return t32_launch_crt<1024, T32_R_1024, T32_WT_1024, 1>(ctx, c, d_t, npolys, d_parts, wm);
  }
  // the generic form: the same window at run time -- from the first word whose dropped part stays below bit logQ - 28 (t32_j0) up to bit 2 logQ
  const i64 n_out = ctx->phim, nrow = t32_nrow(ctx);
  const int WU = (2 * logQ + 27) / 28;
  if (c->NP > T32_NP_28) FHESI_FAIL("tensor32: %d primes exceed the bound the CRT window is derived from", c->NP);
  const int J0 = t32_j0(logQ, 28, T32_NP_28);
  const int NW = WU - J0;
  if (NW > T32_GEN_NW || WU > T32_GEN_NWX || WU > c->WT) FHESI_FAIL("tensor32: logQ=%d outside the generic CRT window", logQ);
  const dim3 grid((unsigned)((n_out + 127) / 128), (unsigned)npolys);
  void* d_fl;
  FHESI_TRY(ws_reserve(ctx, 6, (size_t)grid.x * grid.y, &d_fl));
  unsigned char* fl = (unsigned char*)d_fl;
  const int fold = !ctx->lin_q ? 0 : (ctx->lin_prime ? 2 : 1);
  const i64 off = ctx->lin_q ? lin_fold_pack(ctx->lin_q, ctx->lin_s, false) : 0;      // (the kind of fold is the template argument)
  if (S >= 2) {      // rows of 2^16 and longer: the tail stages as a pass of their own over the sub-inverses (in place), then the fold from whole rows
    const fhesi_tensor32* x = ctx->tensor32;
    if (!launch_ntt32_tail_pass(ctx->stream, S, const_cast<u32*>(d_t), npolys * c->NP, c->NP, 0, x->tab, 0)) FHESI_FAIL("tensor32: no kernel for rows of 2^%d", A32_LOGN + x->S);
    HIP_TRY(hipGetLastError());
  }
  // (A compiled form of this kernel for the reference drivers' own shapes -- logQ, word window and limb positions as constants, the words in
  // registers from the multiply-adds to the limbs -- was measured in round 6 and removed: crt class 8.80-8.85 ms per 1024 multiplications at
  // m = 32602 with this run-time form, 8.92-8.99 with the compiled one (profiles/r06_ab_crt_compiled.txt).  The kernel's time is its loads -- two
  // sub-rows at three folded positions per prime -- and its multiply-adds, twice the metric ring's for rows twice as long, not its indexing.)
  // (S == 1, FOLD) compile-time; the first pass over 16 or 24 words, whichever holds the window
  int rc = 0;
  auto go = [&](auto nwm, auto ss, auto ff) -> int {
    constexpr int NWM = decltype(nwm)::value, SS = decltype(ss)::value, FF = decltype(ff)::value;
    PROF_KERNEL(ctx, PROF_CRT, (crt32_scale_generic_kernel<NWM, false, SS, FF>));
    crt32_scale_generic_kernel<NWM, false, SS, FF><<<grid, 128, 0, ctx->stream>>>(d_t, nrow, n_out, off, c->NP, logQ, J0, NW, c->WT, c->pr, c->d_cinv, c->d_inv57, c->d_Mw, d_parts, fl, wm ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (!ctx->opt.crt_skip_cleanup) {
      crt32_scale_generic_kernel<T32_GEN_NWX, true, SS, FF><<<grid, 128, 0, ctx->stream>>>(d_t, nrow, n_out, off, c->NP, logQ, 0, WU, c->WT, c->pr, c->d_cinv, c->d_inv57, c->d_Mw, d_parts, fl, wm ? 1 : 0);
      HIP_TRY(hipGetLastError());
    }
    return 0;
  };
  auto go_sf = [&](auto nwm) {      // (a32_with_S: a run-time value of a small range as a compile-time constant)
    a32_with_S<0, 1>(S == 1 ? 1 : 0, [&](auto ss) { a32_with_S<0, 2>(fold, [&](auto ff) { rc = go(nwm, ss, ff); }); });
  };
  if (NW <= 16) go_sf(std::integral_constant<int, 16>{}); else go_sf(std::integral_constant<int, T32_GEN_NW>{});
  return rc;
}

// ---- pairs (fhesi_ct_mul_relin_batch_dev): a, b [count][2][phi(m)][nlimbs] -> d_parts [count * 3][ceil(logQ/64)][phi(m)]: the scaled-down tProd as ByteDecomp takes it
int launch_tensor32(fhesi_ctx* ctx, u64 p, const u64* d_a, const u64* d_b, int nlimbs, int logQ, i64 count, u64* d_parts, bool parts_wm) {
  T32Config* c;
  FHESI_TRY(t32_config(ctx, p, nlimbs, logQ, 1, &c));
  if (!count) return 0;
  const fhesi_tensor32* x = ctx->tensor32;
  const int NP = c->NP, S = x->S;
  const i64 nrow = t32_nrow(ctx);
  void *d_r, *d_t;
  FHESI_TRY(ws_reserve(ctx, 5, (size_t)count * 4 * NP * nrow * 4, &d_r));
  FHESI_TRY(ws_reserve(ctx, 1, (size_t)count * 3 * NP * nrow * 4, &d_t));
  FHESI_TRY(t32_rns(ctx, c, d_a, d_b, count * 4, 0, true, (u32*)d_r));
  FHESI_TRY(t32_fwd(ctx, c, (u32*)d_r, count * 4));
  const dim3 grid((unsigned)(count >= 8 ? ((count + 7) / 8) * 24 : count * 3), (unsigned)(NP << S));      // (groups of 8 ciphertexts x 3 rows, or the rows themselves: see the kernel)
  FHESI_TRY(t32_inv<true>(ctx, c, (u32*)d_t, count * 3, grid, (const u32*)d_r));
  return t32_crt(ctx, c, (const u32*)d_t, count * 3, c->pr.closing, d_parts, parts_wm);
}

// ---- sums of products per group (fhesi_ct_mul_sum_relin_dev)
int tensor32_sum_begin(fhesi_ctx* ctx, u64 p, int nlimbs, int logQ, i64 gmax) {
  T32Config* c;
  FHESI_TRY(t32_config(ctx, p, nlimbs, logQ, gmax, &c));
  ctx->tensor32->cur = c;
  return 0;
}
size_t tensor32_sum_bytes(const fhesi_ctx* ctx, i64 ngroups) { return (size_t)ngroups * 3 * ctx->tensor32->cur->NP * t32_nrow(ctx) * 4; }
// d_ops: [nua + nub][2][phi(m)][nlimbs] (the a operands first); slots / segments on the device; d_sum [ng][3][NP][nrow]
int tensor32_sum_pass(fhesi_ctx* ctx, const u64* d_ops, i64 nua, i64 nub, const int* d_slot_a, const int* d_slot_b, const int* d_seg, i64 ng, i64 nterms, bool accumulate, void* d_sum) {
  const T32Config* c = ctx->tensor32->cur;
  const i64 nrow = t32_nrow(ctx), n = ctx->phim;
  void* d_r;
  FHESI_TRY(ws_reserve(ctx, 0, (size_t)(nua + nub) * 2 * c->NP * nrow * 4, &d_r));
  const u64* d_b = d_ops + (size_t)nua * 2 * n * c->nl;
  FHESI_TRY(t32_rns(ctx, c, d_ops, d_b, (nua + nub) * 2, nua * 2, false, (u32*)d_r));
  FHESI_TRY(t32_fwd(ctx, c, (u32*)d_r, (nua + nub) * 2));
  const u32* ra = (const u32*)d_r;
  const u32* rb = ra + (size_t)nua * 2 * c->NP * nrow;
  ProfScope prof(ctx, PROF_TENSOR, (double)nterms);
  PROF_KERNEL(ctx, PROF_TENSOR, tensor_sum32_kernel);
  grid_chunks(ng, [&](i64 done, i64 cnt) {
    dim3 grid((unsigned)(nrow / 256), (unsigned)c->NP, (unsigned)cnt);
    tensor_sum32_kernel<<<grid, 256, 0, ctx->stream>>>(ra, rb, d_slot_a, d_slot_b, d_seg + done, accumulate ? 1 : 0, (u32*)d_sum + (size_t)done * 3 * c->NP * nrow, nrow, c->NP, c->pr);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}
int tensor32_sum_finish(fhesi_ctx* ctx, void* d_sum, i64 ng, u64* d_parts, bool parts_wm) {
  const T32Config* c = ctx->tensor32->cur;
  const dim3 grid((unsigned)(ng * 3), (unsigned)(c->NP << ctx->tensor32->S));
  FHESI_TRY(t32_inv<false>(ctx, c, (u32*)d_sum, ng * 3, grid, nullptr));
  return t32_crt(ctx, c, (const u32*)d_sum, ng * 3, c->pr.closing, d_parts, parts_wm);
}
