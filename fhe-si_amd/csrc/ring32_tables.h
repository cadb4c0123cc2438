// ring32_tables.h -- the host tables of the 30-bit rows, built once: the twiddle tables of the row transforms of ntt32_core.inc (ring32_build),
// which the key switch through four auxiliary primes (kernels_aux32.hip) and the tensor half through 35 .. 72 of them (kernels_tensor32.hip)
// both upload as they come, and the tensor half's conversion tables (conv32_build: residues in, CRT out).  Host-only and free of HIP headers
// (like hostbig.h, which it builds on): tests/host/ring32_tables_dump.cpp prints every table for tests/test_ring32_tables.py to compare with a
// model in Python's integers, so a constant that moves is moved here, once, and checked on the CPU first.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "hostbig.h"

// ---- what the kernels of ntt32_core.inc share with the builders (global names: the kernels' symbols carry Tw32)
struct Tw32 { uint32_t w, wp; };          // constant and floor(w 2^32 / p)
static constexpr int A32_LOGN = 14, A32_N = 1 << A32_LOGN;      // the sub-transform: rows of 2^(14 + S) are 2^S of them behind S head stages
// S = 2: constants per prime of the stand-alone head / tail passes (ntt32_head2_kernel, ntt32_tail2_kernel):
// [0..2] head w0, w1a, w1b;  [4..7] tail 1/2, w1a^-1 / 2, w1b^-1 / 2, w0^-1 / 2
static constexpr int A32_HT = 8;
// S >= 3: per prime [2][A32_HSN(S)] -- direction 0: psi^brv(idx) (stage s, group i: idx = 2^s + i); direction 1: psi^-brv(idx) and, at the end,
// the constants of the last inverse stage: 2^-S, psi^-brv(1) 2^-S, and both times 2^32 (rows that carry dot32's factor 2^-32)
constexpr int A32_HSN(int S) { return (1 << S) + 4; }
// mu61 = floor(2^(32 + sh) / p) with sh = 29 for primes of 30 bits, 28 for primes of 29 bits
constexpr uint32_t t32_shift(uint32_t p) { return (p >> 29) ? 29u : 28u; }

// out[idx] = psi^brv(idx) (with its Shoup word) for idx < 2^lg -- running powers in natural order scattered to their bit-reversed
// slots, two 64-bit divisions per entry (p < 2^30).  (A power per entry cost 2.7 s on the first call of a ring with rows of 2^20.)
static inline void a32_bitrev_powers(uint64_t p, uint64_t psi, int lg, std::vector<Tw32>& out) {
  const uint64_t n = (uint64_t)1 << lg;
  uint64_t w = 1;
  for (uint64_t e = 0; e < n; ++e) { out[hm::brv(e, lg)] = Tw32{(uint32_t)w, (uint32_t)((w << 32) / p)}; w = w * psi % p; }
}
// The per-lane twiddles of the last four stages (table entries 1024 .. 16383) in the ORDER THE WAVES LOAD THEM (ntt32_core.inc, A32_LOAD_TC):
// every block of 2^14 entries (one per prime and sub-block) has its regions [1024 << v, 2048 << v), v = 0 .. 3, re-ordered:
// pair (t, q) of stage v  ->  position ((t >> 6) * 2^v + q) * 64 + (t & 63)  of that stage's region
static inline void a32_permute_phase_c(std::vector<Tw32>& t) {
  std::vector<Tw32> tmp;
  for (size_t base = 0; base + ((size_t)1 << 14) <= t.size(); base += (size_t)1 << 14)
    for (int v = 0; v < 4; ++v) {
      const size_t off = base + ((size_t)1024 << v), nq = (size_t)1 << v;      // nq 16-byte pairs per thread
      tmp.assign(t.begin() + off, t.begin() + off + ((size_t)1024 << v));
      for (size_t tid = 0; tid < 512; ++tid)
        for (size_t q = 0; q < nq; ++q) {
          const size_t src = tid * nq + q, dst = ((tid >> 6) * nq + q) * 64 + (tid & 63);
          t[off + 2 * dst] = tmp[2 * src]; t[off + 2 * dst + 1] = tmp[2 * src + 1];
        }
    }
}

namespace hm {
inline Tw32 tw32(uint64_t w, uint64_t p) { return Tw32{(uint32_t)w, (uint32_t)((w << 32) / p)}; }      // w < p < 2^32

// ---------------------------------------------------------------------------------------------- the transform tables
// per prime, what the two users derive their own constants from (psi: the prime's 2n-th root, n = 2^(14 + S) the row length)
struct Ring32Prime {
  Tw32 head, head1[2], tail;         // psi^brv(1);  psi^brv(2), psi^brv(3): the first and second head stage;  psi^-brv(1)
  uint32_t ninv;                     // 2^-14: the scaling of the sub-transform (the tail stages carry the other 2^-S)
};
struct Ring32Consts {
  int S = 0;                         // rows of 2^(14 + S)
  std::vector<uint32_t> primes;
  std::vector<Ring32Prime> pp;       // [prime]
  std::vector<uint32_t> last;        // [prime][2^S] the twiddle of the sub-block's last inverse stage: what entry 1 of its table held before the 1/n went in
};
struct Ring32Tables {
  Ring32Consts k;
  // [prime][2^S][2^14], phase-C permuted: psi^brv(idx) as a32_ct<NEGW> takes it, (-w mod 2^32, floor(w 2^32 / p)), and psi^-brv(idx) as it is
  // with entries 0 and 1 of every sub-block replaced by 1/n and w/n (n = 2^14, w: `last`) -- the last inverse stage carries the scaling.
  // Sub-block h runs stage s >= S of the row on its groups i = h 2^(s-S) + i':  own index m' + i' (m' = 2^(s-S))  <->  (m' << S) + h m' + i'
  std::vector<Tw32> fwd, inv;
  std::vector<Tw32> ht;              // [prime][A32_HT], filled at S = 2 (zero otherwise)
  std::vector<Tw32> hs;              // S >= 3: [prime][2][A32_HSN(S)]
};
// For any number of primes p = 1 mod 2^(15 + S) below 2^30 and S = 0 .. 6.  false: a prime has no 2n-th root among the powers of 2 .. 999
inline bool ring32_build(const std::vector<uint32_t>& primes, int S, Ring32Tables& t) {
  const int lg = A32_LOGN + S, NS = 1 << S, NP = (int)primes.size(), HSN = A32_HSN(S);
  const uint64_t n = (uint64_t)1 << lg;
  const size_t per_prime = (size_t)A32_N << S;
  t = Ring32Tables();
  t.k.S = S; t.k.primes = primes; t.k.pp.resize(NP); t.k.last.resize((size_t)NP * NS);
  t.fwd.assign((size_t)NP * per_prime, Tw32{0, 0}); t.inv.assign((size_t)NP * per_prime, Tw32{0, 0});
  t.ht.assign((size_t)NP * A32_HT, Tw32{0, 0}); t.hs.assign(S >= 3 ? (size_t)NP * 2 * HSN : 0, Tw32{0, 0});
  std::vector<Tw32> ff((size_t)n), fi((size_t)n);
  for (int a = 0; a < NP; ++a) {
    const uint64_t p = primes[a];
    uint64_t psi = 0;
    for (uint64_t gq = 2; gq < 1000 && !psi; ++gq) {
      const uint64_t cand = powmod(gq, (p - 1) / (2 * n), p);
      if (powmod(cand, n, p) == p - 1) psi = cand;
    }
    if (!psi) return false;
    a32_bitrev_powers(p, psi, lg, ff); a32_bitrev_powers(p, invmod(psi, p), lg, fi);       // the full tables of the n-point transform
    auto fwd_form = [](Tw32 x) { return Tw32{0u - x.w, x.wp}; };
    Tw32 *hf = &t.fwd[(size_t)a * per_prime], *hi = &t.inv[(size_t)a * per_prime];
    if (!S) {
      std::transform(ff.begin(), ff.end(), hf, fwd_form);
      std::copy(fi.begin(), fi.end(), hi);
    } else {
      for (int h = 0; h < NS; ++h)
        for (uint64_t mp = 1; mp < (uint64_t)A32_N; mp <<= 1)
          for (uint64_t ip = 0; ip < mp; ++ip) {
            hf[(size_t)h * A32_N + mp + ip] = fwd_form(ff[(mp << S) + h * mp + ip]);
            hi[(size_t)h * A32_N + mp + ip] = fi[(mp << S) + h * mp + ip];
          }
    }
    Ring32Prime& q = t.k.pp[a];
    q.head = ff[1]; q.head1[0] = ff[2]; q.head1[1] = ff[3]; q.tail = fi[1];
    const uint64_t inv2 = (p + 1) / 2;
    if (S == 2) {
      Tw32* c = &t.ht[(size_t)a * A32_HT];
      c[0] = ff[1]; c[1] = ff[2]; c[2] = ff[3];
      c[4] = tw32(inv2, p); c[5] = tw32(mulmod(fi[2].w, inv2, p), p); c[6] = tw32(mulmod(fi[3].w, inv2, p), p); c[7] = tw32(mulmod(fi[1].w, inv2, p), p);
    }
    if (S >= 3) {
      Tw32 *f = &t.hs[(size_t)a * 2 * HSN], *b = f + HSN;
      for (int idx = 1; idx < NS; ++idx) { f[idx] = ff[idx]; b[idx] = fi[idx]; }
      const uint64_t c = invmod((uint64_t)NS % p, p), cm = mulmod(c, ((uint64_t)1 << 32) % p, p);      // 2^-S and 2^-S 2^32
      b[NS] = tw32(c, p); b[NS + 1] = tw32(mulmod(fi[1].w, c, p), p); b[NS + 2] = tw32(cm, p); b[NS + 3] = tw32(mulmod(fi[1].w, cm, p), p);
    }
    const uint64_t ninv = q.ninv = (uint32_t)invmod(A32_N % p, p);
    for (int h = 0; h < NS; ++h) {
      Tw32* t0 = hi + (size_t)h * A32_N;
      t.k.last[(size_t)a * NS + h] = t0[1].w;
      t0[1] = tw32(mulmod(t0[1].w, ninv, p), p); t0[0] = tw32(ninv, p);
    }
  }
  a32_permute_phase_c(t.fwd); a32_permute_phase_c(t.inv);
  return true;
}

// ---------------------------------------------------------------------------------------------- the tensor half's conversion tables
// [NP + 1][WT] words of R bits and 64 words of padding (the generic CRT kernel multiplies a fixed number of words per row, whatever the window):
// row i = M / p_i, row NP = 2^(R WT) - M, M the product of the NP primes.  rem (optional): (M / p_i) mod p_i
inline std::vector<uint32_t> crt32_mw(const uint32_t* primes, int NP, int R, int WT, std::vector<uint64_t>* rem = nullptr) {
  std::vector<uint32_t> Mw((size_t)(NP + 1) * WT + 64);
  if (rem) rem->resize(NP);
  Big M{1};
  for (int a = 0; a < NP; ++a) M = bn_mul_small(M, primes[a]);
  for (int a = 0; a < NP; ++a) {
    Big Mi{1};
    for (int b = 0; b < NP; ++b) if (b != a) Mi = bn_mul_small(Mi, primes[b]);
    if (rem) (*rem)[a] = bn_mod_small(Mi, primes[a]);
    for (int l = 0; l < WT; ++l) Mw[(size_t)a * WT + l] = bn_word(Mi, l, R);
  }
  // 2^(R WT) - M: two's complement of M over enough limbs, read through the same word extraction (masked to R WT bits)
  Big N = bn_resized(M, (R * WT + 63) / 64 + 1);
  uint64_t carry = 1;
  for (auto& w : N) { const uint64_t v = ~w + carry; carry = (carry && v == 0) ? 1 : 0; w = v; }
  for (int l = 0; l < WT; ++l) Mw[(size_t)NP * WT + l] = bn_word(N, l, R);
  return Mw;
}
struct Conv32Tables {
  int stride = 0;                    // words per row of rns: 2 nl + 8, rounded up to whole 32-byte lines (the kernel reads them with scalar loads)
  // [2][NP][stride]: (s 2^(32k) mod p) k < 2 nl, -(s 2^(64 nl)) mod p, 2^32 mod p, mu61, p, head twiddles (w, w') x 2;  s = lift (class 0) or 1
  std::vector<uint32_t> rns;
  // [NP][2] (M / p_i)^-1 mod p_i, at S = 1 times 1/2 | times psi^-brv(1) / 2: the tail of a 2^15-point inverse (rows of 2^14 do not read it)
  std::vector<Tw32> cinv;
  std::vector<uint32_t> inv57, mu61; // [NP] floor(2^57 / p_i);  floor(2^(32 + t32_shift(p_i)) / p_i)
  std::vector<uint32_t> Mw;          // crt32_mw
  // [NP][2] the closing pair of the inverse's last stage (T32Primes: ninv, ninv_w).  S = 0: c = (M / p_i)^-1 / n and c times the last stage's twiddle --
  // the rows leave the inverse as y_i = x (M / p_i)^-1 mod p_i and the CRT kernels multiply by nothing; longer rows: 1 / n and zero
  std::vector<Tw32> closing;
};
// for the first NP primes of k, operands of nl limbs of 64 bits lifted by `lift`, table rows of WT words of R bits
inline Conv32Tables conv32_build(const Ring32Consts& k, int NP, uint64_t lift, int nl, int R, int WT) {
  const int S = k.S, NS = 1 << S;
  Conv32Tables c;
  c.stride = (2 * nl + 8 + 7) & ~7;
  c.rns.assign((size_t)2 * NP * c.stride, 0);
  c.cinv.resize((size_t)NP * 2); c.closing.resize((size_t)NP * 2); c.inv57.resize(NP); c.mu61.resize(NP);
  std::vector<uint64_t> rem;
  c.Mw = crt32_mw(k.primes.data(), NP, R, WT, &rem);
  for (int a = 0; a < NP; ++a) {
    const uint64_t p = k.primes[a];
    const Ring32Prime& q = k.pp[a];
    c.mu61[a] = (uint32_t)(((uint64_t)1 << (32 + t32_shift((uint32_t)p))) / p);
    c.inv57[a] = (uint32_t)(((uint64_t)1 << 57) / p);
    for (int cls = 0; cls < 2; ++cls) {
      uint32_t* e = &c.rns[((size_t)cls * NP + a) * c.stride];
      const uint64_t b32 = ((uint64_t)1 << 32) % p;
      uint64_t cur = cls == 0 ? lift % p : 1;
      for (int j = 0; j < 2 * nl; ++j) { e[j] = (uint32_t)cur; cur = mulmod(cur, b32, p); }
      e[2 * nl] = (uint32_t)((p - cur) % p);          // two's complement: value = unsigned - 2^(64 nl)
      e[2 * nl + 1] = (uint32_t)b32; e[2 * nl + 2] = c.mu61[a]; e[2 * nl + 3] = (uint32_t)p;
      // head stage of a 2^15-point row: psi^brv(1); padded rows of 2^16: the second head stage's psi^brv(2), psi^brv(3) (the first is a duplication)
      const Tw32 z{0, 0}, h0 = S == 2 ? q.head1[0] : (S ? q.head : z), h1 = S == 2 ? q.head1[1] : z;
      e[2 * nl + 4] = h0.w; e[2 * nl + 5] = h0.wp; e[2 * nl + 6] = h1.w; e[2 * nl + 7] = h1.wp;
    }
    const uint64_t ci = invmod(rem[a], p), inv2 = (p + 1) / 2;
    const uint64_t cn = S ? q.ninv : mulmod(ci, q.ninv, p);
    c.closing[(size_t)a * 2] = tw32(cn, p);
    c.closing[(size_t)a * 2 + 1] = S ? Tw32{0, 0} : tw32(mulmod(cn, k.last[(size_t)a * NS], p), p);
    // (rows of 2^16 and longer: the tail stages are a pass of their own, ntt32_tail2_kernel / ntt32_tailS_kernel)
    c.cinv[(size_t)a * 2] = tw32(S == 1 ? mulmod(ci, inv2, p) : ci, p);
    c.cinv[(size_t)a * 2 + 1] = tw32(S == 1 ? mulmod(ci, mulmod(q.tail.w, inv2, p), p) : ci, p);
  }
  return c;
}
}  // namespace hm
