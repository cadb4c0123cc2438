// crt32_bytes.h -- host tables of crt32_mfma_kernel (kernels_tensor32.hip): the window of the tensor half's CRT constants as balanced signed
// bytes in the operand layout of v_mfma_i32_32x32x32_i8.  Host-only and free of HIP headers (like hostbig.h, which it builds on), so that a
// plain C++ program can print the tables for tests/test_crt32_mfma_model.py to check against Python's integers.
//
// The fast CRT pass forms  F = sum_s y_s C_s  mod 2^576  over the slots s < NP (y_s the residue of prime s, below 2^30) and s = NP (y = kappa),
// C_s = words [J0, J0 + 21) of table row s of Mw, i.e. bits 448 .. 1035 of M / p_s (of 2^(R WT) - M for the kappa row); bits 448 .. 1023 of x are
// all the kernel reads, hence mod 2^576.  With y = sum_a yb_a 256^a:
//   F = sum_(s, a) yb_(s, a) D_(s, a),   D_(s, a) = 256^a C_s mod 2^576 = sum_(c < 72) d_(s, a, c) 256^c  (mod 2^576),  d in [-128, 127]
// so column c of an int8 matrix product over the depth (s, a) -- 40 slots x 4 bytes = 160, five steps of 32 -- is  S_c = sum yb d_c,  and
// F = sum_c S_c 256^c.  The instruction takes signed bytes on both sides: the kernel hands it yb - 128 (y ^ 0x80808080), which leaves every
// column short by 128 sum_(s, a) d_(s, a, c), in all  0x80808080 sum_s C_s  (mod 2^576).  That constant, less a bias of 2^22 per column, is one
// more slot of the depth (NP + 1) whose operand bytes are (1, 0, 0, 0) as they stand: the accumulators start at the bias, so every column sum
// the kernel reads is a positive number below 2^23 (|S_c| <= 37 * 4 * 128 * 128 + 128 < 2^22: exact in the int32 accumulators) and its
// carry pass is unsigned.
#pragma once
#include <cstdint>
#include <vector>

#include "hostbig.h"

namespace hm {
static constexpr int C32B_SLOTS = 40;       // depth slots: NP primes, kappa, the constant, zero padding (NP + 2 <= 40)
static constexpr int C32B_BIAS = 1 << 22;   // what the accumulators start at
static constexpr int C32B_COLS = 72;        // byte columns: bits 448 .. 1023
static constexpr int C32B_HALF = 36;        // columns per half wave: lanes 0-31 hold columns 0 .. 35 (bits 448 .. 735) of their coefficient, lanes 32-63 columns 36 .. 71
static constexpr int C32B_TILES = 3;        // 32-row output tiles: 16 accumulator registers per lane and tile, 36 of the 48 used
static constexpr int C32B_KSTEPS = 5;       // depth steps of 32 bytes = 8 slots: a lane of half h holds slots 8 ks + 4 h + (0 .. 3)
static constexpr int C32B_LIMBS = 9;        // 576 bits

struct Crt32Bytes {
  std::vector<int8_t> d;          // [slot][a][col]: balanced bytes of 256^a C_slot mod 2^576; slot NP + 1, a = 0: of the constant; zero elsewhere
  std::vector<uint32_t> aop;      // [tile][kstep][lane][4]: operand A, four bytes a = 0 .. 3 of one slot per word
};

// the column an output row of tile t holds: row m sits in lanes of half (m / 4) % 2, register 4 (m / 8) + m % 4 (tools/mfma_i8_layout.hip);
// -1: a register the kernel does not read (its row of A is zero)
inline int crt32_bytes_col(int tile, int m) {
  const int q = tile * 16 + 4 * (m >> 3) + (m & 3);
  return q < C32B_HALF ? ((m >> 2) & 1) * C32B_HALF + q : -1;
}

// Mw: [NP + 1][WT] words of R bits (row NP: 2^(R WT) - M), as t32_config builds them; the window starts at word J0 and has NW words
inline Crt32Bytes crt32_bytes_build(const uint32_t* Mw, int NP, int WT, int R, int J0, int NW) {
  Crt32Bytes t;
  t.d.assign((size_t)C32B_SLOTS * 4 * C32B_COLS, 0);
  Big sum(C32B_LIMBS, 0);
  for (int s = 0; s <= NP; ++s) {
    const Big C = bn_resized(bn_from_words(Mw + (size_t)s * WT + J0, NW, R), C32B_LIMBS);      // mod 2^576
    bn_add(sum, C);
    for (int a = 0; a < 4; ++a) {
      Big v(C);
      bn_shl(v, 8 * a);
      bn_balanced_bytes(v, C32B_COLS, &t.d[((size_t)s * 4 + a) * C32B_COLS]);
    }
  }
  {
    // the constant: 0x80808080 sum_s C_s - bias sum_c 256^c  (mod 2^576)
    Big K = bn_resized(bn_mul_small(sum, 0x80808080ull), C32B_LIMBS);
    for (int c = 0; c < C32B_COLS; ++c) {
      Big b(C32B_LIMBS, 0);
      b[0] = (bn_limb)C32B_BIAS;
      bn_shl(b, 8 * c);
      bn_sub(K, b);
    }
    bn_balanced_bytes(K, C32B_COLS, &t.d[((size_t)(NP + 1) * 4 + 0) * C32B_COLS]);
  }
  t.aop.assign((size_t)C32B_TILES * C32B_KSTEPS * 64 * 4, 0);
  for (int tile = 0; tile < C32B_TILES; ++tile)
    for (int ks = 0; ks < C32B_KSTEPS; ++ks)
      for (int l = 0; l < 64; ++l) {
        const int col = crt32_bytes_col(tile, l & 31);
        if (col < 0) continue;
        for (int tt = 0; tt < 4; ++tt) {
          const int s = ks * 8 + (l >> 5) * 4 + tt;
          uint32_t w = 0;
          for (int a = 0; a < 4; ++a) w |= (uint32_t)(uint8_t)t.d[((size_t)s * 4 + a) * C32B_COLS + col] << (8 * a);
          t.aop[(((size_t)tile * C32B_KSTEPS + ks) * 64 + l) * 4 + tt] = w;
        }
      }
  return t;
}
}  // namespace hm
