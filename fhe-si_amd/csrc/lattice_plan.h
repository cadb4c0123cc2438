// lattice_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/lattice_plan_check.cpp): the plan of a sum pooling on packed
// slots whose live pixels sit on a lattice of the plane (fhesi_pool2d_plan, fhesi_ct_pool2d_dev), and the conditions it is refused on.  The lattice itself and
// the strided / dilated convolution on it: conv_plan.h.  tests/lattice_model.py is the normative statement; this header follows it.
//
// Sum pooling: non-overlapping windows of kh x kw logical pixels that tile the plane (kh sy | H, kw sx | W), so no window crosses a plane border, no mask
// is needed and NO plaintext product is taken:  out = sum_{dy < kh} rot_{(dy sy W) mod cols}( sum_{dx < kw} rot_{(dx sx) mod cols}(in) ), the window's sum
// at its top left pixel, output step (sy kh, sx kw); slots off the output lattice hold the cyclic sums the formula gives.  It is a SUM: the caller folds
// 1 / (kh kw) into the next layer's weights.  Form 1: per direction the k - 1 rotations hoisted from ONE digit set, summed with the input as base --
// (kw - 1) + (kh - 1) key switches over two key-switch levels.  Form 2, kw and kh powers of two: doubling folds y <- y + rot(y) by sx 2^j, then by
// sy W 2^j -- log2 kw + log2 kh key switches and as many levels.  Form 0: the form of fewer key switches, form 1 on a tie (fewer levels).  Global
// pooling is kh = Hl, kw = Wl.  Overlapping or padded pooling is no tiling: it stays a convolution with a constant kernel, run with Cin = Cout = 1 over
// `count`.
#pragma once
#include "conv_plan.h"

// ------------------------------------------------------------------------------------------------ sum pooling
struct PoolShape { int64_t cols, H, W, kh, kw, sy, sx; };
inline bool pool_pow2(int64_t k) { return k >= 1 && !(k & (k - 1)); }
inline int pool_log2(int64_t k) { int l = 0; while (((int64_t)1 << l) < k) ++l; return l; }

// nullptr, or the condition the shape breaks, written into `why` (the order fhesi_pool2d_plan checks them in)
inline const char* pool_refused(const PoolShape& s, int form, char* why, size_t len) {
  const long long cols = s.cols, H = s.H, W = s.W, kh = s.kh, kw = s.kw, sy = s.sy, sx = s.sx;
  if (cols < 1 || cols > ((int64_t)1 << 20)) { std::snprintf(why, len, "a row of %lld slots outside [1, 2^20]", cols); return why; }
  if (H < 1 || W < 1 || kh < 1 || kw < 1 || sy < 1 || sx < 1) {
    std::snprintf(why, len, "a %lld x %lld plane, a %lld x %lld window, a step (%lld, %lld) (every size at least 1)", H, W, kh, kw, sy, sx);
    return why;
  }
  if (H > cols || W > cols || H * W > cols || cols % (H * W)) { std::snprintf(why, len, "the plane of %lld x %lld pixels does not divide the row of %lld slots", H, W, cols); return why; }
  if (H % sy || W % sx) { std::snprintf(why, len, "the step (%lld, %lld) does not divide the %lld x %lld plane", sy, sx, H, W); return why; }
  // (sy <= H and sx <= W from here on; a window larger than the logical plane cannot tile it)
  if (kh > H / sy || kw > W / sx || (H / sy) % kh || (W / sx) % kw) {
    std::snprintf(why, len, "windows of %lld x %lld pixels do not tile the logical plane of %lld x %lld pixels", kh, kw, H / sy, W / sx);
    return why;
  }
  if (form < 0 || form > 2) { std::snprintf(why, len, "form %d (0 the planner's, 1 hoisted sums, 2 doubling)", form); return why; }
  if (form == 2 && !(pool_pow2(kh) && pool_pow2(kw))) { std::snprintf(why, len, "form 2 (doubling) takes windows of powers of two, not %lld x %lld", kh, kw); return why; }
  return nullptr;
}
inline int64_t pool_key_switches(const PoolShape& s, int form) {
  return form == 1 ? (s.kw - 1) + (s.kh - 1) : pool_log2(s.kw) + pool_log2(s.kh);
}
struct PoolPlan {
  int form = 0, nh = 0, nhor = 0;      // 1 hoisted sums, 2 doubling; the matrices the run call takes, the horizontal ones among them
  int64_t key_switches = 0;            // per ciphertext
  int levels = 0;                      // key switches one behind the other
  std::vector<int64_t> amounts;        // the horizontal ones first, then the vertical ones; none is 0
  int64_t oy = 1, ox = 1;              // the output step
};
// a shape pool_refused admits.  form = 0: the form of fewer key switches, of equal ones form 1 (fewer levels)
inline PoolPlan pool_plan(const PoolShape& s, int form) {
  PoolPlan pl;
  const bool can2 = pool_pow2(s.kh) && pool_pow2(s.kw);
  pl.form = form ? form : (can2 && pool_key_switches(s, 2) < pool_key_switches(s, 1) ? 2 : 1);
  pl.key_switches = pool_key_switches(s, pl.form);
  if (pl.form == 1) {
    for (int64_t dx = 1; dx < s.kw; ++dx) pl.amounts.push_back(conv_mod(dx * s.sx, s.cols));
    pl.nhor = (int)pl.amounts.size();
    for (int64_t dy = 1; dy < s.kh; ++dy) pl.amounts.push_back(conv_mod(dy * s.sy * s.W, s.cols));
    pl.levels = (s.kw > 1) + (s.kh > 1);
  } else {
    for (int64_t a = 1; a < s.kw; a *= 2) pl.amounts.push_back(conv_mod(a * s.sx, s.cols));
    pl.nhor = (int)pl.amounts.size();
    for (int64_t a = 1; a < s.kh; a *= 2) pl.amounts.push_back(conv_mod(a * s.sy * s.W, s.cols));
    pl.levels = (int)pl.key_switches;
  }
  pl.nh = (int)pl.amounts.size();
  pl.oy = s.sy * s.kh;
  pl.ox = s.sx * s.kw;
  return pl;
}
