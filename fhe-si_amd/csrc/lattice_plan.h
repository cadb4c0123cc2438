// lattice_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/lattice_plan_check.cpp): the plans of a strided / dilated
// convolution and of a sum pooling on packed slots whose live pixels sit on a lattice of the plane (fhesi_conv2d_lattice_*, fhesi_pool2d_plan,
// fhesi_ct_pool2d_dev), and the conditions they are refused on.  tests/lattice_model.py is the normative statement; this header follows it.
//
// The plane H x W of conv_plan.h is never compacted: after a stride of 2 the live pixels stay on every second row and column, and the next layer reads
// them with its offsets stretched.  Input step (sy, sx), sy | H, sx | W: logical pixel (a, b) of the Hl x Wl = H/sy x W/sx logical plane at physical
// pixel (a sy, b sx); slots off the lattice are don't care.  Stride (ty, tx), ty | Hl, tx | Wl; dilation (ey, ex); output step (sy ty, sx tx).
//   out[I](a', b') = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](a' ty + (dy - ah) ey, b' tx + (dx - aw) ex),  logical pixels outside Hl x Wl = 0,
//   every output slot off the output lattice exactly 0 (bias included).
// Offset t = dy kw + dx in physical pixels: u = (dy - ah) ey sy, v = (dx - aw) ex sx, amount a_t = (u W + v) mod cols,
//   mask mu_t[i] = [sy ty | y and sx tx | x and 0 <= y + u < H and 0 <= x + v < W];  the flat and the split form as in conv_plan.h, the split form's
//   plaintexts moved back by the giant amount (u W) mod cols.  Key switches and the planner's rule: conv_plan.h's.  With step, stride and dilation all
//   (1, 1) the refusals, the plan and every word of the plaintexts are those of conv_plan.h.
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

struct LatticeGeom { int64_t sy = 1, sx = 1, ty = 1, tx = 1, ey = 1, ex = 1; };      // step, stride, dilation
struct LatticeShape { ConvShape c; LatticeGeom g; };

// a b clamped into [-2^62, 2^62]: an offset that absurd has an empty mask whatever its exact value
inline int64_t lattice_mul(int64_t a, int64_t b) {
  const __int128 r = (__int128)a * b, top = (__int128)1 << 62;
  return (int64_t)(r > top ? top : r < -top ? -top : r);
}
inline int64_t lattice_u(const LatticeShape& s, int64_t dy) { return lattice_mul(lattice_mul(dy - s.c.ah, s.g.ey), s.g.sy); }
inline int64_t lattice_v(const LatticeShape& s, int64_t dx) { return lattice_mul(lattice_mul(dx - s.c.aw, s.g.ex), s.g.sx); }

// nullptr, or the condition the shape breaks, written into `why` (the order fhesi_conv2d_lattice_plan checks them in; conv_refused's with the geometry's
// three conditions between the plane and the anchor)
inline const char* lattice_refused(const LatticeShape& s, int form, char* why, size_t len) {
  const long long cols = s.c.cols, H = s.c.H, W = s.c.W, Cin = s.c.Cin, Cout = s.c.Cout, kh = s.c.kh, kw = s.c.kw, ah = s.c.ah, aw = s.c.aw;
  const long long sy = s.g.sy, sx = s.g.sx, ty = s.g.ty, tx = s.g.tx, ey = s.g.ey, ex = s.g.ex;
  if (cols < 1 || cols > ((int64_t)1 << 20)) { std::snprintf(why, len, "a row of %lld slots outside [1, 2^20]", cols); return why; }
  if (H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1) {
    std::snprintf(why, len, "a %lld x %lld plane, %lld -> %lld channels, a %lld x %lld kernel (every size at least 1)", H, W, Cin, Cout, kh, kw);
    return why;
  }
  if (H > cols || W > cols || H * W > cols || cols % (H * W)) { std::snprintf(why, len, "the plane of %lld x %lld pixels does not divide the row of %lld slots", H, W, cols); return why; }
  if (sy < 1 || sx < 1 || ty < 1 || tx < 1 || ey < 1 || ex < 1) {
    std::snprintf(why, len, "a step (%lld, %lld), a stride (%lld, %lld), a dilation (%lld, %lld) (every factor at least 1)", sy, sx, ty, tx, ey, ex);
    return why;
  }
  if (H % sy || W % sx) { std::snprintf(why, len, "the step (%lld, %lld) does not divide the %lld x %lld plane", sy, sx, H, W); return why; }
  if ((H / sy) % ty || (W / sx) % tx) {
    std::snprintf(why, len, "the stride (%lld, %lld) does not divide the logical plane of %lld x %lld pixels", ty, tx, H / sy, W / sx);
    return why;
  }
  if (ah < 0 || ah >= kh || aw < 0 || aw >= kw) { std::snprintf(why, len, "the anchor (%lld, %lld) is outside the %lld x %lld kernel", ah, aw, kh, kw); return why; }
  for (long long dy = 0; dy < kh; ++dy)
    for (long long dx = 0; dx < kw; ++dx) {
      const long long u = lattice_u(s, dy), v = lattice_v(s, dx);
      if (u <= -H || u >= H || v <= -W || v >= W) {
        std::snprintf(why, len, "the offset (%lld, %lld) has an empty mask on the %lld x %lld plane", u, v, H, W);
        return why;
      }
    }
  // (kh < 2 H and kw < 2 W from here on: no product below leaves 64 bits before it is compared)
  if (Cout > kConvMaxRows || Cin > kConvMaxRows || Cout * Cin > kConvMaxRows || Cout * Cin * kh * kw > kConvMaxRows) {
    std::snprintf(why, len, "%lld x %lld channel pairs of %lld offsets per handle, 1 .. 65535 plaintexts are taken", Cout, Cin, kh * kw);
    return why;
  }
  if (form < 0 || form > 2) { std::snprintf(why, len, "form %d (0 the planner's, 1 flat, 2 split)", form); return why; }
  return nullptr;
}

struct LatticeConvPlan {
  ConvPlan p;                    // form, nh, key switches, terms and amounts as conv_plan.h lists them
  int64_t oy = 1, ox = 1;        // the output step
};
// a shape lattice_refused admits
inline LatticeConvPlan lattice_conv_plan(const LatticeShape& s, int form) {
  LatticeConvPlan out;
  ConvPlan& pl = out.p;
  const ConvShape& c = s.c;
  pl.form = form ? form : (conv_key_switches(c, 2) < conv_key_switches(c, 1) ? 2 : 1);
  pl.key_switches = conv_key_switches(c, pl.form);
  if (pl.form == 1) {
    pl.nh = (int)(c.kh * c.kw);
    pl.terms = c.Cin * c.kh * c.kw;
    for (int64_t dy = 0; dy < c.kh; ++dy)
      for (int64_t dx = 0; dx < c.kw; ++dx) pl.amounts.push_back(conv_mod(lattice_u(s, dy) * c.W + lattice_v(s, dx), c.cols));
  } else {
    pl.nh = (int)(c.kw + c.kh);
    pl.terms = c.Cin * c.kw;
    for (int64_t dx = 0; dx < c.kw; ++dx) pl.amounts.push_back(conv_mod(lattice_v(s, dx), c.cols));
    for (int64_t dy = 0; dy < c.kh; ++dy) pl.amounts.push_back(conv_mod(lattice_u(s, dy) * c.W, c.cols));
  }
  out.oy = s.g.sy * s.g.ty;
  out.ox = s.g.sx * s.g.tx;
  return out;
}

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
