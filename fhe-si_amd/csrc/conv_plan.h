// conv_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/conv_plan_check.cpp, lattice_plan_check.cpp): the plan of a 2-D
// convolution on packed slots (fhesi_conv2d_*, fhesi_conv2d_lattice_*), the conditions it is refused on, and the index lists of the ONE plaintext sum that
// matvec_run (capi_pipeline.hip) hands to fhesi_ct_plain_sum_dev -- for the dense grids as for the convolution.  tests/conv_model.py and tests/lattice_model.py
// are the normative statements; this header follows them.  ONE refusal and ONE plan, lattice_refused and lattice_conv_plan, take the shape with a geometry --
// step, stride, dilation -- that is (1, 1) throughout by default; conv_refused and conv_plan are that case by name.
//
// An H x W plane, P = H W | cols, pixel (y, x) of image i div P at slot i, (i mod P) = y W + x.  Offset t = dy kw + dx of a kh x kw kernel anchored at
// (ah, aw): u = dy - ah, v = dx - aw, mask mu_{u,v}[i] = [0 <= y + u < H and 0 <= x + v < W].  Where the mask is 1, i + u W + v stays in the P-block of i.
//   flat   out[I] = sum_J sum_t w^{IJ}_t (*) rot_{a_t}(in[J]) + b[I],                              a_t = (u W + v) mod cols
//   split  out[I] = sum_dy rot_{(u W) mod cols}( sum_J sum_dx w'^{IJ}_t (*) rot_{v mod cols}(in[J]) ) + b[I],  w'_t[i] = w_t[(i - u W) mod cols]
//
// On a lattice the plane is never compacted: after a stride of 2 the live pixels stay on every second row and column, and the next layer reads them with its
// offsets stretched.  Input step (sy, sx), sy | H, sx | W: logical pixel (a, b) of the Hl x Wl = H/sy x W/sx logical plane at physical pixel (a sy, b sx);
// slots off the lattice are don't care.  Stride (ty, tx), ty | Hl, tx | Wl; dilation (ey, ex); output step (sy ty, sx tx).
//   out[I](a', b') = b[I] + sum_J sum_dy sum_dx K[I][J][dy][dx] in[J](a' ty + (dy - ah) ey, b' tx + (dx - aw) ex),  logical pixels outside Hl x Wl = 0,
//   every output slot off the output lattice exactly 0 (bias included).
// Offset t in physical pixels: u = (dy - ah) ey sy, v = (dx - aw) ex sx, amount a_t = (u W + v) mod cols,
//   mask mu_t[i] = [sy ty | y and sx tx | x and 0 <= y + u < H and 0 <= x + v < W];  the flat and the split form as above, the split form's plaintexts moved
//   back by the giant amount (u W) mod cols.  The key switches and the planner's rule do not depend on the geometry.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int64_t kConvMaxRows = 65535;      // the plaintexts of one fhesi_plain

struct ConvShape { int64_t cols, H, W, Cin, Cout, kh, kw, ah, aw; };
inline int64_t conv_mod(int64_t a, int64_t n) { const int64_t r = a % n; return r < 0 ? r + n : r; }

struct LatticeGeom { int64_t sy = 1, sx = 1, ty = 1, tx = 1, ey = 1, ex = 1; };      // step, stride, dilation
struct LatticeShape { ConvShape c; LatticeGeom g; };

// a b clamped into [-2^62, 2^62]: an offset that absurd has an empty mask whatever its exact value
inline int64_t lattice_mul(int64_t a, int64_t b) {
  const __int128 r = (__int128)a * b, top = (__int128)1 << 62;
  return (int64_t)(r > top ? top : r < -top ? -top : r);
}
inline int64_t lattice_u(const LatticeShape& s, int64_t dy) { return lattice_mul(lattice_mul(dy - s.c.ah, s.g.ey), s.g.sy); }
inline int64_t lattice_v(const LatticeShape& s, int64_t dx) { return lattice_mul(lattice_mul(dx - s.c.aw, s.g.ex), s.g.sx); }

struct ConvPlan {
  int form = 0, nh = 0;                // 1 flat, 2 split; the matrices the run call takes
  int64_t key_switches = 0, terms = 0; // per item; the longest plaintext sum
  std::vector<int64_t> amounts;        // flat: entry t; split: the kw babies, then the kh giants.  0 exactly at the anchor
};
inline int64_t conv_key_switches(const ConvShape& s, int form) {
  return form == 1 ? s.Cin * (s.kh * s.kw - 1) : s.Cin * (s.kw - 1) + s.Cout * (s.kh - 1);
}
// nullptr, or the condition the shape breaks, written into `why` (the order fhesi_conv2d_plan and fhesi_conv2d_lattice_plan check them in; the geometry's
// three conditions stand between the plane and the anchor, and unit factors pass them)
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
  ConvPlan p;
  int64_t oy = 1, ox = 1;        // the output step
};
// a shape lattice_refused admits.  form = 0: the form of fewer key switches, of equal ones flat (one key-switch level less)
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

// the unit geometry by name
inline const char* conv_refused(const ConvShape& s, int form, char* why, size_t len) { return lattice_refused(LatticeShape{s, LatticeGeom{}}, form, why, len); }
inline ConvPlan conv_plan(const ConvShape& s, int form) { return lattice_conv_plan(LatticeShape{s, LatticeGeom{}}, form).p; }

// The index lists of the ONE plaintext sum of a chunk of cnt items: nI output blocks, nJ input blocks, nk plaintexts per block pair in G groups of B.
//   group (I G + g) cnt + i = sum_J sum_{j < B, g B + j < nk} pool[(J nb + j) cnt + i] (*) w[(I nJ + J) nk + g B + j],   nb = min(B, nk)
// a_idx, b_idx hold nI nJ nk cnt entries, seg nI G cnt + 1.  The dense grid: nk = T diagonals; the convolution: nk = kh kw, B = kw (split) or kh kw (flat).
inline void grid_sum_lists(int nI, int nJ, int nk, int B, int G, int64_t cnt, int32_t* a_idx, int32_t* b_idx, int32_t* seg) {
  const int nb = B < nk ? B : nk;
  int64_t at = 0;
  for (int I = 0; I < nI; ++I)
    for (int g = 0; g < G; ++g)
      for (int64_t i = 0; i < cnt; ++i) {
        seg[((size_t)I * G + g) * cnt + i] = (int32_t)at;
        for (int J = 0; J < nJ; ++J)
          for (int j = 0; j < B && g * B + j < nk; ++j, ++at) { a_idx[at] = (int32_t)(((int64_t)J * nb + j) * cnt + i); b_idx[at] = (I * nJ + J) * nk + g * B + j; }
      }
  seg[(size_t)nI * G * cnt] = (int32_t)at;
}
