// conv_plan.h -- host only (no HIP header; tested stand-alone under sanitizers, tests/host/conv_plan_check.cpp): the plan of a 2-D convolution on packed
// slots (fhesi_conv2d_*), the conditions it is refused on, and the index lists of the ONE plaintext sum that matvec_run (capi_pipeline.hip) hands to
// fhesi_ct_plain_sum_dev -- for the dense grids as for the convolution.  tests/conv_model.py is the normative statement; this header follows it.
//
// An H x W plane, P = H W | cols, pixel (y, x) of image i div P at slot i, (i mod P) = y W + x.  Offset t = dy kw + dx of a kh x kw kernel anchored at
// (ah, aw): u = dy - ah, v = dx - aw, mask mu_{u,v}[i] = [0 <= y + u < H and 0 <= x + v < W].  Where the mask is 1, i + u W + v stays in the P-block of i.
//   flat   out[I] = sum_J sum_t w^{IJ}_t (*) rot_{a_t}(in[J]) + b[I],                              a_t = (u W + v) mod cols
//   split  out[I] = sum_dy rot_{(u W) mod cols}( sum_J sum_dx w'^{IJ}_t (*) rot_{v mod cols}(in[J]) ) + b[I],  w'_t[i] = w_t[(i - u W) mod cols]
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int64_t kConvMaxRows = 65535;      // the plaintexts of one fhesi_plain

struct ConvShape { int64_t cols, H, W, Cin, Cout, kh, kw, ah, aw; };
inline int64_t conv_mod(int64_t a, int64_t n) { const int64_t r = a % n; return r < 0 ? r + n : r; }

// nullptr, or the condition the shape breaks, written into `why` (the order fhesi_conv2d_plan checks them in)
inline const char* conv_refused(const ConvShape& s, int form, char* why, size_t len) {
  const long long cols = s.cols, H = s.H, W = s.W, Cin = s.Cin, Cout = s.Cout, kh = s.kh, kw = s.kw, ah = s.ah, aw = s.aw;
  if (cols < 1 || cols > ((int64_t)1 << 20)) { std::snprintf(why, len, "a row of %lld slots outside [1, 2^20]", cols); return why; }
  if (H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1) {
    std::snprintf(why, len, "a %lld x %lld plane, %lld -> %lld channels, a %lld x %lld kernel (every size at least 1)", H, W, Cin, Cout, kh, kw);
    return why;
  }
  if (H > cols || W > cols || H * W > cols || cols % (H * W)) { std::snprintf(why, len, "the plane of %lld x %lld pixels does not divide the row of %lld slots", H, W, cols); return why; }
  if (ah < 0 || ah >= kh || aw < 0 || aw >= kw) { std::snprintf(why, len, "the anchor (%lld, %lld) is outside the %lld x %lld kernel", ah, aw, kh, kw); return why; }
  for (long long dy = 0; dy < kh; ++dy)
    for (long long dx = 0; dx < kw; ++dx) {
      const long long u = dy - ah, v = dx - aw;
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

struct ConvPlan {
  int form = 0, nh = 0;                // 1 flat, 2 split; the matrices the run call takes
  int64_t key_switches = 0, terms = 0; // per item; the longest plaintext sum
  std::vector<int64_t> amounts;        // flat: entry t; split: the kw babies, then the kh giants.  0 exactly at the anchor
};
inline int64_t conv_key_switches(const ConvShape& s, int form) {
  return form == 1 ? s.Cin * (s.kh * s.kw - 1) : s.Cin * (s.kw - 1) + s.Cout * (s.kh - 1);
}
// a shape conv_refused admits.  form = 0: the form of fewer key switches, of equal ones flat (one key-switch level less)
inline ConvPlan conv_plan(const ConvShape& s, int form) {
  ConvPlan pl;
  pl.form = form ? form : (conv_key_switches(s, 2) < conv_key_switches(s, 1) ? 2 : 1);
  pl.key_switches = conv_key_switches(s, pl.form);
  if (pl.form == 1) {
    pl.nh = (int)(s.kh * s.kw);
    pl.terms = s.Cin * s.kh * s.kw;
    for (int64_t dy = 0; dy < s.kh; ++dy)
      for (int64_t dx = 0; dx < s.kw; ++dx) pl.amounts.push_back(conv_mod((dy - s.ah) * s.W + (dx - s.aw), s.cols));
  } else {
    pl.nh = (int)(s.kw + s.kh);
    pl.terms = s.Cin * s.kw;
    for (int64_t dx = 0; dx < s.kw; ++dx) pl.amounts.push_back(conv_mod(dx - s.aw, s.cols));
    for (int64_t dy = 0; dy < s.kh; ++dy) pl.amounts.push_back(conv_mod((dy - s.ah) * s.W, s.cols));
  }
  return pl;
}

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
