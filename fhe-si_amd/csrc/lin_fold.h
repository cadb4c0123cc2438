// lin_fold.h -- the fold of a linear-convolution ring (fhesi_ctx::lin_q, lin_s) as the closing kernels take it: packed on the host, taken apart
// once per thread on the device (kernels_crt.hip: g32_fold and the position tables; kernels_tensor32.hip: crt32_scale_generic_kernel).
#pragma once
#include <cassert>
#include "fhesi_internal.h"

// ONE kernel argument: the offset (ctx->lin_q) plus (stride - 1) 2^32, negative for an odd m -- so the sign of the argument is the kind of
// fold (`fold > 0`: m = 2Q) and its magnitude is NOT the offset: every reader goes through lin_fold_pos.  For
// s = 1 that is the offset itself, and a kernel that never reads the argument (FOLD = 0, FS = 0 with compiled shapes) keeps its argument list.
static inline i64 lin_fold_pack(i64 off, i64 s, bool odd) {
  assert(off > 0 && off < ((i64)1 << 32) && s >= 1 && s < ((i64)1 << 31));      // (m < 2^20: FHEContext.cpp:89)
  const i64 v = off + ((s - 1) << 32); return odd ? -v : v;
}
// ... and taken apart once per thread, outside every loop over primes and limbs: the offset, the third position phi + (j mod s) and the
// parity of floor(j / s).  j and s are below 2^20: 32-bit division, skipped (wave-uniformly) for s = 1.
__device__ __forceinline__ void lin_fold_pos(i64 fold, i64 j, i64 n, u32& off, u32& top, bool& odd) {
  const u64 a = (u64)(fold < 0 ? -fold : fold);
  off = (u32)a;
  const u32 s = (u32)(a >> 32) + 1, ju = (u32)j;
  const u32 b = s == 1 ? ju : ju / s;
  top = (u32)n + (ju - b * s);
  odd = (b & 1) != 0;
}
