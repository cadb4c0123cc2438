// slots_pow2_core.inc -- the negacyclic transform of length n modulo a run-time prime p < 2^31 on a row of 32-bit words in LDS: the direct path
// of the two-row slot spaces.  ONE body for kernels_slots_pow2.hip (one space per launch, the record passed by value) and
// kernels_slots_basis.hip (k channels per launch, an array of records indexed by blockIdx.y).  Included once per translation unit, after
// fhesi_internal.h.  The layout, the butterflies and the pass structure are described at the head of kernels_slots_pow2.hip.
typedef fhesi_slots::Tw SpTw;

static constexpr int SP2_T = 1024;     // threads of the largest rows; smaller rows take n / 8 (one item of the three-stage passes each), at least one wave

struct Pow2Dev {
  int logn;
  u32 n, p;
  u64 p64, one_sh;                     // floor(2^64 / p): reduces any 64-bit word (the caller's values may be any int64)
  const SpTw *fwd, *inv;               // [n] each
  const u32* pos;                      // [n]
  SpTw ninv, ninv_w1;
};

__device__ __forceinline__ u32 sp2_pad(u32 a) { return a + (a >> 5); }
__device__ __forceinline__ u32 sp2_red(i64 v, u64 p, u64 one_sh) {                 // any int64 -> [0, p)
  const u64 a = v < 0 ? (u64)0 - (u64)v : (u64)v;
  const u64 r = d_shoup(a, 1, one_sh, p);
  return (u32)((v < 0 && r) ? p - r : r);
}
__device__ __forceinline__ u32 sp2_mul(u32 y, SpTw t, u32 p) { return y * t.w - __umulhi(y, t.wp) * p; }       // any y -> [0, 2p)
__device__ __forceinline__ u32 sp2_add(u32 x, u32 y, u32 twop) { const u32 ny = twop - y; return x >= ny ? x - ny : x + y; }   // [0, 2p)^2 -> [0, 2p), no 33rd bit
__device__ __forceinline__ u32 sp2_sub(u32 x, u32 y, u32 twop) { return x >= y ? x - y : x - y + twop; }
// Cooley-Tukey: X' = X + w Y, Y' = X - w Y;  Gentleman-Sande: X' = X + Y, Y' = (X - Y) w.  Values stay in [0, 2p).
__device__ __forceinline__ void sp2_ct(u32& x, u32& y, SpTw t, u32 p) {
  const u32 twop = 2 * p, T = sp2_mul(y, t, p), X = x;
  x = sp2_add(X, T, twop);
  y = sp2_sub(X, T, twop);
}
__device__ __forceinline__ void sp2_gs(u32& x, u32& y, SpTw t, u32 p) {
  const u32 twop = 2 * p, X = x, Y = y;
  x = sp2_add(X, Y, twop);
  y = sp2_mul(sp2_sub(X, Y, twop), t, p);
}

// Stages s .. s + r - 1 of the transform (stage s has 2^s groups, distance n >> (s + 1)) on one item of 2^r words, q = n >> (s + r) apart,
// inside group i of stage s.  Stage s + u pairs the registers k, k + (R >> (u + 1)); its group is (i << u) + (k >> (r - u)).
template <int r, bool FWD>
__device__ __forceinline__ void sp2_pass(u32* __restrict__ lds, const Pow2Dev& D, int s) {
  constexpr int R = 1 << r;
  const int lq = D.logn - s - r;
  const u32 items = D.n >> r;
  const SpTw* __restrict__ tw = FWD ? D.fwd : D.inv;
  for (u32 w = threadIdx.x; w < items; w += blockDim.x) {
    const u32 i = w >> lq, o = w & ((1u << lq) - 1);
    const u32 base = (i << (lq + r)) + o;
    u32 e[R];
#pragma unroll
    for (int k = 0; k < R; ++k) e[k] = lds[sp2_pad(base + ((u32)k << lq))];
#pragma unroll
    for (int uu = 0; uu < r; ++uu) {
      const int u = FWD ? uu : r - 1 - uu;
      const int hk = R >> (u + 1);
      const u32 g0 = (1u << (s + u)) + (i << u);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (k & hk) continue;
        if (FWD) sp2_ct(e[k], e[k + hk], tw[g0 + (k >> (r - u))], D.p);
        else if (s + u) sp2_gs(e[k], e[k + hk], tw[g0 + (k >> (r - u))], D.p);
        else {                          // the last stage of the inverse carries n^-1
          const u32 twop = 2 * D.p, X = e[k], Y = e[k + hk];
          e[k] = sp2_mul(sp2_add(X, Y, twop), D.ninv, D.p);
          e[k + hk] = sp2_mul(sp2_sub(X, Y, twop), D.ninv_w1, D.p);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) lds[sp2_pad(base + ((u32)k << lq))] = e[k];
  }
  __syncthreads();
}
template <bool FWD>
__device__ __forceinline__ void sp2_transform(u32* __restrict__ lds, const Pow2Dev& D) {
  const int r0 = D.logn % 3;
  if (FWD) {
    if (r0 == 1) sp2_pass<1, true>(lds, D, 0);
    if (r0 == 2) sp2_pass<2, true>(lds, D, 0);
    for (int s = r0; s < D.logn; s += 3) sp2_pass<3, true>(lds, D, s);
  } else {
    for (int s = D.logn - 3; s >= r0; s -= 3) sp2_pass<3, false>(lds, D, s);
    if (r0 == 1) sp2_pass<1, false>(lds, D, 0);
    if (r0 == 2) sp2_pass<2, false>(lds, D, 0);
  }
}

// the record of one space (host side): tables built by slots_pow2_build
static Pow2Dev sp2_dev(const fhesi_slots* s) {
  const hm::SlotSpace& S = s->S;
  Pow2Dev D;
  D.n = (u32)S.phim; D.p = (u32)S.p; D.p64 = S.p; D.one_sh = hm::shoup(1, S.p);
  D.logn = 0;
  while ((1u << D.logn) < D.n) ++D.logn;
  D.fwd = s->d_p2tw; D.inv = s->d_p2tw + D.n; D.pos = s->d_p2pos;
  D.ninv = s->p2ninv; D.ninv_w1 = s->p2ninv_w1;
  return D;
}
static unsigned sp2_threads(u32 n) { return (unsigned)std::min<u32>(SP2_T, std::max<u32>(64, n / 8)); }
static size_t sp2_shmem(u32 n) { return (size_t)(n + (n >> 5)) * sizeof(u32); }
