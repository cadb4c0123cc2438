"""GPU: DoubleCRT / SingleCRT objects over PROPER index sets on every class of row transform, bit for bit against the C oracle.

An object over a proper subset of the chain reaches the device with a slot -> prime map (prime_of_slot in the kernels, d_pos in the launchers,
h_pos for Bluestein); over the whole chain the map is null (upload_idx, capi_ctx.hip) and `prime_of_slot ? prime_of_slot[slot] : slot` takes
its cheap side.  A slot taken for a prime index is in range everywhere: nothing faults, the row comes out modulo another prime or with another
prime's twiddles, chirps, Garner constants or q_tile.  So: one case per transform class (RINGS), a chain whose five primes all differ in size
(index_sets_common.mixed_chain: 60, small, 59, 49, 60 bits), the sets [1], [1, 3], [0, 2, 4], [2, 3, 4] and the whole chain as the control in the
same case -- if the control fails too, the map is not what is wrong.

Per (ring, set S), the polynomial is centred within the product of S's primes (both ends of the range, 0, 1, -1 in front, the lower end last):
  1 from_poly over S (also 5 coefficients; n + 3 and m + 2 coefficients where n <= 2^11: the per-row path of fhesi_cmod_fft)
  2 to_poly over S, centred and positive, against the oracle AND the input integers; to_poly(index_set = T) intersects (DoubleCRT.cpp:352)
  3 cmod_fft / cmod_ifft of every prime of S (a singleton map), random evaluations and, for prime 1, all q - 1
  4 to_scrt / from_scrt / SingleCRT.assign_dcrt
  5 add_primes(complement) / remove_primes(complement): exact, the polynomial is within +-(P_S - 1) / 2
  6 scale_down_to_set and add_primes_and_scale with p = 23 (DoubleCRT.cpp:162-208, 518-558)
  7 automorph on the subset object; the full-chain operand beside it stays as it was
Rings with n >= 2^15 or m >= 8000 run 1 (without the over-long polynomials), 2, 3, 4, 6; m = 2^19 runs 1, 2, 3.  The sets of each case: RINGS.

Which kernels a case reaches with a non-null map (read from launch_ntt_fwd / launch_ntt_inv, kernels_ntt.hip, and blue_chunk, bluestein.hip; all
of them with launch_rns_reduce and launch_crt over the subset):
  m = 16, 2^11            ntt_fwd_lds<true> / ntt_inv_lds<true> (one block per row; 16: less than a wave)
  m = 2^12 .. 2^15        ntt_fwd_tile<LOGN, false> / ntt_inv_tile<LOGN>, LOGN = 11 .. 14; the small prime in its q_tile form
  m = 2^16, 2^17, 2^18    ntt_fwd_tile<14, false, S0> + ntt_fwd_tail<S0>, ntt_inv_tile<14, S0> + ntt_inv_tail<S0>, S0 = 1, 2, 3 (rb -> (slot, row),
                          grids padded to eight blocks: 1 and 2 rows under a map)
  m = 2^19                ntt_*_global_stage, ntt_*_lds<false>, bitrev_rows
  m = 45, 27              blue_pre / blue_mul (d_bhat) / blue_post, blue_phi_generic (27: Phi_m with stride 9)
  m = 45, FHESI_PHI_CONV  ... blue_mul on d_khat and blue_conv_post instead of blue_phi_generic; the same bits as the case before
  m = 101, 46             blue_phi_fast kind 1, kind 2
  m = 8422                blue_pre<., true> / blue_post<., true> (N = 2^15, head and tail stage fused), blue_phi_fast kind 2
  m = 16411, 32771        the order-free transforms with 2 and 3 head / tail stages (N = 2^16, 2^17), blue_phi_fast kind 1
  m = 17325               N = 2^16 and the reduction by convolutions as the only path (m > 16384)
The tile cases also read the instantiation the library recorded (Context.prof_kernel_name)."""
import numpy as np
import pytest

import fhe_si_amd as F
import index_sets_common as X
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu
P_MOD = 23
ALL_ITEMS = (1, 2, 3, 4, 5, 6, 7)
LARGE_ITEMS = (1, 2, 3, 4, 6)
ONE_SET = ([1, 3],)             # both slots differ from their primes in size class: slot 0 -> the small prime, slot 1 -> the 49-bit one

# (m, FHESI_PHI_CONV, items, sets).  A case may take what test_rows_fwd_inv_vs_oracle[18] (test_gpu_ntt.py) takes, 0.20 s where this was written;
# one that took longer with the whole matrix lost index sets, the most redundant first: [1] (item 3 runs the singleton map of the small prime
# anyway), then [2, 3, 4] and [0, 2, 4].  Measured with all the sets: m = 2^14 0.24 s, 2^15 0.43 s, 2^16 ... 2^19 and the Bluestein rings from
# m = 8422 0.66 ... 3.7 s, most of it the oracle's scaleDownToSet and its Bluestein rows over the five primes of the control.  As cut: 2^14
# 0.20 s, 2^15 0.19 s; 2^16 0.39, 2^17 0.80, 2^18 1.63, 2^19 1.13, 8422 2.48, 16411 0.81, 17325 1.57, 32771 1.93 s with the one set and the
# control, where no set is left to drop.
RINGS = [pytest.param(m, 0, ALL_ITEMS, X.SETS, id=f"m{m}") for m in (16, 1 << 11, 1 << 12, 1 << 13)]
RINGS += [pytest.param(1 << 14, 0, ALL_ITEMS, X.SETS[1:], id=f"m{1 << 14}"), pytest.param(1 << 15, 0, ALL_ITEMS, ONE_SET, id=f"m{1 << 15}")]
RINGS += [pytest.param(m, 0, LARGE_ITEMS, ONE_SET, id=f"m{m}") for m in (1 << 16, 1 << 17, 1 << 18)]
RINGS += [pytest.param(1 << 19, 0, (1, 2, 3), ONE_SET, id=f"m{1 << 19}")]
RINGS += [pytest.param(45, 0, ALL_ITEMS, X.SETS, id="m45"), pytest.param(45, 1, ALL_ITEMS, X.SETS, id="m45-phi-conv")]
RINGS += [pytest.param(m, 0, ALL_ITEMS, X.SETS, id=f"m{m}") for m in (101, 46, 27)]
RINGS += [pytest.param(m, 0, LARGE_ITEMS, ONE_SET, id=f"m{m}") for m in (8422, 16411, 17325, 32771)]


def tile_names(m):
    """the instantiations a power-of-two ring's rows must record, or None where the launchers record none (kernels_ntt.hip)"""
    logn = m.bit_length() - 2
    if m & (m - 1) or not 11 <= logn <= 17:
        return None
    if logn <= 14:
        return f"ntt_fwd_tile<{logn}, false, 0, false>", f"ntt_inv_tile<{logn}, 0, false>"
    return f"ntt_fwd_tile<14, false, {logn - 14}, false>", f"ntt_inv_tile<14, {logn - 14}, false>"


def check_set(ctx, orc, S, items, seed):
    """every item of `items` for the index set S; -> what the device gave, in order (compared between two contexts by the FHESI_PHI_CONV case)"""
    m, n, primes = ctx.m, ctx.phim, ctx.primes
    comp = [i for i in X.FULL if i not in S]
    PS = X.product(primes, S)
    W = len(S) + 2
    rng = np.random.default_rng(seed)
    poly = X.centred_poly(n, PS, seed)
    limbs = X.to_limbs(poly, W)
    full = orc.dcrt_from_poly(limbs)
    got = []

    def same(a, b, *what):
        assert np.array_equal(a, b), (m, S) + what
        got.append(np.array(a, copy=True))

    # 1: launch_rns_reduce over the set + the forward rows
    d = F.DoubleCRT.from_poly(ctx, limbs, index_set=S)
    assert d.index_set() == S
    same(d.rows(), full[S], "from_poly")
    same(F.DoubleCRT.from_poly(ctx, limbs[:5], index_set=S).rows(), orc.dcrt_from_poly(limbs[:5])[S], "from_poly, 5 coefficients")
    if n <= 1 << 11:
        for nc in (n + 3, m + 2):            # degree >= phi(m): folded modulo Phi_m on the host, one fhesi_cmod_fft per row; >= m: ignored
            over = np.concatenate([limbs, P.rand_limbs(rng, (nc - n,), W, PS.bit_length() - 1)])
            rows = F.DoubleCRT.from_poly(ctx, over, index_set=S).rows()
            for s, i in enumerate(S):
                same(rows[s], orc.cmod_fft(i, over), "from_poly", nc, i)
    # 2: the inverse rows + launch_crt over the set
    same(d.to_poly(W), orc.dcrt_to_poly(full, W, idx=S), "to_poly")
    assert X.to_ints(got[-1]) == poly, (m, S, "to_poly: not the input integers")
    same(d.to_poly(W, positive=True), orc.dcrt_to_poly(full, W, idx=S, positive=True), "to_poly positive")
    T = S[:1] + comp[:1]
    same(d.to_poly(W, index_set=T), orc.dcrt_to_poly(full, W, idx=S[:1]), "to_poly", T)
    # 3: Cmodulus::FFT / iFFT of one prime
    ev = P.rand_rows(rng, primes, n)[0]
    for i in S:
        same(ctx.cmod_fft(i, limbs), orc.cmod_fft(i, limbs), "cmod_fft", i)
        same(ctx.cmod_ifft(i, ev[i]), orc.cmod_ifft(i, ev[i]), "cmod_ifft", i)
    if 1 in S:
        top = np.full(n, primes[1] - 1, dtype=np.uint64)
        same(ctx.cmod_ifft(1, top), orc.cmod_ifft(1, top), "cmod_ifft of q - 1")
    if 4 in items:
        coeff = d.to_scrt()
        for s, i in enumerate(S):
            same(coeff[s], orc.cmod_ifft(i, full[i]), "to_scrt", i)
        h = F.DoubleCRT(ctx, S)
        h.from_scrt(coeff)
        assert h.equals(d), (m, S, "from_scrt")
        part = F.SingleCRT(ctx).assign_dcrt(d, S[-1:])
        assert part.index_set() == S[-1:]
        same(part.rows()[0], coeff[-1], "SingleCRT.assign_dcrt")
    if 5 in items and comp:
        e = d.copy()
        e.add_primes(comp)
        assert e.index_set() == X.FULL
        same(e.rows(), full, "add_primes")
        e.remove_primes(comp)
        assert e.index_set() == S
        same(e.rows(), full[S], "remove_primes")
    if 6 in items:
        for keep in [S[1:], S[-1:]][:len(S) - 1]:                 # (one prime: nothing to drop; two: both are the same set)
            e = F.DoubleCRT.from_poly(ctx, limbs, index_set=S)
            e.scale_down_to_set(keep, P_MOD)
            assert e.index_set() == keep
            same(e.rows(), orc.dcrt_scale_down_to_set(full, S, keep, P_MOD)[keep], "scale_down_to_set", keep)
        if comp:
            e = F.DoubleCRT.from_poly(ctx, limbs, index_set=S)
            lf = e.add_primes_and_scale(comp, P_MOD)
            want, wlf = orc.dcrt_add_primes_and_scale(full, S, comp, P_MOD)
            assert e.index_set() == X.FULL
            same(e.rows(), want, "add_primes_and_scale")
            assert abs(lf - wlf) < 1e-9 * max(1.0, abs(wlf)), (m, S, lf, wlf)
    if 7 in items:
        k = next(k for k in range(2, m) if ctx.zms_idx()[k] >= 0)
        whole = F.DoubleCRT.from_poly(ctx, limbs)
        same(d.automorph(k).rows(), orc.dcrt_automorph(full, k)[S], "automorph", k)
        same(whole.rows(), full, "the full-chain operand after automorph")
    return got


def run_ring(m, items, sets):
    primes, roots, _ = X.mixed_chain(m)
    ctx = F.Context(m, primes, roots)
    orc = O.Oracle(m, primes, roots)
    if m > 2000 and m & (m - 1):
        orc.set_bluestein_fft(True)
    got = []
    for S in list(sets) + [X.FULL]:                 # the control last: a failure before it is on the mapped side
        got += check_set(ctx, orc, list(S), items, 100 * m + sum(1 << i for i in S))
    names = tile_names(m)
    if names:                                       # the class this case is there for, as the library recorded it, under a map
        limbs = X.to_limbs(X.centred_poly(ctx.phim, primes[1] * primes[3], m), 4)
        ctx.prof_enable(True)
        F.DoubleCRT.from_poly(ctx, limbs, index_set=[1, 3]).to_scrt()
        rec = ctx.prof_kernel_name("ntt_fwd"), ctx.prof_kernel_name("ntt_inv")
        ctx.prof_enable(False)
        assert rec == names, rec
    return got


@pytest.mark.parametrize("m,phi_conv,items,sets", RINGS)
def test_index_sets_vs_oracle(m, phi_conv, items, sets, monkeypatch):
    if not phi_conv:
        run_ring(m, items, sets)
        return
    monkeypatch.setenv("FHESI_PHI_CONV", "1")       # read when the context is created
    conv = run_ring(m, items, sets)
    monkeypatch.delenv("FHESI_PHI_CONV")
    lds = run_ring(m, items, sets)                  # ... and the long division in LDS gives the same bits
    assert len(conv) == len(lds) and all(np.array_equal(a, b) for a, b in zip(conv, lds))
