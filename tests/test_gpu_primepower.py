"""GPU: the prime-power rings m = q^k and 2 q^k (q an odd prime, k >= 2) on the fused 30-bit paths -- the strided fold of the linear-convolution
rows (tests/test_primepower_fold_model.py holds the identities) in the key switch's recombination, in the tensor half's CRT and in the coefficient
gather of Ciphertext >>=.  Every comparison is bit-exact: against the C oracle on the rings it can afford, against the per-prime device path
(option ks_direct = 1, tensor32 = 0: what test_gpu_general_m.py pins to the oracle) on the large ones."""
import math

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import ks_crafted as K
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu


def stride(m):
    off, st, lg = F.lin_class(m)
    return st


def setup(m, logQ, p, seed, count):
    primes, roots = P.chain_for(m, logQ, p, 1, 60)
    ctx = F.Context(m, primes, roots)
    orc = O.Oracle(m, primes, roots)
    if m > 2000:
        orc.set_bluestein_fft(True)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    rng = np.random.default_rng(seed)
    ksm = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)])
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    a[0, 0, 0] = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0]          # the extremes of the centred range
    b[0, 1, 0] = O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    return ctx, orc, ksm, a, b, nd, nl


def generated_matrix(orc, rng, primes, n, nd, logQ):
    """a matrix shaped like KeySwitchSI::Init's: integer coefficients in [-2^(logQ-1), 2^(logQ-1)), the extremes included"""
    W, half = len(primes) + 2, 1 << (logQ - 1)
    ksm = np.empty((2, 3 * nd, len(primes), n), dtype=np.uint64)
    for r in range(2):
        for c in range(3 * nd):
            ksm[r, c] = orc.dcrt_from_poly(P.rand_limbs(rng, (n,), W, logQ))
    ksm[0, 0] = orc.dcrt_from_poly(O.ints_to_limbs([-half if i % 3 else half - 1 for i in range(n)], W))
    return ksm


def per_prime(ctx, ksm, nd, logQ, p, a, b):
    """the same multiplication on per-prime rows: the parent's only path on these rings"""
    ctx.set_option("ks_direct", 1)
    ctx.set_option("tensor32", 0)
    k = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    got = ctx.ct_mul_relin(k, logQ, p, a, b)
    ctx.set_option("ks_direct", 0)
    ctx.set_option("tensor32", 1)
    assert k.form()[0] == 0, k.form()
    return got


@pytest.mark.parametrize("m,logQ", [(9, 200), (18, 128), (25, 300), (27, 200), (49, 256), (50, 300), (54, 200), (162, 341), (250, 200),
                                    (1458, 341), (2187, 200), (4374, 128)])
def test_mul_relin_on_small_prime_power_rings(m, logQ):
    p = 23 if m != 50 else 101
    ctx, orc, ksm, a, b, nd, nl = setup(m, logQ, p, 11 + m, 2)
    assert ctx.lin_class()[:2] == F.lin_class(m)[:2] and ctx.lin_class()[1] > 1
    rng = np.random.default_rng(m)
    for kind, mat in (("uniform", ksm), ("generated", generated_matrix(orc, rng, ctx.primes, ctx.phim, nd, logQ))):
        ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(mat)
        ctx.prof_enable(True)
        got = ctx.ct_mul_relin(ksk, logQ, p, a, b)
        name = ctx.prof_kernel_name("rns_reduce")
        ctx.prof_enable(False)
        assert ksk.form()[0] == 1, (kind, ksk.form())                   # limbs over the four 30-bit auxiliary primes: the linear-convolution form ran
        assert "rns32_reduce_kernel" in name, name                      # ... and the tensor half over the 30-bit primes
        if kind == "generated":
            assert ksk.key_bits()[0], ksk.key_bits()
        for c in range(2):
            assert np.array_equal(got[c], orc.ct_mul_relin(mat, a[c], b[c], logQ, p)), (kind, c)
        assert np.array_equal(per_prime(ctx, mat, nd, logQ, p, a, b), got), kind


@pytest.mark.parametrize("m,logQ", [(27, 200), (54, 200), (1458, 341)])
def test_key_switch_on_crafted_rows(m, logQ):
    """scaled-down parts = (d X^pos, 0, 0), key row (r, 0) = edge polynomial e: the dot product is d X^pos e mod Phi_m, with the unit digit where
    every residue class j mod s and both parities of floor(j / s) reach the fold"""
    ctx, orc, ksm, a, b, nd, nl = setup(m, logQ, 23, 5 + m, 1)
    n, L, s = ctx.phim, ctx.L, stride(m)
    Pprod = 1
    for q in ctx.primes:
        Pprod *= int(q)
    mod, W, h, pb = 1 << logQ, L + 2, (Pprod - 1) // 2, Pprod.bit_length()
    edge = K.edge_values(Pprod)
    assert edge[:4] == [h, -h, h + 1, h - 1] and edge[-1] == (1 << (pb - 8)) + 17
    for i, pos in enumerate((0, s - 1, s, n - s, n - 1, n // 2)):
        d = 1 if i == 0 else (1 << 24) - 1
        tp = np.zeros((1, 3, L, n), dtype=np.uint64)
        tp[0, 0] = orc.dcrt_from_poly(K.monomial_limbs(n, W, pos, d * mod))
        ksm2 = ksm.copy()
        for r in range(2):
            ksm2[r, 0] = orc.dcrt_from_poly(K.edge_limbs(edge, n, W, r))
        ksk2 = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm2)
        out = ctx.alloc(2 * n * nl * 8)
        ctx.apply_key_switch_dev(ksk2, logQ, ctx.upload(tp), 1, out, nl)
        assert ksk2.form()[0] == 1
        assert np.array_equal(out.download((2, n, nl)), orc.apply_key_switch(ksm2, tp[0], logQ, nl)), (d, pos)


@pytest.mark.parametrize("m,logQ,oracle", [(15625, 128, True), (16807, 128, True), (39366, 200, False), (59049, 128, False)])
def test_mul_relin_on_long_rows(m, logQ, oracle):
    """rows of 2^15 left as their two sub-inverses (the fold and the tail stage in the loaders: m = 15625, 16807, 39366) and rows of 2^17 (the tail
    pass, then the fold from whole rows: m = 59049), with a uniform and with a generated matrix"""
    p = 23
    ctx, orc, ksm, a, b, nd, nl = setup(m, logQ, p, 3 + m, 1)
    assert ctx.lin_class() == F.lin_class(m) and ctx.lin_class()[2] == (17 if m == 59049 else 15)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    got = ctx.ct_mul_relin(ksk, logQ, p, a, b)
    assert ksk.form()[0] == 1, ksk.form()
    if oracle:
        assert np.array_equal(got[0], orc.ct_mul_relin(ksm, a[0], b[0], logQ, p))
    assert np.array_equal(per_prime(ctx, ksm, nd, logQ, p, a, b), got)
    n = ctx.phim
    one = np.zeros((n, 1), dtype=np.uint64)
    one[0, 0] = 1
    t = F.DoubleCRT(ctx).sample(0, 64, 77, 1)
    t2 = t.copy()
    t2.op(t, 2)
    kg = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([F.DoubleCRT.from_poly(ctx, one), t, t2], t, logQ, 77, 78, 100, 3)
    got_g = ctx.ct_mul_relin(kg, logQ, p, a, b)
    assert kg.form()[0] == 1 and kg.key_bits()[0], (kg.form(), kg.key_bits())
    assert np.array_equal(per_prime(ctx, kg.download(), nd, logQ, p, a, b), got_g)


@pytest.mark.parametrize("m,logQ", [(50, 200), (1458, 200)])
def test_sums_of_products(m, logQ):
    p = 101 if m == 50 else 23
    ctx, orc, ksm, a, b, nd, nl = setup(m, logQ, p, 17 + m, 11)
    n = ctx.phim
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    pool = np.concatenate([a, b])
    seg = np.array([0, 1, 4, 11])                                        # groups of 1, 3 and 7 terms
    out = ctx.alloc(3 * 2 * n * nl * 8)
    ctx.ct_mul_sum_relin_dev(ksk, logQ, p, ctx.upload(pool), nl, list(range(11)), list(range(11, 22)), seg, out)
    assert ksk.form()[0] == 1
    got = out.download((3, 2, n, nl))
    for g in range(3):
        tp = None                                                        # composed the way Matrix.cpp does: *= per product, += scaled up, ApplyKeySwitch
        for i in range(seg[g], seg[g + 1]):
            t = orc.ct_mul(a[i], b[i], p)
            if tp is None:
                tp = t
            else:
                for comp in range(3):
                    for r, q in enumerate(ctx.primes):
                        tp[comp][r] = (tp[comp][r] + t[comp][r]) % np.uint64(q)
        assert np.array_equal(got[g], orc.apply_key_switch(ksm, tp, logQ, nl)), g


@pytest.mark.parametrize("m,logQ", [(9, 90), (25, 90), (27, 90), (50, 90), (54, 90), (1458, 128)])
def test_automorphism_is_a_gather(m, logQ):
    p = 23
    ctx, orc, _, a, b, nd, nl = setup(m, logQ, p, 29 + m, 2)
    n, count = ctx.phim, 2
    rng = np.random.default_rng(m)
    ksm = np.stack([P.rand_rows(rng, ctx.primes, n, 2 * nd) for _ in range(2)])
    ksk = F.KeySwitchMatrix(ctx, 2, nd).upload(ksm)
    units = [k for k in range(2, m) if math.gcd(k, m) == 1]
    gen = next(g for g in units if len({pow(g, e, m) for e in range(len(units) + 1)}) == len(units) + 1)
    da = ctx.upload(a)
    for k in (units if m <= 54 else [gen, m - 1]):
        rot = ctx.alloc(count * 2 * n * (nl + 1) * 8)
        ctx.prof_enable(True)
        ctx.ct_automorph_dev(k, da, 2, nl, count, rot, nl + 1)
        launches = ctx.prof_read("ntt_fwd")[0] + ctx.prof_read("ntt_inv")[0]
        ctx.prof_enable(False)
        assert launches == 0, (k, launches)                              # the coefficient gather: no row transform
        got = rot.download((count, 2, n, nl + 1))
        exp = [orc.ct_automorph(a[c], k, nl + 1) for c in range(count)]
        for c in range(count):
            assert np.array_equal(got[c], exp[c]), (k, c)
        out = ctx.alloc(count * 2 * n * nl * 8)
        ctx.prof_enable(True)
        before = ctx.prof_read("ntt_fwd")[0] + ctx.prof_read("ntt_inv")[0]
        ctx.ct_automorph_key_switch_dev(ksk, logQ, k, da, nl, count, out, nl)
        gathered = ctx.prof_read("ntt_fwd")[0] + ctx.prof_read("ntt_inv")[0] - before
        ctx.prof_enable(False)
        sw = out.download((count, 2, n, nl))
        for c in range(count):
            assert np.array_equal(sw[c], orc.apply_key_switch_parts(ksm, exp[c], logQ, nl)), (k, c)
        ctx.set_option("automorph_rows", 1)
        ctx.ct_automorph_dev(k, da, 2, nl, count, rot, nl + 1)
        assert np.array_equal(rot.download((count, 2, n, nl + 1)), got), k
        ctx.prof_enable(True)
        before = ctx.prof_read("ntt_fwd")[0] + ctx.prof_read("ntt_inv")[0]
        ctx.ct_automorph_key_switch_dev(ksk, logQ, k, da, nl, count, out, nl)
        by_rows = ctx.prof_read("ntt_fwd")[0] + ctx.prof_read("ntt_inv")[0] - before
        ctx.prof_enable(False)
        assert np.array_equal(out.download((count, 2, n, nl)), sw), k
        assert gathered < by_rows, (k, gathered, by_rows)                # the rotation inside the key switch is the gather too: only the key switch's own transforms
        ctx.set_option("automorph_rows", 0)


def test_other_classes_are_unchanged():
    for m, want in ((22, (11, 1, 14)), (101, (101, 1, 14))):
        primes, roots = P.chain_for(m, 128, 23, 1, 60)
        assert F.Context(m, primes, roots).lin_class() == want
    ctx, orc, ksm, a, b, nd, nl = setup(45, 200, 23, 45, 1)
    assert ctx.lin_class() == (0, 0, 0)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    got = ctx.ct_mul_relin(ksk, 200, 23, a, b)
    assert np.array_equal(got[0], orc.ct_mul_relin(ksm, a[0], b[0], 200, 23))


def device_keys(ctx, logQ, seed):
    """FHESISecKey::Init + FHESIPubKey::Init (FHE-SI.cpp:86-91, :42-63) from device samples: t = sampleHWt, pk = (e + t c1, -c1) reduced modulo
    2^logQ with c1 uniform below 2^logQ; KeySwitchSI(secretKey) and KeySwitchSI(secretKey, k) are generated on the device by the caller"""
    n, nl, W = ctx.phim, (logQ + 63) // 64, ctx.L + 2
    t = F.DoubleCRT(ctx).sample(0, min(64, n // 2), seed, 1)
    c1 = P.rand_limbs(np.random.default_rng(seed), (n,), nl, logQ)
    x = F.DoubleCRT.from_poly(ctx, c1).op(t, 2).op(F.DoubleCRT(ctx).sample(1, 0, seed, 2), 0)
    pk0 = F.DoubleCRT.from_poly(ctx, O.reduce_coeffs(x.to_poly(W), logQ)[:, :nl].copy())
    minus = O.ints_to_limbs([-v for v in O.limbs_to_ints(c1)], nl + 1)
    pk1 = F.DoubleCRT.from_poly(ctx, O.reduce_coeffs(minus, logQ)[:, :nl].copy())
    return t, pk0, pk1


@pytest.mark.parametrize("m,p,logQ,t_rot", [(50, 101, 200, 3), (1458, 1459, 256, 5), (39366, 39367, 320, 7)])
def test_slots_multiply_and_rotate_on_the_fused_path(m, p, logQ, t_rot):
    """Plaintext slots end to end on the rings the slot layer packs cheaply: encrypt two slot vectors, multiply with relinearisation on the fused
    path, rotate by g^t with the automorphism key switch, decrypt to slots -- the slot-wise product rotated left by t, modulo p.
    logQ: one multiplication and one rotation.  The scheme is scale-invariant (the message sits at Q / p), the noise after the two steps is below
    p^2 n^2 2^8 (tensor product of two fresh ciphertexts) + 2 nd n 2^24 2^6 (two key switches with 24-bit digits and Gaussian errors) -- 2^64 at
    m = 39366 -- and has to stay below Q / 2p: logQ = 200, 256, 320 leave more than 100 bits.  The reference's decrypt predicate
    (Test_AddMul.cpp:84-86) holds on the CPU model (oracle/fhesi_pyref.py: keygen, encrypt, ct_mul_relin, ct_automorph + apply_key_switch_parts,
    decrypt) at these (m, p, logQ) for m = 50 and m = 1458."""
    import slots_model as M
    g = 3 if m == 50 else M.least_generator(m)
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    assert ctx.lin_class()[1] > 1
    S = F.SlotSpace(ctx, p, g)
    n, nl, nd = S.total, (logQ + 63) // 64, R.ndigits(logQ)
    assert n == ctx.phim                                                  # p = 1 mod m: every slot lies in Z_p
    t, pk0, pk1 = device_keys(ctx, logQ, 900 + m)
    one = np.zeros((n, 1), dtype=np.uint64)
    one[0, 0] = 1
    one = F.DoubleCRT.from_poly(ctx, one)
    t2 = t.copy().op(t, 2)
    k = pow(g, t_rot, m)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([one, t, t2], t, logQ, 900 + m, 901 + m, 100, 3)
    ksk_k = F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, t.copy().automorph(k)], t, logQ, 900 + m, 901 + m, 100 + 3 * nd, 3)
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(1, n)).astype(np.int64)
    b = rng.integers(0, p, size=(1, n)).astype(np.int64)
    ca, cb, prod, rot = (ctx.alloc(2 * n * nl * 8) for _ in range(4))
    S.encrypt_batch_seeded(pk0, pk1, logQ, 77, 0, a, ca, nl, False)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 77, 1, b, cb, nl, False)
    assert np.array_equal(S.decrypt_batch(t, logQ, ca, nl, 1, n, False), a)
    ctx.ct_mul_relin_dev(ksk, logQ, p, ca, cb, prod, nl, 1)
    assert ksk.form()[0] == 1 and ksk.key_bits()[0], (ksk.form(), ksk.key_bits())
    want = a * b % p
    assert np.array_equal(S.decrypt_batch(t, logQ, prod, nl, 1, n, False), want)
    ctx.ct_automorph_key_switch_dev(ksk_k, logQ, k, prod, nl, 1, rot, nl)
    assert ksk_k.form()[0] == 1, ksk_k.form()
    assert np.array_equal(S.decrypt_batch(t, logQ, rot, nl, 1, n, False), np.roll(want, -t_rot, axis=1))
