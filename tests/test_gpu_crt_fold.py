"""The tensor half on rows of 2^14 with the CRT constant inside the inverse transform's closing multiplication (kernels_tensor32.hip: the rows
reach crt32_scale_kernel / crt32_scale_generic_kernel as y_i = x (M / p_i)^-1 mod p_i) and the fast pass formed from bit logQ - 64 upwards
(undecided when bits logQ-28 .. logQ-1 of the rounding limb are all ones).  Every output is exact arithmetic followed by an exact integer CRT: all
comparisons are bit for bit against the C oracle.

The fused 30-bit path needs rows of 2^14: m = 2^15, logQ = 512, p = 23, three decomposition bytes.  One batch of 25 ciphertext pairs and its oracle
results are built once and shared: 25 pairs take the grouped block order of the tensor inverse (groups of 8 ciphertexts x 3 rows, the last group
ragged), 1 and 3 the plain one; pair 1 holds -2^511 and pair 2 holds 2^511 - 1 in every coefficient.  The crafted rounding coefficients and what the
window does with them are checked without a GPU in tests/test_crt32_fold_model.py; the test below it checks the same bit patterns on the oracle's
own integers."""
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
import test_crt32_fold_model as W

M, LOGQ, PT = 1 << 15, 512, 23
COUNT = 25
ORACLE_CHECKED = (0, 1, 2, 7, 8, 23, 24)        # first, the two edge pairs, both sides of the first group of 8, the last group's (ragged: 25 = 3 x 8 + 1) neighbours


@functools.lru_cache(maxsize=None)
def ring():
    primes, roots = P.chain_for(M, LOGQ, PT)
    orc = O.Oracle(M, primes, roots)
    n, nd, nl = M // 2, R.ndigits(LOGQ), LOGQ // 64
    rng = np.random.default_rng(512)
    ksm = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)])
    a = P.rand_limbs(rng, (COUNT, 2, n), nl, LOGQ)
    b = P.rand_limbs(rng, (COUNT, 2, n), nl, LOGQ)
    lo, hi = O.ints_to_limbs([-(1 << (LOGQ - 1))], nl)[0], O.ints_to_limbs([(1 << (LOGQ - 1)) - 1], nl)[0]
    a[1], b[1] = lo, lo
    a[2], b[2] = hi, hi
    for x in (a, b, ksm):
        x.setflags(write=False)
    return primes, roots, orc, ksm, a, b, n, nd, nl


@functools.lru_cache(maxsize=None)
def want(c):
    _, _, orc, ksm, a, b, *_ = ring()
    r = orc.ct_mul_relin(ksm, a[c], b[c], LOGQ, PT)
    r.setflags(write=False)
    return r


def device():
    primes, roots, _, ksm, _, _, _, nd, _ = ring()
    ctx = F.Context(M, primes, roots)
    return ctx, F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)


def mul_relin_dev(ctx, ksk, count):
    _, _, _, _, a, b, n, _, nl = ring()
    da, db, dout = ctx.upload(a[:count]), ctx.upload(b[:count]), ctx.alloc(a[:count].nbytes)
    ctx.prof_enable(True)
    ctx.ct_mul_relin_dev(ksk, LOGQ, PT, da, db, dout, nl, count)
    ctx.sync()
    crt = ctx.prof_kernel_name("crt")
    ctx.prof_enable(False)
    return dout.download((count, 2, n, nl)), crt


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3, COUNT])
def test_ct_mul_relin_dev_against_the_oracle(count):
    ctx, ksk = device()
    got, crt = mul_relin_dev(ctx, ksk, count)
    assert crt == "crt32_scale_kernel<512, false, 28, 38, 0>", crt
    for c in [c for c in ORACLE_CHECKED if c < count]:
        assert np.array_equal(got[c], want(c)), c
    if count == COUNT:                               # every pair of the grouped launch: the same bits as in the plain block order of a launch of three
        for c0 in range(0, COUNT, 3):
            cnt = min(3, COUNT - c0)
            _, _, _, _, a, b, n, _, nl = ring()
            assert np.array_equal(ctx.ct_mul_relin(ksk, LOGQ, PT, a[c0:c0 + cnt], b[c0:c0 + cnt]), got[c0:c0 + cnt]), c0


@pytest.mark.gpu
@pytest.mark.parametrize("option,value", [("tensor_bits", 29), ("tensor32", 0)])
def test_other_primes_and_the_chain_path(option, value):
    """primes below 2^29 follow (other primes, one more of them, the same closing stage); the chain path (tensor32 = 0) is untouched"""
    ctx, ksk = device()
    ctx.set_option(option, value)
    got, crt = mul_relin_dev(ctx, ksk, 3)
    assert ("crt32_scale" in crt) == (option == "tensor_bits"), crt
    for c in range(3):
        assert np.array_equal(got[c], want(c)), c


@pytest.mark.gpu
def test_sum_of_two_products_takes_the_plain_inverse():
    """fhesi_ct_mul_sum_relin_dev, one group of two products: tensor_sum32_kernel -> ntt32_inv_kernel3<false, false, T32Primes> -> crt32_scale_kernel
    (the stopwatch's last inverse is the key switch's, so the tensor half's is pinned by the sum kernel in front of it and the CRT kernel behind)"""
    primes, _, orc, ksm, a, b, n, _, nl = ring()
    ctx, ksk = device()
    pool = np.stack([a[0], a[3], b[0], b[3]])
    out = ctx.alloc(2 * n * nl * 8)
    ctx.prof_enable(True)
    ctx.ct_mul_sum_relin_dev(ksk, LOGQ, PT, ctx.upload(pool), nl, [0, 1], [2, 3], np.array([0, 2]), out)
    ctx.sync()
    assert ctx.prof_kernel_name("tensor") == "tensor_sum32_kernel" and ctx.prof_kernel_name("crt") == "crt32_scale_kernel<512, false, 28, 38, 0>"
    ctx.prof_enable(False)
    tp, t1 = orc.ct_mul(pool[0], pool[2], PT), orc.ct_mul(pool[1], pool[3], PT)
    for comp in range(3):
        for i, q in enumerate(primes):
            tp[comp][i] = (tp[comp][i] + t1[comp][i]) % np.uint64(q)
    assert np.array_equal(out.download((1, 2, n, nl))[0], orc.apply_key_switch(ksm, tp, LOGQ, nl))


@pytest.mark.gpu
@pytest.mark.parametrize("logQ,nwmax", [(341, 16), (512, 24)])
def test_linear_convolution_ring_folds_the_multiplied_rows(logQ, nwmax):
    """m = 1006 = 2 x 503 (the safe-prime ring of test_rounding_boundaries_take_the_exact_pass; the oracle needs no Bluestein mode there): zero-padded
    rows of 2^14, crt32_scale_generic_kernel at S = 0 with the fold r_j - r_(j+Q) - (-1)^j r_phi applied to rows that already carry the CRT constant.
    logQ = 341 (Test_Regression's): the window from bit logQ - 64 fits 16 words (24 before); logQ = 512: 21 words of the 24."""
    m, p, count = 1006, 23, 2
    primes, roots = P.chain_for(m, logQ, p)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    rng = np.random.default_rng(logQ)
    ksm = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)])
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    lo, hi = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0], O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    a[1, 0], b[1, 0], a[1, 1], b[1, 1] = lo, lo, hi, lo                      # the largest folded sums
    da, db, dout = ctx.upload(a), ctx.upload(b), ctx.alloc(a.nbytes)
    ctx.prof_enable(True)
    ctx.ct_mul_relin_dev(ksk, logQ, p, da, db, dout, nl, count)
    ctx.sync()
    assert ctx.prof_kernel_name("crt") == f"crt32_scale_generic_kernel<{nwmax}, false, 0, 1>", ctx.prof_kernel_name("crt")
    ctx.prof_enable(False)
    got = dout.download((count, 2, n, nl))
    for c in range(count):
        assert np.array_equal(got[c], orc.ct_mul_relin(ksm, a[c], b[c], logQ, p)), c


# ---------------------------------------------------------------------------------------------- the rounding window
def crafted_pair(deltas, seed):
    """a, b with b0 = 1: coefficient j of the tensor product's first component is x = p a0_j, and (x + 2^511) mod 2^512 = delta at the crafted
    positions (spread over many workgroups of the CRT kernel, 128 coefficients each)"""
    _, _, _, _, _, _, n, _, nl = ring()
    rng = np.random.default_rng(seed)
    a = np.zeros((2, n, nl), dtype=np.uint64)
    b = np.zeros((2, n, nl), dtype=np.uint64)
    a0 = [0] * n
    pos = [(k * 1021 + 5) % n for k in range(len(deltas))]
    for j, v in zip(pos, W.crafted(deltas, PT)):
        a0[j] = v
    a[0] = O.ints_to_limbs(a0, nl)
    a[1] = P.rand_limbs(rng, (n,), nl, LOGQ)
    b[0] = O.ints_to_limbs([1] + [0] * (n - 1), nl)
    b[1] = P.rand_limbs(rng, (n,), nl, LOGQ)
    return a, b, pos


def test_crafted_coefficients_have_their_bit_patterns_in_the_oracle():
    """no GPU: the oracle's own tensor product (Ciphertext::operator*=) of the crafted pairs, brought back to integers, holds the rounding limbs the
    window test needs -- bits 484..511 all ones with a zero in bits 448..483 (new window only), all 64 ones (the former case), and the values just
    above the boundary -- and its ScaleDown rounds them as round-half-up says"""
    primes, _, orc, *_ = ring()
    for deltas, seed in ((W.NEW_ONES + W.NEW_CROSS, 1), (W.OLD_DELTAS, 2)):
        a, b, pos = crafted_pair(deltas, seed)
        rows = orc.ct_mul(a, b, PT)[0]
        xs = O.limbs_to_ints(orc.dcrt_to_poly(rows, len(primes) + 1))
        down = O.limbs_to_ints(orc.scale_down(rows, LOGQ, LOGQ // 64 + 1))
        for j, d in zip(pos, deltas):
            x = xs[j]
            assert (x + (1 << 511)) % (1 << 512) == d % (1 << 512), (j, d)
            G = W.rounding_limb(x)
            if d in W.NEW_ONES:
                assert G >> 36 == (1 << 28) - 1 and G & ((1 << 36) - 1) != (1 << 36) - 1, hex(G)
            elif d in W.OLD_DELTAS:
                assert G == (W.M64 if d < 0 else 0), hex(G)
            else:
                assert G >> 36 == 0 and (1 << 429) < d < (1 << 484), hex(G)
            assert down[j] % (1 << 512) == W.expected(x, LOGQ), (j, d)


@pytest.mark.gpu
def test_rounding_window_from_bit_448():
    """Coefficients undecided only since the fast pass starts at bit 448, and the all-ones case of the former window: both as the oracle rounds
    them; with the exact pass switched off (crt_skip_cleanup) both sets come out wrong (tests/test_crt32_fold_model.py says which coefficients the
    formed value misrounds), so the inputs reach the pass."""
    _, _, orc, ksm, *_ = ring()
    ctx, ksk = device()
    pairs = [crafted_pair(W.NEW_ONES + W.NEW_CROSS, 1), crafted_pair(W.OLD_DELTAS, 2)]
    a, b = np.stack([pr[0] for pr in pairs]), np.stack([pr[1] for pr in pairs])
    exp = [orc.ct_mul_relin(ksm, a[c], b[c], LOGQ, PT) for c in range(2)]
    got = ctx.ct_mul_relin(ksk, LOGQ, PT, a, b)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    ctx.set_option("crt_skip_cleanup", 1)
    raw = ctx.ct_mul_relin(ksk, LOGQ, PT, a, b)
    ctx.set_option("crt_skip_cleanup", 0)
    assert not np.array_equal(raw[1], exp[1]), "the former all-ones case must need the exact pass"
    assert not np.array_equal(raw[0], exp[0]), "the values the window from bit 448 misrounds must need it too"
    assert np.array_equal(ctx.ct_mul_relin(ksk, LOGQ, PT, a, b), np.stack(exp))
