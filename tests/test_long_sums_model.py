"""CPU: the inputs of tests/test_gpu_long_sums.py do what that test assumes, before any GPU time is spent.
(a) the crafted constants give rows of q - 1 under the reference's DoubleCRT(poly * p) (oracle/fhesi_pyref.py), modulo the first two chain primes
    on the 64-bit path and modulo the first two primes of the tensor half on the 30-bit path;
(b) every chain the GPU test builds satisfies the tensor half's plan condition chain >= TB + 1.5 (kernels_tensor32.hip, t32_plan_search) at its
    longest group, and the xi = 1 chain fails it at 40 terms;
(c) the group lengths straddle the fold period the library compiles and the four-term rounds of tensor_sum32_kernel."""
import os
import re

import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import long_sums_common as C
import params as P


def test_group_lengths_straddle_the_fold_period_and_the_rounds():
    Fp = C.fold_period()
    src = open(os.path.join(C.ROOT, "fhe-si_amd", "csrc", "kernels_ew.hip")).read()
    assert re.search(r"folded every (\d+) terms", src).group(1) == str(Fp)          # the comment at the kernel says the same
    ln = C.group_lengths(Fp)
    assert {Fp - 1, Fp, Fp + 1, 2 * Fp, 2 * Fp + 1, 3 * Fp + 1} <= set(ln)
    assert {x % 4 for x in ln} == {0, 1, 2, 3} and 1 in ln and 4 in ln              # no round, whole rounds, every tail
    assert Fp != 32 or ln == [1, 4, 5, 6, 8, 31, 32, 33, 64, 65, 97]                # the cases as listed, at today's period
    # the lone long group: its accumulating passes fold on the 64-bit path and run whole rounds on the 30-bit path
    step = C.LONG_OPERANDS // 2
    assert 2 * C.LONG_DISTINCT > C.LONG_OPERANDS and step > Fp and step % 4 == 0 and C.LONG_TERMS % step and C.LONG_TERMS > 2 * step
    g = C.long_group()
    assert len({x for x, _ in g}) == len({y for _, y in g}) == C.LONG_DISTINCT


@pytest.mark.parametrize("ring,xi", [(C.M1024, 97), (C.M46, 1)])
def test_crafted_constants_give_rows_of_q_minus_1_on_the_chain(ring, xi):
    m, logQ, p = ring
    primes, roots = P.chain_for(m, logQ, p, xi)
    c, d = C.crafted_constants(p, primes[0], primes[1])
    assert 0 < c < 1 << 120 and 0 < d < 1 << 120                                    # both fit the centred range of logQ = 128
    ctx = R.Ctx(m, logQ, p, primes, roots)
    left = R.dcrt_from_poly(ctx, [c * p], [0, 1])                                   # DoubleCRT(poly * p), Ciphertext.cpp:169-176
    right = R.dcrt_from_poly(ctx, [d], [0, 1])
    minus = R.dcrt_from_poly(ctx, [-1])
    for i in (0, 1):
        assert left[i] == [primes[i] - 1] * ctx.phim and right[i] == [primes[i] - 1] * ctx.phim
    assert all(minus[i] == [q - 1] * ctx.phim for i, q in enumerate(primes))
    # ... so a product of such a pair is (q - 1)^2 = 1, and the middle part of a term 2 (q - 1)^2 = 2
    t = R.ct_mul(ctx, [[c], [c]], [[d], [-1]])
    assert [t[k][0][0] for k in range(3)] == [1, 2, 1]


def test_crafted_constants_give_rows_of_q_minus_1_on_the_tensor_half():
    m, logQ, p = C.M46
    off, stride, lg = F.lin_class(m)
    assert (off, stride, lg) == (23, 1, 14)                                         # padded rows of 2^14: negacyclic transforms modulo primes 1 mod 2^15
    t0, t1 = C.tensor_primes(lg, 2)
    assert t0 <= (1 << 30) - (1 << 15) + 1                                          # (t32_plan_search takes no candidate above that)
    assert t0 % (1 << 15) == 1 and t1 % (1 << 15) == 1 and t1 < t0 < 1 << 30 and t1 > 1 << 29
    c, d = C.crafted_constants(p, t0, t1)
    assert 0 < c < 1 << 60
    n = 1 << lg
    for q in (t0, t1):
        psi = next(x for x in (pow(g, (q - 1) // (2 * n), q) for g in range(2, 100)) if pow(x, n, q) == q - 1)
        assert R._ntt_pow2([c * p], n, q, psi) == [q - 1] * n and R._ntt_pow2([d], n, q, psi) == [q - 1] * n


def test_chains_meet_the_plan_condition_or_miss_it_where_intended():
    Fp = C.fold_period()
    m, logQ, p = C.M46
    _, phim = R.zms_idx(m)
    longest = C.longest_group(Fp)
    for xi, gmax in ((longest, longest), (C.LONG_TERMS, C.LONG_TERMS)):
        primes, _ = P.chain_for(m, logQ, p, xi)
        assert C.plan_applies(primes, logQ, p, phim, gmax, True), (xi, C.chain_bits(primes), C.t32_TB(logQ, p, phim, gmax, True))
    primes, _ = P.chain_for(m, logQ, p, 1)
    assert not C.plan_applies(primes, logQ, p, phim, 40, True)                      # the chain of single products is too short for 40 terms
    assert C.plan_applies(primes, logQ, p, phim, 1, True)                           # ... though not for one
    # TB as the source states it
    src = open(os.path.join(C.ROOT, "fhe-si_amd", "csrc", "kernels_tensor32.hip")).read()
    assert "const double TB = 2.0 * (logQ - 1) + pbits + cbits + 1 + gbits + (lin ? 2 : 0);" in src and "if (chain < TB + 1.5) return pl;" in src
    assert C.t32_TB(128, 47, 22, 97, True) == 254 + 6 + 5 + 1 + 7 + 2
    assert C.t32_TB(128, 47, 22, longest, True) == 254 + 6 + 5 + 1 + 8 + 2      # a group size the plan has to add bits for


def test_the_crafted_group_wraps_128_bits_unless_the_kernel_folds():
    """tensor_sum_kernel's middle accumulator on the longest group (rows of q - 1 modulo the first chain prime): two products per term; the sum
    passes 2^128 without the fold, and never with it -- so the group tells a kernel that folds from one that does not"""
    Fp = C.fold_period()
    m, logQ, p = C.M1024
    primes, _ = P.chain_for(m, logQ, p, C.longest_group(Fp))
    q, T, M = primes[0], C.crafted_terms(Fp), 1 << 128
    assert q.bit_length() == 60
    assert 2 * T * (q - 1) ** 2 >= M > 2 * max(C.group_lengths(Fp)) * (q - 1) ** 2      # the lengths around the period alone would not wrap
    acc, wrapped, plain = 0, False, 0
    for t in range(T):
        acc += 2 * (q - 1) ** 2
        plain += 2 * (q - 1) ** 2
        wrapped |= acc >= M
        if t % Fp == Fp - 1:
            acc %= q
    assert not wrapped and acc % q == 2 * T % q
    assert (plain % M) % q != 2 * T % q                                             # what a kernel without the fold would store
