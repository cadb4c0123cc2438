"""GPU: fhesi_ct_mul_sum_relin_dev on groups past every fold and round boundary of its sum kernels -- the fold of tensor_sum_kernel's 128-bit
accumulators (kernels_ew.hip; the period is read from the source), the four-term rounds and the tail of tensor_sum32_kernel
(kernels_tensor32.hip), the tensor half's plan at group sizes of up to 2^7, and the piecewise sum of one long group whose accumulating passes
fold as well.  Operands at the top of the residue range included (tests/test_long_sums_model.py shows on the CPU that they are).
The oracle side is composed the way Matrix.cpp does: operator*= per product, += on the scaled-up ciphertexts, then ApplyKeySwitch.
Every comparison is bit-exact."""
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import long_sums_common as C
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu
SUM64, SUM32 = "tensor_sum_kernel", "tensor_sum32"


def pool_for(ring, primes, npool, path32):
    """npool random ciphertexts (the extremes of the centred range in entry 0), then the crafted left and right constants of the path's first
    two moduli: chain primes on the 64-bit path, the tensor half's primes on the 30-bit path"""
    m, logQ, p = ring
    _, n = R.zms_idx(m)
    nl = (logQ + 63) // 64
    rng = np.random.default_rng(1000 + m)
    pool = P.rand_limbs(rng, (npool + 2, 2, n), nl, logQ)
    lo, hi = -(1 << (logQ - 1)), (1 << (logQ - 1)) - 1
    pool[0, 0] = O.ints_to_limbs([lo if v else hi for v in rng.integers(0, 2, n)], nl)
    q0, q1 = C.tensor_primes(F.lin_class(m)[2], 2) if path32 else primes[:2]
    c, d = C.crafted_constants(p, q0, q1)
    pool[npool] = C.constant_ct(n, nl, c, c)
    pool[npool + 1] = C.constant_ct(n, nl, d, -1)
    return pool


def oracle_sums(orc, primes, ksm, pool, groups, logQ, p, nl):
    """KeySwitch(sum of the group's products) per group; a product that occurs more than once is multiplied once"""
    prod = {}
    out = []
    for g in groups:
        tp = None
        for pair in g:
            if pair not in prod:
                prod[pair] = orc.ct_mul(pool[pair[0]], pool[pair[1]], p)
            t = prod[pair]
            if tp is None:
                tp = t.copy()
            else:
                for i, q in enumerate(primes):
                    tp[:, i] = (tp[:, i] + t[:, i]) % np.uint64(q)
        out.append(orc.apply_key_switch(ksm, tp, logQ, nl))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def case(ring, xi, kind):
    """(primes, roots, ksm, pool, groups, expected) -- computed once per case, shared by its run variants, never written to"""
    m, logQ, p = ring
    primes, roots = P.chain_for(m, logQ, p, xi)
    _, n = R.zms_idx(m)
    nd, nl = R.ndigits(logQ), (logQ + 63) // 64
    path32 = m == 46 and xi > 1
    if kind == "wave":
        groups, npool = C.wave_groups(m), 12
    elif kind == "long":
        groups, npool = [C.long_group()], 2 * C.LONG_DISTINCT
    else:                                                   # 40 terms on the chain of single products; the crafted pair among them
        groups, npool = [[(t % 12, (5 * t + 1) % 12) for t in range(38)] + [(12, 13)] * 2], 12
    pool = pool_for(ring, primes, npool, path32)
    ksm = np.stack([P.rand_rows(np.random.default_rng(7 + m), primes, n, 3 * nd) for _ in range(2)])
    orc = O.Oracle(m, primes, roots)
    exp = oracle_sums(orc, primes, ksm, pool, groups, logQ, p, nl)
    for a in (ksm, pool, exp):
        a.setflags(write=False)
    return primes, roots, ksm, pool, groups, exp


def run(ring, xi, kind, options, kernel):
    m, logQ, p = ring
    primes, roots, ksm, pool, groups, exp = case(ring, xi, kind)
    ctx = F.Context(m, primes, roots)
    for name, v in options.items():
        ctx.set_option(name, v)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    a_idx = [x for g in groups for x, _ in g]
    b_idx = [y for g in groups for _, y in g]
    seg = np.cumsum([0] + [len(g) for g in groups])
    out = ctx.alloc(len(groups) * 2 * n * nl * 8)
    ctx.prof_enable(True)
    ctx.ct_mul_sum_relin_dev(ksk, logQ, p, ctx.upload(pool), nl, a_idx, b_idx, seg, out)
    name = ctx.prof_kernel_name("tensor")
    ctx.prof_enable(False)
    assert kernel in name, name                             # the intended sum kernel really ran ("tensor_sum_kernel" is no part of "tensor_sum32_kernel")
    got = out.download((len(groups), 2, n, nl))
    for gi, g in enumerate(groups):
        assert np.array_equal(got[gi], exp[gi]), (gi, len(g))


VARIANTS = [{}, {"batch_chunk": 3}, {"wave_operands": 2}]      # as it is; three groups per key switch; every group piecewise, one term per pass


@pytest.mark.parametrize("options", VARIANTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "plain")
@pytest.mark.parametrize("ring,kernel", [(C.M1024, SUM64), (C.M46, SUM32)])
def test_groups_around_the_fold_period_and_the_rounds(ring, kernel, options):
    F_ = C.fold_period()
    run(ring, C.longest_group(F_), "wave", options, kernel)      # xi = the longest group: the reference's own rule for sums (FHEContext.cpp:83-85)


@pytest.mark.parametrize("ring,kernel", [(C.M1024, SUM64), (C.M46, SUM32)])
def test_one_long_group_summed_piecewise(ring, kernel):
    """100 terms over 45 + 45 distinct operands, 80 operands per pass: passes of 40, 40 and 20 terms into one accumulator -- the accumulating
    passes fold on the 64-bit path and run ten rounds on the 30-bit path"""
    assert C.LONG_OPERANDS // 2 > C.fold_period()
    run(ring, C.LONG_TERMS, "long", {"wave_operands": C.LONG_OPERANDS}, kernel)


def test_chain_too_short_for_the_plan_takes_the_64_bit_kernel():
    """m = 46 with the chain of single products (xi = 1) and a group of 40 terms: the 30-bit plan does not apply, the call sums on the chain
    primes -- and still equals the oracle, since both wrap modulo the chain"""
    run(C.M46, 1, "short", {}, SUM64)
