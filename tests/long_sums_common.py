"""What tests/test_gpu_long_sums.py, tests/test_gpu_ew_edges.py and tests/test_long_sums_model.py share: the fold period of tensor_sum_kernel as the
library compiles it, the tensor half's prime rule and plan condition restated from kernels_tensor32.hip, and the constant polynomials whose
evaluation rows sit at the top of the residue range."""
import math
import os
import re

import numpy as np

import fhesi_pyref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M1024 = (1024, 128, 23)         # the 64-bit path (tensor_sum_kernel): a power-of-two ring below the rows of 2^14
M46 = (46, 128, 47)             # the 30-bit path on padded rows (tensor_sum32_kernel)
LONG_TERMS, LONG_OPERANDS, LONG_DISTINCT = 100, 80, 45      # one long group alone: passes of 40, 40 and 20 terms


def fold_period():
    """terms between two folds of tensor_sum_kernel's 128-bit accumulators, read from `if (((t - t0) & 31) == 31)`"""
    src = open(os.path.join(ROOT, "fhe-si_amd", "csrc", "kernels_ew.hip")).read()
    body = src[src.index("void __launch_bounds__(256) tensor_sum_kernel("):]
    mask, at = re.search(r"\(\(t - t0\) & (\d+)\) == (\d+)\)", body).groups()
    assert mask == at and (int(mask) + 1) & int(mask) == 0
    return int(mask) + 1


def group_lengths(F):
    """before, at and after the fold period, twice and three times it; whole four-term rounds of tensor_sum32_kernel and tails of 1 to 3
    (6: the tail of two, which the lengths around the period do not give)"""
    return [1, 4, 5, 6, 8, F - 1, F, F + 1, 2 * F, 2 * F + 1, 3 * F + 1]


def crafted_terms(F):
    """the longest group: crafted pairs only.  Its middle accumulator takes two products of (q - 1)^2 per term, and with the chain's 60-bit
    primes 2 (4 F + 2) (q - 1)^2 passes 2^128 (test_long_sums_model.py): without the fold the sum wraps, which shorter groups never show"""
    return 4 * F + 2


def longest_group(F):
    return max(group_lengths(F) + [crafted_terms(F)])


def tensor_primes(lg, count, bits=30):
    """the tensor half's primes on rows of 2^lg (t32_plan_search; primes_below_2_30 of test_arith32_models.py): the largest below 2^bits that are 1 mod 2^(lg+1)"""
    step, out = 1 << (lg + 1), []
    q = (1 << bits) + 1
    while len(out) < count:
        q -= step
        if R.is_prime(q):
            out.append(q)
    return out


def t32_TB(logQ, p, phim, gmax, lin):
    """kernels_tensor32.hip: TB = 2 (logQ - 1) + bits(p) + log2(coefficients) + 1 + log2(terms per sum) + 2 on the folded rings, logarithms rounded up"""
    up = lambda v: (v - 1).bit_length()
    return 2.0 * (logQ - 1) + p.bit_length() + up(phim) + 1 + up(gmax) + (2 if lin else 0)


def chain_bits(primes):
    return sum(math.log2(q) for q in primes)


def plan_applies(primes, logQ, p, phim, gmax, lin):
    """t32_plan_search's condition on the chain (the ring and the room in the table rows are not restated)"""
    return chain_bits(primes) >= t32_TB(logQ, p, phim, gmax, lin) + 1.5


def crafted_constants(p, q0, q1):
    """(c, d): c p = -1 and d = -1 modulo q0 q1, both in [0, q0 q1).  A constant polynomial has every evaluation equal to the constant, and the
    left operand of a product is lifted by p: every word of the rows modulo q0 and q1 is q - 1."""
    mod = q0 * q1
    return (-pow(p, -1, mod)) % mod, mod - 1


def constant_ct(n, nl, v0, v1):
    """[2][n][nl]: the ciphertext whose two parts are the constant polynomials v0 and v1"""
    ct = np.zeros((2, n, nl), dtype=np.uint64)
    ct[0, 0] = O.ints_to_limbs([v0], nl)[0]
    ct[1, 0] = O.ints_to_limbs([v1], nl)[0]
    return ct


def wave_groups(m):
    """the groups of the wave of long sums on the ring m: a pool of 12 random ciphertexts -- shared between groups, repeated inside a group,
    squares included -- and entries 12 (left) and 13 (right) crafted; the last three groups, of F + 1, of 8 and of crafted_terms(F) terms, are
    crafted pairs only"""
    F = fold_period()
    rng = np.random.default_rng(m)
    groups = []
    for ln in group_lengths(F):
        g = [(int(x), int(y)) for x, y in rng.integers(0, 12, size=(ln, 2))]
        g[0] = (g[0][0], g[0][0])                               # a square
        if ln >= 4:
            g[-1] = g[1]                                        # a repeated product
        groups.append(g)
    groups += [[(12, 13)] * (F + 1), [(12, 13)] * 8, [(12, 13)] * crafted_terms(F)]
    return groups


def long_group():
    """LONG_TERMS terms over LONG_DISTINCT distinct left (0 ..) and as many distinct right operands (LONG_DISTINCT ..)"""
    return [(t % LONG_DISTINCT, LONG_DISTINCT + 7 * t % LONG_DISTINCT) for t in range(LONG_TERMS)]
