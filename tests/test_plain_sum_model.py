"""CPU: the arithmetic fhesi_ct_plain_sum_dev rests on, without a GPU.
(a) an integer model of plain_sum_kernel's accumulate-and-fold schedule, with wrap-around at 128 bits, on worst-case operands;
(b) fhesi_plain_sum_bits, the capacity rule, against its stated formula and against brute force on small rings;
(c) the ABI revision the header, the binding and the library agree on."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M128 = (1 << 128) - 1


def fold_period():
    """kPlainSumFold as the library compiles it"""
    src = open(os.path.join(ROOT, "fhe-si_amd", "csrc", "fhesi_internal.h")).read()
    return int(re.search(r"constexpr int kPlainSumFold = (\d+);", src).group(1))


def admitted_bits():
    """the widest residue launch_plain_sum admits (bar_k = bit length of q)"""
    src = open(os.path.join(ROOT, "fhe-si_amd", "csrc", "kernels_plain.hip")).read()
    return int(re.search(r"bar_k > (\d+)\) FHESI_FAIL\(\"plain_sum", src).group(1))


def prime_below(bound):
    q = bound - 1
    while not R.is_prime(q):
        q -= 1
    return q


def kernel_schedule(q, a, w, period, carry=0):
    """One accumulator of plain_sum_kernel over the terms a[t] * w[t]: 128-bit multiply-add (acc_mad), a fold modulo q after every `period`
    terms while more terms follow, the closing reduction (acc_reduce).  -> (stored residue, whether the 128-bit word ever wrapped)"""
    acc, wrapped, t, T = carry, False, 0, len(a)
    while t < T:
        te = T if T - t < period else t + period
        while t < te:
            s = acc + a[t] * w[t]
            wrapped |= s > M128
            acc = s & M128
            t += 1
        if t < T:
            acc %= q
    return acc % q, wrapped


def test_fold_period_is_derived_from_the_admitted_width():
    F_, k = fold_period(), admitted_bits()
    top = (1 << k) - 1                      # residues are below q < 2^k, a carried-in value too
    assert F_ * top * top + top <= M128     # F terms never wrap ...
    assert (F_ + 1) * top * top > M128      # ... and F is the largest such period for that width


@pytest.mark.parametrize("which", ["below_2^60", "widest_admitted"])
def test_accumulate_and_fold_schedule_never_wraps(which):
    """Worst case: every residue q - 1, the accumulator carried in at q - 1 (a piecewise sum).  The stored word is the exact sum modulo q."""
    F_ = fold_period()
    q = prime_below(1 << 60) if which == "below_2^60" else prime_below(1 << admitted_bits())
    assert q.bit_length() == (60 if which == "below_2^60" else admitted_bits())
    for T in (F_ - 1, F_, F_ + 1, 4 * F_):
        for carry in (0, q - 1):
            got, wrapped = kernel_schedule(q, [q - 1] * T, [q - 1] * T, F_, carry)
            assert not wrapped, (T, carry)
            assert got == (carry + T * (q - 1) * (q - 1)) % q, (T, carry)
    rng = np.random.default_rng(5)
    a = [int(x) for x in rng.integers(0, q, size=3 * F_ + 7)]
    w = [int(x) for x in rng.integers(0, q, size=3 * F_ + 7)]
    assert kernel_schedule(q, a, w, F_) == (sum(x * y for x, y in zip(a, w)) % q, False)


def test_a_fold_one_term_late_wraps():
    """The same model folding after F + 1 terms: on the widest admitted residue the accumulator wraps as soon as a run of F + 1 terms exists
    and the stored word is wrong, so the test above can see the bug.  (Below 2^60 a product is under 2^120 and even 65 of them stay four times
    below 2^128: only the widest residue can show a late fold, which is why the period is derived from it.)"""
    F_ = fold_period()
    q = prime_below(1 << admitted_bits())
    for T in (F_ + 1, 4 * F_):
        got, wrapped = kernel_schedule(q, [q - 1] * T, [q - 1] * T, F_ + 1)
        assert wrapped and got != (T * (q - 1) * (q - 1)) % q, T
    for T in (F_ - 1, F_):                                      # no run of F + 1 terms: nothing to see yet
        assert not kernel_schedule(q, [q - 1] * T, [q - 1] * T, F_ + 1)[1]
    q60 = prime_below(1 << 60)
    assert not kernel_schedule(q60, [q60 - 1] * (4 * F_), [q60 - 1] * (4 * F_), F_ + 1)[1]


# ---------------------------------------------------------------------------------------------------------------------------------- (b)
def growth_bits(m):
    """log2 of the growth the remainder modulo Phi_m is sized with: 1 (a power of two), 2 (m = q^k, 2 q^k, q an odd prime), phi(m) otherwise"""
    n = R.zms_idx(m)[1]
    if m >= 4 and m & (m - 1) == 0:
        return 0.0
    Q = m if m & 1 else m // 2
    if Q & 1 and Q >= 3 and len(set(R.factorize(Q))) == 1:
        return 1.0
    return math.log2(n)


@pytest.mark.parametrize("m", [64, 22, 50, 21, 4096, 105])
def test_plain_sum_bits_is_the_stated_formula(m):
    """fhesi_plain_sum_bits = log2(2 T growth n 2^(logQ-1) maxabs); loads the library without a GPU (the parent commit lacks the symbol)."""
    n = R.zms_idx(m)[1]
    for logQ, maxabs, T in ((90, 256, 1), (128, 65536, 16), (80, 22, 1 << 20), (100, 1, 3), (512, (1 << 62) + 12345, 7)):
        want = 1 + math.log2(T) + growth_bits(m) + math.log2(n) + (logQ - 1) + math.log2(maxabs)
        assert abs(F.plain_sum_bits(m, logQ, maxabs, T) - want) < 1e-9, (m, logQ, maxabs, T)
    assert F.plain_sum_bits(m, 90, 0, 5) == 0.0 and F.plain_sum_bits(m, 90, 7, 0) == 0.0
    lib = ctypes.CDLL(F.library_path())
    assert hasattr(lib, "fhesi_plain_sum_bits")
    for bad in ((1, 90, 3, 1), (m, 0, 3, 1), (m, 90, 3, -1), ((1 << 20) + 1, 90, 3, 1)):
        with pytest.raises(F.FhesiError, match="plain_sum_bits"):
            F.plain_sum_bits(*bad)


def product_matrices(m):
    """M[j][i][k] = coefficient j of X^(i + k) rem Phi_m: the product a w rem Phi_m is bilinear, c_j = a^T M[j] w"""
    phi = R.cyclotomic(m)
    n = len(phi) - 1
    red = []
    for e in range(2 * n - 1):
        r = [0] * e + [1]
        while len(r) > n:                                       # Phi_m is monic
            c = r.pop()
            for d in range(n):
                r[len(r) - n + d] -= c * phi[d]
        red.append(r + [0] * (n - len(r)))
    M = np.zeros((n, n, n), dtype=np.int64)
    for i in range(n):
        for k in range(n):
            M[:, i, k] = red[i + k]
    return M


@pytest.mark.parametrize("m", [8, 16, 7, 9, 14, 18, 12, 15, 20, 24])
def test_brute_force_products_stay_inside_the_bound(m):
    """Rings of n <= 8: over ALL sign patterns of a ciphertext part at the extreme magnitude 2^(logQ-1) and a plaintext at maxabs, the largest
    coefficient of T equal products is within the bound fhesi_plain_sum_bits returns (and meets it exactly where the growth is exact)."""
    M = product_matrices(m)
    n = M.shape[0]
    assert n <= 8 and n == R.zms_idx(m)[1]
    signs = np.array(list(itertools.product((-1, 1), repeat=n)), dtype=np.int64)          # [2^n][n]
    # max over w in {+-1}^n of a^T M_j w is the 1-norm of a^T M_j
    best = max(int(np.abs(signs @ M[j]).sum(axis=1).max()) for j in range(n))
    logQ, maxabs, T = 40, 1000, 5
    worst = T * best * (1 << (logQ - 1)) * maxabs
    bits = F.plain_sum_bits(m, logQ, maxabs, T)
    assert worst <= 2.0 ** (bits - 1) * (1 + 1e-12), (best, n)
    if m & (m - 1) == 0:
        assert best == n                                        # X^n + 1: the bound is attained


# ---------------------------------------------------------------------------------------------------------------------------------- (c)
def test_abi_revision_9():
    header = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    assert int(re.search(r"#define FHESI_ABI_VERSION (\d+)", header).group(1)) == 9 == F.binding.ABI_VERSION
    lib = ctypes.CDLL(F.library_path())
    lib.fhesi_abi_version.restype = ctypes.c_int32
    assert lib.fhesi_abi_version() == 9
