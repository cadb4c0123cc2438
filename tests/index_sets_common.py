"""What the index-set tests share (test_gpu_index_sets.py on the device, test_index_sets_oracle.py on the CPU): a chain of five primes of
different sizes, the proper index sets over it, and polynomials centred within the product of a set's primes.

The chain is (60, small, 59, 49, 60) bits by index.  A DoubleCRT over a proper subset reaches the kernels with a slot -> prime map; with this
chain a slot number taken for a prime index changes the modulus, the form the tile kernels run the row in (a prime below 2^48 goes modulo a
60-bit multiple of itself, PrimeConst::q_tile) and the class of the closing reduction at once.  The small prime sits at index 1, so no prefix
of the chain holds it alone."""
import random

import numpy as np

import params as P

SETS = ([1], [1, 3], [0, 2, 4], [2, 3, 4])         # the small prime alone; two classes below 2^60, no prefix; gaps; a suffix
FULL = [0, 1, 2, 3, 4]                             # the control: the identity set reaches the kernels with a null map


def small_bits(m: int) -> int:
    """size of the small prime: on m = 2^k the rule of test_gpu_ntt.py on n = m / 2 (20 bits at least, log2(n) + 4 up to n = 2^12, log2(n) + 8
    above).  On every other ring n = phi(m) is no power of two and the primes are 1 modulo 2m, so the same margin of 8 bits stands on the bit
    length of 2m, from 21 bits: 21 at m = 45, 25 at m = 32771."""
    if m == 1 << 19:
        return 25                                  # the rule gives 26, and no prime of 26 bits is 1 mod 2^20: one bit less
    if m & (m - 1) == 0:
        logn = m.bit_length() - 2
        return max(20, logn + (4 if logn <= 12 else 8))
    return max(21, (2 * m).bit_length() + 8)


def mixed_chain(m: int):
    """-> (primes, roots, bits): every prime is the first one = 1 mod 2m below 2^bits, the two 60-bit ones the first two"""
    bits = (60, small_bits(m), 59, 49, 60)
    big, broots = P.first_primes(m, 2, 60)
    primes, roots = [big[0]], [broots[0]]
    for b in bits[1:4]:
        q, r = P.first_primes(m, 1, b)
        primes.append(q[0])
        roots.append(r[0])
    primes.append(big[1])
    roots.append(broots[1])
    assert [q.bit_length() for q in primes] == list(bits), (m, [q.bit_length() for q in primes])
    assert primes[1] < 1 << 48 <= primes[3]
    return primes, roots, bits


def product(primes, S) -> int:
    out = 1
    for i in S:
        out *= primes[i]
    return out


def to_limbs(vals, nlimbs: int) -> np.ndarray:
    """oracle_lib.ints_to_limbs (signed Python integers -> [len][nlimbs] two's complement words), through bytes: rows of 2^18 coefficients"""
    mod, nb = 1 << (64 * nlimbs), 8 * nlimbs
    buf = b"".join((v % mod).to_bytes(nb, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), nlimbs).astype(np.uint64)


def to_ints(limbs: np.ndarray) -> list:
    """oracle_lib.limbs_to_ints, through bytes"""
    nb = 8 * limbs.shape[-1]
    buf = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(buf[o:o + nb], "little", signed=True) for o in range(0, len(buf), nb)]


def centred_poly(n: int, PS: int, seed: int) -> list:
    """n coefficients in [-(PS - 1) / 2, (PS - 1) / 2]: the two ends, 0, 1, -1 first, the lower end last, the rest uniform (n = 8 holds all six)"""
    half = (PS - 1) // 2
    rng = random.Random(seed)
    poly = [rng.randrange(-half, half + 1) for _ in range(n)]
    poly[:5] = [half, -half, 0, 1, -1]
    poly[n - 1] = -half
    return poly
