"""Model of the two-row slot space of a power-of-two ring, written from the definition and independent of the library: m = 2^k (k >= 3),
n = m/2, h = n/2, p prime, p = 1 mod m, g = 3 or 5 mod 8.  X^n + 1 has the n roots rho0^e, e odd, modulo p; (Z/m)^* = <-1> x <g>, so slot
s = r h + j (row r, column j) is the VALUE a(rho0^(e_s)), e_s = (-1)^r g^j mod m, with rho0 the least integer in [1, p) of order m.
Decoding evaluates at the roots (Horner); embedding interpolates by the direct O(n^2) inverse.  Nothing here knows about transforms,
bit reversal, LDS or chirps: those are the device's business (fhe-si_amd/csrc/kernels_slots_pow2.hip) and are tested against this file."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

import fhesi_pyref as R
import slots_model as M


def refusal(m: int, p: int, g: int):
    """None, or a keyword naming the condition that takes (m, p, g) out of scope"""
    if m < 1 or m & (m - 1):
        return "power of two"
    if m < 8:
        return "k < 3"
    if p >= 1 << 32:
        return "2^32"
    if not R.is_prime(p):
        return "not prime"
    if (p - 1) % m:
        return "ord_m(p) > 1"
    if g % 8 not in (3, 5):
        return "mod 8"
    return None


def path(m: int, p: int) -> int:
    """0: the direct transform (n <= 2^15, p < 2^31); else the chirp with 1 or 2 auxiliary primes (m p^2 against 2^59)"""
    if m // 2 <= 1 << 15 and p < 1 << 31:
        return 0
    return 1 if m * p * p < 1 << 59 else 2


class SlotSpace:
    def __init__(self, m: int, p: int, g: int):
        why = refusal(m, p, g)
        if why:
            raise ValueError(why)
        self.m, self.p, self.g = m, p, g % m
        self.total = self.usable = m // 2
        self.rows, self.cols = 2, m // 4
        self.rho0 = M.least_root_of_order(m, p)
        col = [pow(g, j, m) for j in range(self.cols)]
        self.exps = col + [m - e for e in col]
        assert sorted(self.exps) == list(range(1, m, 2)), "the two rows do not reach every odd exponent"
        self.roots = [pow(self.rho0, e, p) for e in self.exps]
        self.path = path(m, p)

    def cap(self, only_usable: bool = True) -> int:
        return self.total


def slot_space(m: int, p: int, g: int) -> SlotSpace:
    return SlotSpace(m, p, g)


decode_slot = M.decode_slot


def decode_slots(S: SlotSpace, a: Sequence[int], nvals: int = None, only_usable: bool = True) -> List[int]:
    nvals = S.total if nvals is None else nvals
    return [decode_slot(S, a, j) for j in range(nvals)]


def embed_slots(S: SlotSpace, vals: Sequence[int], only_usable: bool = True) -> List[int]:
    """the polynomial of degree < n whose slot s is vals[s] for s < len(vals) and 0 elsewhere: a_i = n^-1 sum_s v_s root_s^-i (the roots of
    X^n + 1 satisfy sum_s root_s^d = 0 for 0 < |d| < n)"""
    n, p = S.total, S.p
    take = min(len(vals), n)
    ninv = pow(n, -1, p)
    if p < 1 << 20 and take:      # sums of n products below 2^40 fit int64
        v = np.array([x % p for x in vals[:take]], dtype=np.int64)
        rinv = np.array([pow(r, -1, p) for r in S.roots[:take]], dtype=np.int64)
        cur, out = np.ones(take, dtype=np.int64), []
        for _ in range(n):
            out.append(int((v * cur).sum() % p) * ninv % p)
            cur = cur * rinv % p
        return out
    rinv = [pow(r, -1, p) for r in S.roots[:take]]
    return [sum(vals[s] % p * pow(rinv[s], i, p) for s in range(take)) * ninv % p for i in range(n)]


def automorph(S: SlotSpace, a: Sequence[int], k: int) -> List[int]:
    """a(X^k) mod (X^n + 1, p)"""
    n, p = S.total, S.p
    b = [0] * n
    for i, c in enumerate(a):
        e = i * k % S.m
        if e < n:
            b[e] = (b[e] + c) % p
        else:
            b[e - n] = (b[e - n] - c) % p
    return b


def poly_mul(S: SlotSpace, a: Sequence[int], b: Sequence[int]) -> List[int]:
    """a b mod (X^n + 1, p)"""
    n, p = S.total, S.p
    f = R.poly_mul(list(a), list(b)) + [0] * (2 * n)
    return [(f[i] - f[i + n]) % p for i in range(n)]


def total_sum_exponents(S: SlotSpace) -> List[int]:
    """g, g^2, g^4, ..., g^(h/2), then m - 1: log2 n automorphisms, each followed by an addition, leave the sum of all slots in every slot"""
    ks, k, c = [], S.g, S.cols
    while c > 1:
        ks.append(k)
        k = k * k % S.m
        c >>= 1
    return ks + [S.m - 1]


def rotate_rows(S: SlotSpace, v: Sequence[int], t: int) -> List[int]:
    h = S.cols
    return [v[r * h + (j + t) % h] for r in range(2) for j in range(h)]


def swap_rows(S: SlotSpace, v: Sequence[int]) -> List[int]:
    return list(v[S.cols:]) + list(v[:S.cols])
