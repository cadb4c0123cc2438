"""Model of plaintext slot packing (PlaintextSpace / Plaintext::EmbedInSlots / DecodeSlots, Regression::GenerateNoise), written from the
definition: slot j of a polynomial a is the VALUE a(rho0^(e_j)) modulo p, e_j = g^j mod m, where p is prime, p = 1 mod m, g generates (Z/m)^*
and rho0 is the least integer in [1, p) of multiplicative order m.  Decoding evaluates at the roots; embedding interpolates by the direct
O(m^2) inverse DFT and one long division by Phi_m.  Nothing here knows about chirps, auxiliary primes or folds: those are the device's
business (fhe-si_amd/csrc/kernels_slots.hip) and are tested against this file."""
from __future__ import annotations

from math import gcd
from typing import List, Sequence

import numpy as np

import fhesi_pyref as R

PHX_SLOT_NOISE = 7      # purpose code of the noise-mask stream (fhe-si_amd/csrc/philox.h)


def _prime_factors(n: int) -> List[int]:
    return sorted(set(R.factorize(n))) if n > 1 else []


def order_mod(x: int, n: int) -> int:
    """multiplicative order of x modulo n (gcd(x, n) = 1), by brute force"""
    k, y = 1, x % n
    while y != 1 % n:
        y = y * x % n
        k += 1
    return k


def refusal(m: int, p: int, g: int):
    """None, or a keyword naming the condition that takes (m, p, g) out of scope"""
    if p >= 1 << 32:
        return "p >= 2^32"
    if not R.is_prime(p):
        return "not prime"
    if (p - 1) % m:
        return "ord_m(p) > 1"
    units = [x for x in range(1, m) if gcd(x, m) == 1] if m > 2 else [1]
    if gcd(g, m) != 1:
        return "generator"
    if m <= 4096:
        walk = {pow(g, j, m) for j in range(len(units))}
        if len(walk) != len(units):
            # cyclic at all?
            cyclic = any(len({pow(u, j, m) for j in range(len(units))}) == len(units) for u in units)
            return "generator" if cyclic else "not cyclic"
    return None


def least_root_of_order(m: int, p: int) -> int:
    """the least x in [1, p) with x^m = 1 and x^(m/f) != 1 for every prime f | m"""
    fm = _prime_factors(m)

    def has_order_m(x):
        return pow(x, m, p) == 1 and all(pow(x, m // f, p) != 1 for f in fm)

    if p < 1 << 18:
        return next(x for x in range(1, p) if has_order_m(x))
    # large p: the elements of order m are z^j, gcd(j, m) = 1, for any one z of order m
    z = next(c for c in (pow(h, (p - 1) // m, p) for h in range(2, p)) if has_order_m(c))
    best, x = p, 1
    for j in range(1, m):
        x = x * z % p
        if x < best and gcd(j, m) == 1:
            best = x
    return best


class SlotSpace:
    def __init__(self, m: int, p: int, g: int):
        why = refusal(m, p, g)
        if why:
            raise ValueError(why)
        self.m, self.p, self.g = m, p, g % m
        self.total = R.zms_idx(m)[1]
        self.usable = 1 << (self.total.bit_length() - 1)
        self.rho0 = least_root_of_order(m, p)
        self.exps = [pow(g, j, m) for j in range(self.total)]
        assert len(set(self.exps)) == self.total, "generator"
        self.roots = [pow(self.rho0, e, p) for e in self.exps]
        self._phi = None

    @property
    def phi(self):
        if self._phi is None:
            self._phi = R.cyclotomic(self.m)
        return self._phi

    def cap(self, only_usable: bool = True) -> int:
        return self.usable if only_usable else self.total


def slot_space(m: int, p: int, g: int) -> SlotSpace:
    return SlotSpace(m, p, g)


def decode_slot(S: SlotSpace, a: Sequence[int], j: int) -> int:
    r, v = S.roots[j], 0
    for c in reversed(a):
        v = (v * r + c) % S.p
    return v


def decode_slots(S: SlotSpace, a: Sequence[int], nvals: int = None, only_usable: bool = True) -> List[int]:
    nvals = S.total if nvals is None else nvals
    take = min(nvals, S.cap(only_usable))
    return [decode_slot(S, a, j) if j < take else 0 for j in range(nvals)]


def embed_slots(S: SlotSpace, vals: Sequence[int], only_usable: bool = True) -> List[int]:
    """the polynomial of degree < phi(m) whose slot j is vals[j] for j < min(len(vals), cap) and 0 elsewhere"""
    m, p = S.m, S.p
    take = min(len(vals), S.cap(only_usable))
    x = [0] * m
    for j in range(take):
        x[S.exps[j]] = vals[j] % p
    rinv, minv = pow(S.rho0, -1, p), pow(m, -1, p)
    if p < 1 << 20:      # sums of m products below 2^40 fit int64
        k = np.array([e for e in S.exps[:take]], dtype=np.int64)
        xv = np.array([x[e] for e in S.exps[:take]], dtype=np.int64)
        rp = np.ones(m, dtype=np.int64)
        for i in range(1, m):
            rp[i] = rp[i - 1] * rinv % p
        f = []
        for i in range(m):
            f.append(int((xv * rp[(k * i) % m]).sum() % p) * minv % p)
    else:
        f = [sum(x[e] * pow(rinv, i * e, p) for e in S.exps[:take]) * minv % p for i in range(m)]
    return R.poly_rem_monic(f, S.phi, p)


def draw_noise_slots(S: SlotSpace, seed: int, index: int) -> List[int]:
    """slot values of the noise mask of object `index`: slot 0 is 0, slot j >= 1 is floor(u p / 2^64), u = word0 | word1 << 32"""
    out = [0]
    for j in range(1, S.total):
        w = R.phx_draw(seed, index, j, PHX_SLOT_NOISE)
        out.append(((w[0] | w[1] << 32) * S.p) >> 64)
    return out


def automorph_mod_phi(S: SlotSpace, a: Sequence[int], k: int) -> List[int]:
    """a(X^k) mod (Phi_m, p)"""
    b = [0] * S.m
    for i, c in enumerate(a):
        b[i * k % S.m] = (b[i * k % S.m] + c) % S.p
    return R.poly_rem_monic(b, S.phi, S.p)


def poly_mul_mod_phi(S: SlotSpace, a: Sequence[int], b: Sequence[int]) -> List[int]:
    return R.poly_rem_monic(R.poly_mul(list(a), list(b)), S.phi, S.p)


def least_generator(m: int) -> int:
    """the least g >= 1 generating (Z/m)^* (m = 2, 4, q^k, 2 q^k)"""
    n = R.zms_idx(m)[1]
    fs = _prime_factors(n)
    for g in range(1, m):
        if gcd(g, m) == 1 and all(pow(g, n // f, m) != 1 for f in fs):
            return g
    raise ValueError("not cyclic")
