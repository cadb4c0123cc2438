"""Model of a slot basis, written from the definition and independent of the library: k distinct primes p_c = 1 mod m on one two-row ring
(m = 2^3 .. 2^16, every p_c < 2^31), P = prod p_c.  A slot holds an integer modulo P, read as the signed representative in (-P/2, P/2);
channel c of a logical plaintext is the two-row plaintext (tests/slots_pow2_model.py) of the residues v mod p_c.  Everything here is Python
integers: residues, the Chinese remainder theorem by its formula, the centred lift.  Mixed-radix digits, Shoup constants, limb carries and
LDS are the device's business (fhe-si_amd/csrc/kernels_slots_basis.hip) and are tested against this file.
`python tests/slots_basis_model.py` rewrites tests/golden/slots_basis.json."""
from __future__ import annotations

import json
import os
import random
import sys
from typing import List, Sequence

if __name__ == "__main__":       # run as a script (the suite's conftest puts oracle/ on the path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import fhesi_pyref as R
import slots_pow2_model as M2

MAXK, MAXL = 32, 16


def ring_refusal(m: int, g: int):
    if m < 1 or m & (m - 1):
        return "power of two"
    if m < 8:
        return "k < 3"
    if m > 1 << 16:
        return "above 2^16"
    if g % m % 8 not in (3, 5):
        return "mod 8"
    return None


def refusal(m: int, primes: Sequence[int], g: int):
    """None, or a keyword naming the condition that takes the basis out of scope"""
    why = ring_refusal(m, g)
    if why:
        return why
    if len(primes) < 1:
        return "at least one"
    if len(primes) > MAXK:
        return "more than 32 primes"
    for c, p in enumerate(primes):
        if p >= 1 << 31:
            return "2^31"
        if not R.is_prime(p):
            return "not prime"
        if (p - 1) % m:
            return "ord_m(p) > 1"
        if p in primes[:c]:
            return "twice"
    return None


def limbs_of(P: int) -> int:
    return (P.bit_length() + 1 + 63) // 64


def plan(m: int, bits: int, prime_bits: int, g: int) -> List[int]:
    """the largest primes = 1 mod m below 2^prime_bits, descending, until P > 2^(bits + 1)"""
    why = ring_refusal(m, g)
    if why:
        raise ValueError(why)
    primes, P = [], 1
    cand = ((1 << prime_bits) - 2) // m * m + 1
    while P <= 1 << (bits + 1):
        while cand > m and not R.is_prime(cand):
            cand -= m
        if cand <= m:
            raise ValueError("not enough primes")
        if len(primes) == MAXK:
            raise ValueError("more than 32 primes")
        primes.append(cand)
        P *= cand
        cand -= m
    return primes


class SlotBasis:
    def __init__(self, m: int, primes: Sequence[int], g: int):
        why = refusal(m, list(primes), g)
        if why:
            raise ValueError(why)
        self.m, self.g, self.primes, self.k = m, g % m, list(primes), len(primes)
        self.total, self.rows, self.cols = m // 2, 2, m // 4
        self.modulus = 1
        for p in primes:
            self.modulus *= p
        self.limbs = limbs_of(self.modulus)
        self._ch = {}

    def channel(self, c: int) -> M2.SlotSpace:
        if c not in self._ch:
            self._ch[c] = M2.slot_space(self.m, self.primes[c], self.g)
        return self._ch[c]


def centred(v: int, P: int) -> int:
    """the representative of v modulo the odd P in (-P/2, P/2)"""
    v %= P
    return v - P if v > P // 2 else v


def crt(res: Sequence[int], primes: Sequence[int]) -> int:
    """the integer in [0, P) with the given residues: sum r_c (P / p_c) ((P / p_c)^-1 mod p_c) mod P"""
    P = 1
    for p in primes:
        P *= p
    return sum(r * (P // p) * pow(P // p, -1, p) for r, p in zip(res, primes)) % P


def residues(vals: Sequence[int], p: int) -> List[int]:
    return [v % p for v in vals]


def embed(B: SlotBasis, vals: Sequence[int]) -> List[List[int]]:
    """[k][n]: channel c is the two-row embedding of vals mod p_c"""
    return [M2.embed_slots(B.channel(c), residues(vals, B.primes[c])) for c in range(B.k)]


def decode(B: SlotBasis, msgs: Sequence[Sequence[int]], nvals: int = None) -> List[int]:
    nvals = B.total if nvals is None else nvals
    per = [M2.decode_slots(B.channel(c), msgs[c], nvals) for c in range(B.k)]
    return [centred(crt([per[c][j] for c in range(B.k)], B.primes), B.modulus) for j in range(nvals)]


def to_limbs(v: int, L: int) -> List[int]:
    """L little-endian 64-bit limbs, two's complement, as unsigned words"""
    assert -(1 << (64 * L - 1)) <= v < 1 << (64 * L - 1)
    v &= (1 << (64 * L)) - 1
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(L)]


def from_limbs(w: Sequence[int]) -> int:
    L = len(w)
    v = sum((int(x) & 0xFFFFFFFFFFFFFFFF) << (64 * i) for i, x in enumerate(w))
    return v - (1 << (64 * L)) if v >> (64 * L - 1) else v


def fixture_cases():
    rnd = random.Random(20261016)
    out = []
    for m, primes, g in [(8, [17, 41], 3), (16, [97, 17, 113], 5), (32, [193, 97], 3), (16, plan(16, 20, 31, 3), 3), (32, plan(32, 100, 31, 3), 3),
                         (64, [257, 193, 449, 577, 641], 5)]:
        B = SlotBasis(m, primes, g)
        half = (B.modulus - 1) // 2
        vals = [half, -half, 0, -1] + [rnd.randint(-half, half) for _ in range(B.total - 4)]
        vals = vals[:B.total]
        out.append({"m": m, "primes": primes, "g": g, "modulus": str(B.modulus), "limbs": B.limbs, "vals": [str(v) for v in vals], "msg": embed(B, vals)})
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slots_basis.json")
    with open(path, "w") as f:
        json.dump({"cases": fixture_cases()}, f, separators=(",", ":"))
    print("wrote", path)
