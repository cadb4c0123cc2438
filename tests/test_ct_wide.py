"""CPU (no GPU): the multi-limb steps of the coefficient-domain ciphertext kernels (fhe-si_amd/csrc/ct_wide.h: add with carry, multiply by a word,
negation, the signed limb of a gathered term, the centred store, the floor division of Ciphertext += ZZX, Decrypt's rounding and the noise
residual) as the stand-alone program tests/host/ct_wide_check.cpp runs them on the host under AddressSanitizer + UndefinedBehaviorSanitizer,
against Python integers.  The cases are drawn here; the program reads them from standard input and prints limbs.

Every limb class the kernels are compiled for (2, 4, 8, 9, 16, 17, 32, 34) with nl at both ends of the class within its launcher's list
(2 / 8 / 16 / 32, 2 / 9 / 17 / 32, 4 / 8 / 16 / 34); logQ at 64 nl, 64 nl - 1,
64 (nl - 1) + 1 and in between -- the shift counts 0, 63 and 1 of the sign bit, the top limb's mask and the split of the constant; operands of
all ones, the two extremes of the centred range, 0 and random; multipliers 1, 2^63 and 2^64 - 1."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
FAMILIES = ((2, 8, 16, 32), (2, 9, 17, 32), (4, 8, 16, 34))      # the launchers' class lists: limbs, words of logQ + 1 bits, limbs + 2
W = 1 << 64


def ends(fam, i):
    """the counts at both ends of class i of a family: one above the class below (1 for the first), and the class itself"""
    return {fam[i - 1] + 1 if i else 1, fam[i]}


SHAPES = sorted({(fam[i], nl) for fam in FAMILIES for i in range(len(fam)) for nl in ends(fam, i)})


def logqs(nl):
    return sorted({64 * nl, 64 * nl - 1, 64 * (nl - 1) + 1, 64 * (nl - 1) + 33})


def limbs(v, n):
    """the low n limbs of v (two's complement for a negative v), as the program reads them"""
    v %= 1 << (64 * n)
    return " ".join(hex((v >> (64 * i)) & (W - 1)) for i in range(n))


def centred(v, logQ):
    h = 1 << (logQ - 1)
    return ((v + h) % (1 << logQ)) - h


def stored(v, nl, logQ):
    """what the centred store leaves: the centred residue as nl two's complement limbs"""
    c = centred(v, logQ) % (1 << (64 * nl))
    return [(c >> (64 * i)) & (W - 1) for i in range(nl)]


def operands(rng, nl, logQ):
    full, lo = (1 << (64 * nl)) - 1, 1 << (logQ - 1)
    return [full, (-lo) % (full + 1), lo - 1, lo, 0, 1, rng.getrandbits(64 * nl), rng.getrandbits(64 * nl)]


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-C", HOST, "ct_wide_check"], stdout=subprocess.DEVNULL)

    def run(cases):
        """cases: [(input line, expected words)]"""
        text = "\n".join(line for line, _ in cases) + "\n"
        r = subprocess.run([os.path.join(HOST, "ct_wide_check")], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        got = [[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()]
        assert len(got) == len(cases)
        for (line, want), g in zip(cases, got):
            assert g == want, line[:300]
    return run


def test_add_with_carry_and_centred_store(check):
    rng, cases = random.Random(1), []
    for M, nl in SHAPES:
        for logQ in logqs(nl):
            ops = operands(rng, nl, logQ)
            for x in ops:
                for f in ops[:4] + ops[6:]:
                    g, carry, two = rng.choice(ops), rng.choice((0, 1, 2)), rng.choice((0, 1))
                    s = x + f + (g if two else 0) + carry
                    cases.append((f"add {M} {nl} {logQ} {carry} {two} {limbs(x, nl)} {limbs(f, nl)} {limbs(g, nl)}", [s >> (64 * nl)] + stored(s, nl, logQ)))
    check(cases)


def test_multiply_by_a_word_and_negation(check):
    rng, cases = random.Random(2), []
    for M, nl in SHAPES:
        for logQ in logqs(nl):
            ops = operands(rng, nl, logQ)
            for f in ops:
                for w in (1, 1 << 63, W - 1, 0, rng.getrandbits(64)):
                    for x in (0, ops[0], rng.choice(ops)):              # 0: *= long and 2 p z; otherwise the accumulation of delta * msg
                        neg = rng.choice((0, 1))
                        s = x + f * w
                        cases.append((f"mul {M} {nl} {logQ} {hex(w)} {neg} {limbs(x, nl)} {limbs(f, nl)}", [s >> (64 * nl)] + stored(-s if neg else s, nl, logQ)))
    check(cases)


def test_signed_terms_of_a_gather(check):
    rng, cases = random.Random(3), []
    for M, nl in SHAPES:
        for logQ in logqs(nl):
            ops = operands(rng, nl, logQ)
            for s1 in (-1, 0, 1):
                for s2 in (-1, 0, 1):
                    for a1 in ops[:3] + ops[4:5] + ops[6:7]:
                        x, a2 = rng.choice(ops), rng.choice(ops)
                        cases.append((f"gather {M} {nl} {logQ} {s1} {s2} {limbs(x, nl)} {limbs(a1, nl)} {limbs(a2, nl)}", stored(x + s1 * a1 + s2 * a2, nl, logQ)))
    check(cases)


def test_floor_division_of_the_scaled_constant(check):
    """floor(cv 2^logQ / p) modulo 2^(64 M), M the class of nl + 2 as launch_ct_add_const chooses it: negative constants with zero and with non-zero
    remainder, p = 2, 23 and just below 2^63, the extremes of a machine word"""
    rng, cases = random.Random(4), []
    lim = 1 << 63
    for nl in (1, 2, 3, 6, 7, 14, 15, 32):
        M = next(c for c in (4, 8, 16, 34) if c >= nl + 2)
        for logQ in logqs(nl):
            for p in (2, 23, lim - 25, rng.getrandbits(40) | 1):
                cvs = [0, 1, -1, -p, p, -p - 1 if p + 1 <= lim else -p + 1, -(p - 1), lim - 1, -lim, -2 * p if 2 * p <= lim else -3, rng.getrandbits(63), -rng.getrandbits(63)]
                for cv in cvs:
                    q = ((cv << logQ) // p) % (1 << (64 * M))
                    cases.append((f"quot {M} {logQ} {cv} {p}", [(q >> (64 * i)) & (W - 1) for i in range(M)]))
    check(cases)


def test_rounding_of_decrypt_and_the_residual(check):
    """P = 2 p zl + q (zl = z mod 2q), its quotient by 2q and |P mod 2q - q|.  2 p z + q is even (q = 2^logQ, logQ >= 1), so of the half-way
    points (2 p z + q) mod 2q in {0, q - 1, q, 2q - 1} a z reaches 0 and q, and q - 2 and 2q - 2 next to the odd ones; the residual step takes
    all four from a P given directly."""
    rng, cases = random.Random(5), []
    for i, M in enumerate((2, 9, 17, 32)):
        for nw in sorted({(2, 9, 17, 32)[i - 1] + 1 if i else 1, M}):
            for logQ in sorted({64 * nw - 1, 64 * (nw - 1), 64 * (nw - 1) + 1, 64 * (nw - 1) + 33} - {0}):
                q = 1 << logQ
                for p in (2, 23, 65537, (1 << 63) - 25):
                    zs = [0, 1, q - 1, q, 2 * q - 1, (1 << (64 * nw)) - 1, rng.getrandbits(64 * nw), rng.getrandbits(64 * nw)]
                    if p & 1:
                        zs += [((t - q) // 2 * pow(p, -1, q)) % q for t in (0, q - 2, q, 2 * q - 2)]
                    for z in zs:
                        T = 2 * p * (z % (2 * q)) + q
                        Pm = T % (2 * q)
                        want = [T >> (64 * nw), T >> (logQ + 1)] + [(T >> (64 * k)) & (W - 1) for k in range(nw)] + [(abs(Pm - q) >> (64 * k)) & (W - 1) for k in range(nw)]
                        cases.append((f"round {M} {nw} {logQ} {p} {limbs(z, nw)}", want))
                    if p & 1:
                        reached = {(2 * p * (z % (2 * q)) + q) % (2 * q) for z in zs[-4:]}
                        assert reached == {t % (2 * q) for t in (0, q - 2, q, 2 * q - 2)}
                for Pm in (0, q - 1, q, 2 * q - 1, rng.getrandbits(logQ + 1)):
                    # (bits of P above 2q are not the residual's: set, they must be ignored)
                    P = Pm | (rng.getrandbits(64 * nw) >> (logQ + 1) << (logQ + 1))
                    cases.append((f"resid {M} {nw} {logQ} {limbs(P, nw)}", [(abs(Pm - q) >> (64 * k)) & (W - 1) for k in range(nw)]))
    check(cases)
