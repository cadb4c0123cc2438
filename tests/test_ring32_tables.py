"""CPU (no GPU): the host tables of the 30-bit rows as the library's own builders make them (fhe-si_amd/csrc/ring32_tables.h: ring32_build for
the transform tables of kernels_aux32.hip and kernels_tensor32.hip, conv32_build for the tensor half's conversion tables), printed by the
stand-alone program tests/host/ring32_tables_dump.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, against a model in Python's
integers written from the definitions:

  * table entry idx of the n-point transform (n = 2^(14 + S)) = psi^brv(idx) with floor(w 2^32 / p), psi = g^((p - 1) / 2n) for the smallest
    g in 2 .. 999 that gives an element of order 2n; forward entries as (-w mod 2^32, floor(w 2^32 / p));
  * sub-block h of 2^S: own entry m' + i' (m' = 1, 2, .., 2^13; i' < m') is entry (m' << S) + h m' + i' of the row's table;
  * the regions [1024 << v, 2048 << v), v = 0 .. 3, of every block of 2^14 in the order the waves load them:
    pair (t, q) of stage v  ->  pair ((t >> 6) 2^v + q) 64 + (t & 63);
  * entries 0 and 1 of every inverse block: 1 / 2^14 and (entry 1) / 2^14;  ht (S = 2), hs (S >= 3);
  * M / p_i in words of R bits and 2^(R WT) - M; (M / p_i)^-1 with its 1/2 and psi^-brv(1) / 2 variants; floor(2^57 / p); the rows of the
    big integer -> residue conversion with their two's complement entry; the closing pair of rows of 2^14.

Shapes: the smallest that reach every branch -- S = 0, 1, 2, 3 with the two largest primes below 2^30 that are 1 mod 2^(15 + S); S = 0 with the
two largest below 2^29 (option tensor_bits = 29); the conversion tables of the two compiled shapes (28-bit words x 38 with 35 primes, 26-bit
words x 82 with 70 primes on rows of 2^15) and of the run-time form (28-bit words, the row length from the bit count) at S = 0 and S = 2."""
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

import fhesi_pyref as R
import test_arith32_models as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
LOGN, N, HT = 14, 1 << 14, 8


def brv(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def root_2n(p, n):
    for g in range(2, 1000):
        c = pow(g, (p - 1) // (2 * n), p)
        if pow(c, n, p) == p - 1:
            return c
    raise AssertionError("no 2n-th root")


def tw(w, p):
    return (w, (w << 32) // p)


def aux_rule(S, bits=30):
    """the largest primes below 2^bits that are 1 mod 2n, n = 2^(14 + S)"""
    return (A.primes_below_2_30 if bits == 30 else A.primes_below_2_29)(2, 1 << (LOGN + S + 1))


class RingModel:
    """one prime: the full table of the n-point transform, forward and inverse, and what is cut from it"""

    def __init__(self, p, S):
        self.p, self.S = p, S
        lg = LOGN + S
        n = 1 << lg
        self.psi = root_2n(p, n)
        ipsi = pow(self.psi, -1, p)
        assert pow(self.psi, 2 * n, p) == 1 and pow(self.psi, n, p) == p - 1
        rev = [brv(e, lg) for e in range(n)]
        self.ff, self.fi = [0] * n, [0] * n
        w = v = 1
        for e in range(n):                                    # entry brv(e) = psi^e
            self.ff[rev[e]], self.fi[rev[e]] = w, v
            w, v = w * self.psi % p, v * ipsi % p
        self.ninv = pow(N, -1, p)

    def pw(self, idx, inverse=False):
        return pow(self.psi, (-1 if inverse else 1) * brv(idx, LOGN + self.S), self.p)

    def block(self, h, inverse):
        """sub-block h as [2^14][2] numpy words, scaled entries in, before the re-ordering of the last four stages"""
        S, p = self.S, self.p
        full = self.fi if inverse else self.ff
        w = [0] * N
        m = 1
        while m < N:
            for i in range(m):
                w[m + i] = full[(m << S) + h * m + i]
            m <<= 1
        if not S:
            w[0] = full[0]
        if inverse:
            w[0], w[1] = self.ninv, w[1] * self.ninv % p
        rows = [(x if inverse else (-x) % (1 << 32), (x << 32) // p) for x in w]
        if S and not inverse:
            rows[0] = (0, 0)                                  # (a sub-block's forward entry 0 is never read: zero)
        return np.array(rows, dtype=np.uint64)

    def last(self, h):
        return self.fi[(1 << self.S) + h]


def load_order(blk):
    """the regions of the last four stages: pair (t, q) of stage v -> pair ((t >> 6) 2^v + q) 64 + (t & 63); a pair is two entries"""
    out = blk.copy()
    for v in range(4):
        off, nq = 1024 << v, 1 << v
        reg = blk[off:2 * off].reshape(8, 64, nq, 2, 2)       # [t >> 6][t & 63][q][entry of the pair][word]
        out[off:2 * off] = reg.transpose(0, 2, 1, 3, 4).reshape(off, 2)
    return out


def test_load_order_follows_the_stated_rule():
    """the numpy transposition above against the rule itself, pair by pair, on a block of distinct numbers"""
    blk = np.arange(2 * N, dtype=np.uint64).reshape(N, 2)
    got = load_order(blk)
    for v in range(4):
        off, nq = 1024 << v, 1 << v
        for t in (0, 1, 63, 64, 65, 300, 511):
            for q in range(nq):
                src, dst = t * nq + q, ((t >> 6) * nq + q) * 64 + (t & 63)
                assert np.array_equal(got[off + 2 * dst:off + 2 * dst + 2], blk[off + 2 * src:off + 2 * src + 2])
    assert np.array_equal(got[:1024], blk[:1024])


def sha_le(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype="<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def dump():
    subprocess.check_call(["make", "-C", HOST, "ring32_tables_dump"], stdout=subprocess.DEVNULL)

    def run(*args):
        r = subprocess.run([os.path.join(HOST, "ring32_tables_dump")] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            f = line.split()
            if f[1] == ":":                                   # "sizes : ..."
                out[f[0]] = [int(v) for v in f[2:]]
            elif f[2] == ":":                                 # "name index : hex words"
                out[f[0], int(f[1])] = [int(v, 16) for v in f[3:]]
            else:                                             # "name prime length sha256"
                out[f[0], int(f[1])] = (int(f[2]), f[3])
        return out
    return run


@pytest.mark.parametrize("S,bits", [(0, 30), (1, 30), (2, 30), (3, 30), (0, 29)])
def test_transform_tables(dump, S, bits):
    primes = aux_rule(S, bits)
    assert len(primes) == 2 and all(p < 1 << bits and p % (1 << (LOGN + S + 1)) == 1 and R.is_prime(p) for p in primes)
    got = dump("ring", S, *primes)
    NS, HSN = 1 << S, (1 << S) + 4
    per = N << S
    assert got["sizes"] == [2 * per, 2 * per, 2 * HT, 2 * 2 * HSN if S >= 3 else 0]
    flat = lambda pairs: [x for pr in pairs for x in pr]
    for a, p in enumerate(primes):
        m = RingModel(p, S)
        inv2 = (p + 1) // 2
        assert inv2 * 2 % p == 1
        # the per-prime values the two users derive their own constants from
        assert got["pp", a] == flat([tw(m.pw(1), p), tw(m.pw(2), p), tw(m.pw(3), p), tw(m.pw(1, True), p)])
        assert got["ninv", a] == [m.ninv] and m.ninv * N % p == 1
        assert got["last", a] == [m.last(h) for h in range(NS)]
        for h in range(NS):                                   # the last inverse stage of sub-block h: group h of stage S + 13 ... its own entry 1
            assert m.last(h) == m.pw((1 << S) + h, True)
        ht = [(0, 0)] * HT
        if S == 2:
            ht = [tw(m.pw(1), p), tw(m.pw(2), p), tw(m.pw(3), p), (0, 0), tw(inv2, p), tw(m.pw(2, True) * inv2 % p, p), tw(m.pw(3, True) * inv2 % p, p),
                  tw(m.pw(1, True) * inv2 % p, p)]
        assert got["ht", a] == flat(ht)
        if S >= 3:
            c = pow(NS, -1, p)
            cm = c * (1 << 32) % p
            f = [(0, 0)] + [tw(m.pw(i), p) for i in range(1, NS)] + [(0, 0)] * 4
            b = [(0, 0)] + [tw(m.pw(i, True), p) for i in range(1, NS)] + [tw(c, p), tw(m.pw(1, True) * c % p, p), tw(cm, p), tw(m.pw(1, True) * cm % p, p)]
            assert got["hs", a] == flat(f + b)
        else:
            assert ("hs", a) not in got
        # the large tables: [2^S][2^14] pairs of this prime, hashed as little-endian words
        for name, inverse in (("fwd", False), ("inv", True)):
            blocks = np.concatenate([load_order(m.block(h, inverse)) for h in range(NS)])
            assert got[name, a] == (per, sha_le(blocks)), (name, a)


def tensor_rule(count, S, bits=30):
    return (A.primes_below_2_30 if bits == 30 else A.primes_below_2_29)(count, 1 << (LOGN + S + 1))


def generic_wt(primes):
    return int((sum(math.log2(p) for p in primes) + 8) / 28) + 2


CONV = [  # (S, R, WT or None: from the bit count, primes, limbs, lift)
    (0, 28, 38, 35, 8, 257),
    (1, 26, 82, 70, 16, (1 << 30) + 3),
    (0, 28, None, 9, 2, 23),
    (2, 28, None, 9, 2, 23),
]


@pytest.mark.parametrize("S,Rw,WT,NP,nl,lift", CONV)
def test_conversion_tables(dump, S, Rw, WT, NP, nl, lift):
    primes = tensor_rule(NP, S)
    WT = WT or generic_wt(primes)
    got = dump("conv", S, Rw, WT, nl, lift, *primes)
    stride = (2 * nl + 8 + 7) & ~7
    assert got["sizes"] == [stride, 2 * NP * stride, 2 * NP, NP, (NP + 1) * WT + 64]
    M = math.prod(primes)
    assert M < 1 << (Rw * WT)
    word = lambda v, l: (v >> (Rw * l)) & ((1 << Rw) - 1)
    n = 1 << (LOGN + S)
    for a, p in enumerate(primes):
        psi = root_2n(p, n)
        pw = lambda idx, sign=1: pow(psi, sign * brv(idx, LOGN + S), p)
        sh = 29 if p >> 29 else 28
        mu61 = (1 << (32 + sh)) // p
        head = [0, 0, 0, 0]
        if S == 1:
            head = list(tw(pw(1), p)) + [0, 0]
        if S == 2:
            head = list(tw(pw(2), p)) + list(tw(pw(3), p))
        for cls, s in ((0, lift), (1, 1)):
            row = [s * (1 << (32 * k)) % p for k in range(2 * nl)]
            row += [(-s * (1 << (64 * nl))) % p, (1 << 32) % p, mu61, p] + head
            assert got["rns%d" % cls, a] == row + [0] * (stride - len(row)), (cls, a)
        Mi = M // p
        ci = pow(Mi % p, -1, p)
        inv2, ninv = (p + 1) // 2, pow(N, -1, p)
        if S == 1:
            cinv = list(tw(ci * inv2 % p, p)) + list(tw(ci * pw(1, -1) * inv2 % p, p))
        else:
            cinv = list(tw(ci, p)) * 2
        assert got["cinv", a] == cinv
        if S == 0:                                            # rows of 2^14 leave the inverse as x (M / p_i)^-1: the closing pair carries it
            cn = ci * ninv % p
            closing = list(tw(cn, p)) + list(tw(cn * pw(1, -1) % p, p))
        else:
            closing = list(tw(ninv, p)) + [0, 0]
        assert got["consts", a] == [(1 << 57) // p, mu61]
        assert got["closing", a] == closing
        assert got["Mw", a] == [word(Mi, l) for l in range(WT)]
    Nn = ((1 << (Rw * WT)) - M) % (1 << (Rw * WT))
    assert got["Mw", NP] == [word(Nn, l) for l in range(WT)]
    assert got["pad", 0] == [0] * 64
