"""GPU: prepared plaintext operands (fhesi_plain_*), fhesi_ct_plain_sum_dev and fhesi_ct_add_slots_dev.
Bit for bit against the composition of the calls that existed before them (embed, a copy of the operand, ct_mul_poly_dev and ct_add_dev per term,
ct_add_const_dev), through the scheme (decrypt = sum a o w + c modulo p, slot by slot), and the handle's life and refusals."""
import functools
import math
import re

import numpy as np
import pytest

import fhe_si_amd as F
import oracle_lib as O
import params as P
import slots_common as SC
from test_plain_sum_model import fold_period

pytestmark = pytest.mark.gpu

# (m, p, g, logQ, two-row)
RINGS = {
    "two_row_64": (64, 257, 5, 90, True),
    "two_row_4096": (4096, 65537, 3, 128, True),        # more than one block of j, the direct embed path
    "single_22": (22, 23, 7, 80, False),                # n = 10: less than one wave
    "single_50": (50, 101, 3, 100, False),              # a prime-power ring: two-term fold, Bluestein rows
}
NPOOL = 5


class Ring:
    """context, space, a pool of NPOOL random ciphertexts (with extreme coefficients), six weights in one handle, and the reference products
    pool[a] (*) w[b] of every pair, formed once by the existing calls"""

    def __init__(self, name):
        self.m, self.p, self.g, self.logQ, two = RINGS[name]
        self.ctx, _ = SC.context(self.m, self.logQ, self.p)
        self.space = F.SlotSpace.pow2(self.ctx, self.p, self.g) if two else F.SlotSpace(self.ctx, self.p, self.g)
        n = self.n = self.ctx.phim
        self.nl = (self.logQ + 63) // 64
        self.words = 2 * n * self.nl
        rng = np.random.default_rng(self.m)
        pool = P.rand_limbs(rng, (NPOOL, 2, n), self.nl, self.logQ)
        lo, hi = -(1 << (self.logQ - 1)), (1 << (self.logQ - 1)) - 1
        for ct in range(NPOOL):                           # some coefficients at both ends of the centred range
            for part in range(2):
                pool[ct, part, rng.integers(0, n, size=3)] = O.ints_to_limbs([lo], self.nl)[0]
                pool[ct, part, rng.integers(0, n, size=3)] = O.ints_to_limbs([hi], self.nl)[0]
        self.pool_host = pool
        self.pool = self.ctx.upload(pool)
        one = np.zeros(n, dtype=np.int64)
        one[n // 3] = self.p - 2                          # a single non-zero slot
        self.vals = np.stack([rng.integers(0, self.p, size=n), np.full(n, self.p - 1), np.zeros(n, dtype=np.int64), one,
                              rng.integers(-(1 << 40), 1 << 40, size=n), rng.integers(0, self.p, size=n)]).astype(np.int64)
        self.nw = self.vals.shape[0]
        self.plain = self.space.plain(self.vals)
        # every pair's product by the existing calls: embed, a copy of the operand, ct_mul_poly_dev
        polys = self.space.embed(self.vals)
        pairs = [(a, b) for a in range(NPOOL) for b in range(self.nw)]
        self.prod = self.ctx.alloc(len(pairs) * self.words * 8)
        self.ctx.ct_gather_dev(self.pool, [a for a, _ in pairs], self.words, self.prod)
        self.ctx.ct_mul_poly_dev(self.logQ, self.prod, 2, self.nl, len(pairs), np.stack([polys[b] for _, b in pairs]))
        self.pair = {ab: i for i, ab in enumerate(pairs)}

    def composed(self, a_idx, b_idx, seg):
        """sum per group by ct_add_dev on the products"""
        ng = len(seg) - 1
        acc = self.ctx.upload(np.zeros((ng, self.words), dtype=np.uint64))
        for g in range(ng):
            for t in range(seg[g], seg[g + 1]):
                self.ctx.ct_add_dev(self.logQ, SC.View(acc, g * self.words * 8), SC.View(self.prod, self.pair[(a_idx[t], b_idx[t])] * self.words * 8), 2, self.nl, 1)
        return acc.download((ng, self.words))

    def fused(self, a_idx, b_idx, seg, plain=None):
        ng = len(seg) - 1
        out = self.ctx.upload(np.full((ng, self.words), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        self.ctx.ct_plain_sum_dev(plain or self.plain, self.logQ, self.pool, NPOOL, self.nl, a_idx, b_idx, seg, out)
        return out.download((ng, self.words))


@functools.lru_cache(maxsize=None)
def ring(name):
    return Ring(name)


def segments(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


@pytest.mark.parametrize("name", list(RINGS))
def test_sum_equals_the_composition(name):
    """Segment lengths 0, 1, 2, F - 1, F, F + 1, 2 F + 1 in one call; ciphertexts shared between groups, weights between terms, a_idx repeating
    inside a segment (5 ciphertexts under up to 129 terms)."""
    r, Fp = ring(name), fold_period()
    seg = segments([0, 1, 2, Fp - 1, Fp, Fp + 1, 2 * Fp + 1])
    rng = np.random.default_rng(11)
    a_idx = [int(x) for x in rng.integers(0, NPOOL, size=seg[-1])]
    b_idx = [int(x) for x in rng.integers(0, r.nw, size=seg[-1])]
    b_idx[:6] = [1, 2, 3, 0, 4, 5]                         # every kind of weight early on: all p - 1, all 0, one slot, random
    want = r.composed(a_idx, b_idx, seg)
    got = r.fused(a_idx, b_idx, seg)
    assert not want[0].any() and want[1].any() and np.array_equal(got[0], want[0])            # the empty segment: the zero ciphertext
    for g in range(len(seg) - 1):
        assert np.array_equal(got[g], want[g]), (name, g, seg[g + 1] - seg[g])
    assert np.array_equal(r.fused(a_idx, b_idx, seg), got)                   # a second call on the same handle: the same bits
    # one group alone, and the same wave cut into passes of two ciphertexts / two groups (a group with more distinct ciphertexts is summed piecewise)
    g = 5
    assert np.array_equal(r.fused(a_idx[seg[g]:seg[g + 1]], b_idx[seg[g]:seg[g + 1]], [0, seg[g + 1] - seg[g]])[0], want[g])
    keep = r.ctx.get_option("wave_operands")
    r.ctx.set_option("wave_operands", 2)
    try:
        assert np.array_equal(r.fused(a_idx, b_idx, seg), want)
    finally:
        r.ctx.set_option("wave_operands", keep)


@pytest.mark.parametrize("name", list(RINGS))
def test_constructors_against_mul_poly(name):
    """A single product through each constructor equals fhesi_ct_mul_poly_dev with npoly = 1 on a copy of the operand."""
    r = ring(name)
    n, rng = r.n, np.random.default_rng(3)

    def by_mul_poly(poly):
        ct = r.ctx.upload(r.pool_host[2])
        r.ctx.ct_mul_poly_dev(r.logQ, ct, 2, r.nl, 1, poly)
        return ct.download((r.words,))

    signed = rng.integers(-(1 << 30), 1 << 30, size=(2, n)).astype(np.int64)
    w = r.ctx.plain_from_poly(signed)
    assert (w.nw, w.maxabs, w.p) == (2, int(np.abs(signed).max()), 0)
    assert np.array_equal(r.fused([2], [1], [0, 1], w)[0], by_mul_poly(signed[1]))
    w.close()
    assert (r.plain.nw, r.plain.maxabs, r.plain.p) == (r.nw, r.p - 1, r.p)
    vals = rng.integers(0, r.p, size=(1, n)).astype(np.int64)
    for only_usable in (True, False):
        w = r.space.plain(vals, only_usable=only_usable)
        assert np.array_equal(r.fused([2], [0], [0, 1], w)[0], by_mul_poly(r.space.embed(vals, only_usable=only_usable)[0])), only_usable
        w.close()
    few = vals[:, :max(1, n // 3)]                           # nvals < n: the other slots are zero
    w = r.space.plain(few)
    assert np.array_equal(r.fused([2], [0], [0, 1], w)[0], by_mul_poly(r.space.embed(few)[0]))
    w.close()


@pytest.mark.parametrize("name,nv_each", [("two_row_64", False), ("two_row_64", True), ("two_row_4096", False), ("two_row_4096", True)])
def test_through_the_scheme(name, nv_each):
    """decrypt(sum_t Enc(a_t) (*) w_t + c) = (sum_t a_t o w_t + c) mod p slot by slot, c added by ct_add_slots_dev (one constant for all groups,
    or one each).  logQ = 90 / 128 and T = 3 leave the composition's noise below 1e-17 of the rounding limit on these rings (an integer model
    of Encrypt, the per-term products and sums and Decrypt with keys of this shape, run on the CPU for T = 3 and T = 130)."""
    r = ring(name)
    ctx, n, p, logQ, nl = r.ctx, r.n, r.p, r.logQ, r.nl
    sk1, pk0, pk1 = SC.device_keys(ctx, logQ, 77)
    G, T = 3, 3
    rng = np.random.default_rng(21)
    data = rng.integers(0, p, size=(G * T, n)).astype(np.int64)
    enc = ctx.alloc(G * T * r.words * 8)
    r.space.encrypt_batch_seeded(pk0, pk1, logQ, 1234, 100, data, enc, nl)
    a_idx, seg = list(range(G * T)), segments([T] * G)
    b_idx = [int(x) for x in rng.integers(0, r.nw, size=G * T)]
    out = ctx.alloc(G * r.words * 8)
    ctx.ct_plain_sum_dev(r.plain, logQ, enc, G * T, nl, a_idx, b_idx, seg, out)
    c = rng.integers(0, p, size=(G if nv_each else 1, n)).astype(np.int64)
    twin = ctx.upload(out.download((G, r.words)))
    r.space.ct_add_slots_dev(logQ, out, 2, nl, G, c)
    ctx.ct_add_const_dev(logQ, p, twin, 2, nl, G, r.space.embed(c))
    assert np.array_equal(out.download((G, r.words)), twin.download((G, r.words)))       # ct_add_slots_dev = ct_add_const_dev(embed(c))
    got = r.space.decrypt_batch(sk1, logQ, out, nl, G)
    w = np.mod(r.vals, p)
    for g in range(G):
        want = (sum(data[t] * w[b_idx[t]] for t in range(seg[g], seg[g + 1])) + c[g if nv_each else 0]) % p
        assert np.array_equal(got[g], want), g


def test_handle_life_and_contexts():
    m, p, g, logQ, _ = RINGS["two_row_64"]
    lib = F.binding._load()
    ctx, _ = SC.context(m, logQ, p)
    space = F.SlotSpace.pow2(ctx, p, g)
    w = space.plain(np.arange(ctx.phim, dtype=np.int64))
    other, _ = SC.context(m, logQ, p)                       # made after the handle
    nl, words = (logQ + 63) // 64, 2 * ctx.phim * ((logQ + 63) // 64)
    pool = other.upload(P.rand_limbs(np.random.default_rng(1), (1, 2, other.phim), nl, logQ))
    out = other.alloc(words * 8)
    with pytest.raises(F.FhesiError, match="belongs to another context"):
        other.ct_plain_sum_dev(w, logQ, pool, 1, nl, [0], [0], [0, 1], out)
    # the handle counts as a live handle of its context, as the space does
    assert lib.fhesi_ctx_destroy(ctx.h) != 0 and "still alive" in lib.fhesi_last_error().decode()
    space.close()
    assert lib.fhesi_ctx_destroy(ctx.h) != 0 and "still alive" in lib.fhesi_last_error().decode()
    w.close()
    w.close()                                               # (closing twice is harmless)
    assert lib.fhesi_ctx_destroy(ctx.h) == 0
    ctx.h = None


def test_refusals_leave_the_context_usable():
    r = ring("two_row_64")
    ctx, n, nl, logQ = r.ctx, r.n, r.nl, r.logQ
    good = r.fused([1, 2], [0, 5], [0, 2])
    out = ctx.alloc(2 * r.words * 8)

    def refused(match, *args, plain=None, pool=None, out_=None):
        with pytest.raises(F.FhesiError, match=match):
            ctx.ct_plain_sum_dev(plain or r.plain, logQ, pool or r.pool, NPOOL, nl, *args, out_ or out)
        assert np.array_equal(r.fused([1, 2], [0, 5], [0, 2]), good)         # one small valid call after each refusal

    refused("ciphertext index 5 of term 1 out of range", [0, NPOOL], [0, 0], [0, 2])
    refused("ciphertext index -1 of term 0 out of range", [-1], [0], [0, 1])
    refused(f"plaintext index {r.nw} of term 0 out of range", [0], [r.nw], [0, 1])
    refused("seg is not non-decreasing", [0, 1], [0, 0], [0, 2, 1])
    refused("seg must start at 0", [0, 1], [0, 0], [1, 2])
    refused("out overlaps pool", [0], [0], [0, 1], out_=SC.View(r.pool, (NPOOL - 1) * r.words * 8))
    refused("out overlaps pool", [0], [0], [0, 1, 1], out_=SC.View(r.pool, -r.words * 8))       # (the range ends inside the pool; nothing is written)
    for bad in (np.zeros((1, n + 1), dtype=np.int64), np.zeros((1, 0), dtype=np.int64)):
        with pytest.raises(F.FhesiError, match=f"{bad.shape[1]} values per plaintext, the ring has {n} slots"):
            r.space.plain(bad)
        with pytest.raises(F.FhesiError, match=f"{bad.shape[1]} values per plaintext, the ring has {n} slots"):
            r.space.ct_add_slots_dev(logQ, out, 2, nl, 1, bad)
        assert np.array_equal(r.fused([1, 2], [0, 5], [0, 2]), good)
    with pytest.raises(F.FhesiError, match="2 constants for 3 ciphertexts"):
        r.space.ct_add_slots_dev(logQ, out, 2, nl, 3, np.zeros((2, n), dtype=np.int64))
    assert np.array_equal(r.fused([1, 2], [0, 5], [0, 2]), good)


def test_a_chain_too_short_for_the_sum_is_refused_on_the_host():
    """Two 60-bit primes hold one product on (64, 257, logQ 90) -- 103 bits -- but not a sum of 2^20 of them -- 123 bits.  The segment claims
    that length over one repeated pair, so nothing but the host checks runs."""
    m, p, g, logQ, _ = RINGS["two_row_64"]
    primes, roots = P.first_primes(m, 2)
    ctx = F.Context(m, primes, roots)
    space = F.SlotSpace.pow2(ctx, p, g)
    n, nl = ctx.phim, (logQ + 63) // 64
    w = space.plain(np.arange(n, dtype=np.int64))
    pool = ctx.upload(P.rand_limbs(np.random.default_rng(2), (1, 2, n), nl, logQ))
    out = ctx.alloc(2 * n * nl * 8)
    T = 1 << 20
    zeros = np.zeros(T, dtype=np.int32)
    with pytest.raises(F.FhesiError) as e:
        ctx.ct_plain_sum_dev(w, logQ, pool, 1, nl, zeros, zeros, [0, T], out)
    found = re.search(r"a sum of 1048576 products needs (\d+) bits, the chain holds (\d+)", str(e.value))
    assert found, str(e.value)
    assert int(found.group(1)) == math.ceil(F.plain_sum_bits(m, logQ, p - 1, T)) == 123
    assert int(found.group(2)) == math.floor(sum(math.log2(q) for q in primes))         # (two primes just below 2^60: 120 in double precision)
    assert math.ceil(F.plain_sum_bits(m, logQ, p - 1, 1)) == 103
    ctx.ct_plain_sum_dev(w, logQ, pool, 1, nl, [0], [0], [0, 1], out)          # one product fits, and the context works
    ref = ctx.upload(pool.download((2 * n * nl,)))
    ctx.ct_mul_poly_dev(logQ, ref, 2, nl, 1, space.embed(np.arange(n, dtype=np.int64)))
    assert np.array_equal(out.download((2 * n * nl,)), ref.download((2 * n * nl,)))
