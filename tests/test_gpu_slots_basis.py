"""GPU: integer slots over a basis of plaintext primes (fhesi_slots_basis_*: loader-side reduction of the limbs, the direct transform per
channel, mixed-radix recombination with the centred lift) through the C ABI against the model of tests/slots_basis_model.py, which is Python
integers from the definition; channel by channel against the single-prime two-row space word for word; and through the scheme on one key set.
Exact."""
import json
import os

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
import slots_basis_model as MB
import slots_pow2_model as M2
from slots_common import I, View, context, device_keys, rand_pk

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def signed_values(rng, half, shape):
    """Python ints uniform on [-half, half], the extremes included"""
    flat = [int.from_bytes(rng.bytes((half.bit_length() + 7) // 8 + 8), "little") % (2 * half + 1) - half for _ in range(int(np.prod(shape)))]
    flat[0], flat[-1] = half, -half
    if len(flat) > 3:
        flat[1], flat[2] = -1, 0
    out = np.empty(len(flat), dtype=object)
    out[:] = flat
    return out.reshape(shape)


BASES = [(16, [17], 3), (16, [97, 17], 5), (16, MB.plan(16, 130, 31, 3), 3), (64, [257, 193, 449, 577, 641], 5), (64, MB.plan(64, 460, 15, 3), 3),
         (4096, MB.plan(4096, 20, 31, 3), 3), (4096, MB.plan(4096, 120, 30, 5), 5), (4096, MB.plan(4096, 900, 31, 3), 3), (1 << 16, [65537, 786433], 3),
         (1 << 16, MB.plan(1 << 16, 140, 31, 5), 5)]


@pytest.mark.parametrize("m,primes,g", BASES, ids=[f"m{m}-k{len(p)}" for m, p, _ in BASES])
def test_embed_and_decode_against_the_model(m, primes, g):
    ctx, _ = context(m)
    B, mod = F.SlotBasis.pow2(ctx, primes, g), MB.SlotBasis(m, primes, g)
    n, k, L = B.total, B.k, B.limbs
    assert (B.k, B.primes, B.modulus, B.limbs, B.total, B.rows, B.cols) == (mod.k, mod.primes, mod.modulus, mod.limbs, n, 2, n // 2)
    half = (B.modulus - 1) // 2
    rng = np.random.default_rng(m + k)
    singles = [F.SlotSpace.pow2(ctx, p, g) for p in (primes if m > 64 else [])]
    for count, nvals in ((1, n), (3, n), (2, 3), (2, n // 2)):
        vals = signed_values(rng, half, (count, nvals))
        msg = B.embed(vals)
        assert msg.shape == (k, count, n) and msg.min() >= 0 and all(int(msg[c].max()) < primes[c] for c in range(k))
        for c in range(k):          # channel c is the two-row embedding of vals mod p_c: the model on small rings, the single-prime space word for word on large ones
            for i in range(count):
                if m <= 64:
                    assert I(msg[c, i]) == M2.embed_slots(mod.channel(c), [int(v) % primes[c] for v in vals[i]]), (count, nvals, c, i)
            if m > 64:
                red = np.array([[int(v) % primes[c] for v in row] for row in vals], dtype=np.int64)
                assert np.array_equal(msg[c], singles[c].embed(red, False)), (count, nvals, c)
        # L_in = L (least limbs the binding picks may be fewer) and L_in = 16 give the same words
        assert np.array_equal(B.embed(vals, L), msg) and np.array_equal(B.embed(vals, 16), msg)
        got = B.decode(msg, nvals)
        assert got.shape == (count, nvals) and [I(r) for r in got] == [I(r) for r in vals], (count, nvals)
        if m <= 64:
            assert I(got[0]) == MB.decode(mod, [I(msg[c, 0]) for c in range(k)], nvals)
    # plain int64 data is L_in = 1; values beyond (-P/2, P/2) are reduced modulo P and come back centred
    v64 = rng.integers(-(1 << 63), (1 << 63) - 1, size=(2, n), dtype=np.int64)
    v64[0, :2] = [-(1 << 63), (1 << 63) - 1]
    back = B.decode(B.embed(v64))
    assert [I(r) for r in back] == [[MB.centred(int(x), B.modulus) for x in row] for row in v64]
    # decode takes any int64 coefficients (reduced modulo p_c)
    coef = rng.integers(-(1 << 62), 1 << 62, size=(k, 2, n)).astype(np.int64)
    red = np.stack([coef[c] % primes[c] for c in range(k)])
    assert np.array_equal(B.decode(coef, raw=True), B.decode(red, raw=True))
    with pytest.raises(F.FhesiError):
        B.embed(np.zeros((1, n + 1), dtype=np.int64))
    with pytest.raises(F.FhesiError):
        B.embed(np.zeros((1, 2), dtype=np.int64), 17)


def test_one_prime_equals_the_single_prime_space_word_for_word():
    for m, p, g in [(16, 17, 3), (4096, 65537, 3), (1 << 16, 786433, 5), (1024, 2147473409, 3)]:
        ctx, _ = context(m)
        B, S = F.SlotBasis.pow2(ctx, [p], g), F.SlotSpace.pow2(ctx, p, g)
        n = S.total
        rng = np.random.default_rng(m)
        vals = rng.integers(-(1 << 62), 1 << 62, size=(3, n)).astype(np.int64)
        assert np.array_equal(B.embed(vals)[0], S.embed(vals, False))
        ch = B.channel(0)
        assert (ch.p, ch.total, ch.rho0, ch.rows, ch.path) == (p, n, S.rho0, 2, 0) and I(ch.exponents()) == I(S.exponents())
        assert np.array_equal(ch.embed(vals, False), S.embed(vals, False))
        coef = rng.integers(0, p, size=(3, n)).astype(np.int64)
        dec = S.decode(coef, n, False)
        assert [I(r) for r in B.decode(coef[None])] == [[MB.centred(int(x), p) for x in row] for row in dec]


def test_fixtures():
    for c in json.load(open(os.path.join(G, "slots_basis.json")))["cases"]:
        ctx, _ = context(c["m"])
        B = F.SlotBasis.pow2(ctx, c["primes"], c["g"])
        vals = np.array([[int(v) for v in c["vals"]]], dtype=object)
        assert (str(B.modulus), B.limbs) == (c["modulus"], c["limbs"])
        assert [I(r) for r in B.embed(vals)[:, 0]] == c["msg"]
        assert I(B.decode(np.array(c["msg"], dtype=np.int64)[:, None, :])[0]) == I(vals[0])


@pytest.mark.parametrize("m,primes,g,logQ", [(64, [257, 193, 449], 5, 90), (4096, MB.plan(4096, 100, 31, 3), 3, 128), (1 << 16, [65537, 786433], 3, 64)])
def test_device_forms_and_fused_encrypt_decrypt(m, primes, g, logQ):
    ctx, chain = context(m, logQ, max(primes))
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k, L, nl, count = B.total, B.k, B.limbs, (logQ + 63) // 64, 3
    half = (B.modulus - 1) // 2
    rng = np.random.default_rng(m + 11)
    pk0, pk1 = rand_pk(ctx, chain, rng)
    for nvals in (n, 5):
        vals = signed_values(rng, half, (count, nvals))
        msg = B.embed(vals)
        limbs = F.pack_limbs(vals, L)
        # _dev forms
        d_vals, d_msg, d_back = ctx.upload(limbs), ctx.alloc(k * count * n * 8), ctx.alloc(count * nvals * L * 8)
        B.embed_dev(d_vals, L, nvals, count, d_msg)
        assert np.array_equal(d_msg.download((k, count, n), np.int64), msg)
        B.decode_dev(d_msg, count, nvals, d_back)
        assert np.array_equal(d_back.download((count, nvals, L), np.int64), limbs)
        # the fused encryption, channel by channel, is the single-prime fused encryption of vals mod p_c under index first + c count, bit for bit
        words = count * 2 * n * nl
        out, ref = ctx.alloc(k * words * 8), ctx.alloc(words * 8)
        B.encrypt_batch_seeded(pk0, pk1, logQ, 0x1234, 77, vals, out, nl)
        got = out.download((k, count, 2, n, nl))
        for c in range(k):
            red = np.array([[int(v) % primes[c] for v in row] for row in vals], dtype=np.int64)
            B.channel(c).encrypt_batch_seeded(pk0, pk1, logQ, 0x1234, 77 + c * count, red, ref, nl, False)
            assert np.array_equal(got[c], ref.download((count, 2, n, nl))), (nvals, c)
        # the fused decryption = k decryptions, decode, recombine (any ciphertext, any key rows)
        raw = P.rand_limbs(rng, (k * count, 2, n), nl, logQ)
        cts = ctx.upload(raw)
        plain = np.stack([ctx.decrypt_batch(pk1, logQ, primes[c], ctx.upload(raw[c * count:(c + 1) * count]), nl, count) for c in range(k)])
        assert np.array_equal(B.decrypt_batch(pk1, logQ, cts, nl, count, nvals, raw=True), B.decode(plain, nvals, raw=True))


def test_big_integers_through_the_scheme_on_one_key_set():
    m, logQ, g = 4096, 300, 3
    primes = MB.plan(m, 100, 20, g)                 # six primes near 2^20: P > 2^101
    assert len(primes) == 6
    chain, roots = P.chain_for(m, logQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B, mod = F.SlotBasis.pow2(ctx, primes, g), M2.slot_space(m, primes[0], g)
    Pm, n, k, nl, nd = B.modulus, B.total, B.k, (logQ + 63) // 64, R.ndigits(logQ)
    seed, pub = 0xABCDEF12345, 0x5DEECE66D
    sk1, pk0, pk1 = device_keys(ctx, logQ, seed)                 # ONE key set for every channel
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
    ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([one, sk1, sk1.copy().op(sk1, F.OP_MUL)], sk1, logQ, seed, pub, 1000)
    ks = M2.total_sum_exponents(mod)
    autos = [F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(e)], sk1, logQ, seed, pub, 2000 + 100 * i) for i, e in enumerate(ks)]
    rng = np.random.default_rng(m)
    a = signed_values(rng, 1 << 48, (1, n))
    b = signed_values(rng, 1 << 50, (1, n))
    words = 2 * n * nl                                          # of one channel ciphertext
    ca, cb = ctx.alloc(k * words * 8), ctx.alloc(k * words * 8)
    B.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, a, ca, nl)
    B.encrypt_batch_seeded(pk0, pk1, logQ, 99, k, b, cb, nl)
    assert I(B.decrypt_batch(sk1, logQ, ca, nl, 1)[0]) == I(a[0])

    def per_channel(fn):
        for c in range(k):
            fn(c, primes[c], c * words * 8)

    # Dec(Enc(a) * Enc(b)) = a * b exactly, |a b| up to 2^98: channel by channel with that channel's p
    prod = ctx.alloc(k * words * 8)
    per_channel(lambda c, p, off: ctx.ct_mul_relin_dev(ksk, logQ, p, View(ca, off), View(cb, off), View(prod, off), nl, 1))
    exact = [int(x) * int(y) for x, y in zip(a[0], b[0])]
    assert max(abs(v) for v in exact) > 1 << 90 and max(abs(v) for v in exact) < Pm // 2
    assert I(B.decrypt_batch(sk1, logQ, prod, nl, 1)[0]) == exact
    # rotation and row swap of signed values
    out = ctx.alloc(k * words * 8)
    per_channel(lambda c, p, off: ctx.ct_automorph_key_switch_dev(autos[0], logQ, ks[0], View(ca, off), nl, 1, View(out, off), nl))
    assert I(B.decrypt_batch(sk1, logQ, out, nl, 1)[0]) == M2.rotate_rows(mod, I(a[0]), 1)
    per_channel(lambda c, p, off: ctx.ct_automorph_key_switch_dev(autos[-1], logQ, m - 1, View(ca, off), nl, 1, View(out, off), nl))
    assert I(B.decrypt_batch(sk1, logQ, out, nl, 1)[0]) == M2.swap_rows(mod, I(a[0]))
    # the total-sum walk: the exact sum of all n signed slots in every slot
    cur = ctx.alloc(k * words * 8)
    ctx.dev_copy(cur.ptr.value, ca.ptr.value, k * words * 8)
    for ksm, e in zip(autos, ks):
        per_channel(lambda c, p, off: ctx.ct_automorph_key_switch_dev(ksm, logQ, e, View(cur, off), nl, 1, View(out, off), nl))
        ctx.ct_add_dev(logQ, cur, out, 2, nl, k)
    assert I(B.decrypt_batch(sk1, logQ, cur, nl, 1)[0]) == [sum(I(a[0]))] * n
    # noise masks: slot 0 is 0 modulo P, the rest changes; channel c of mask i is the single-prime mask of index first + c count + i
    count = 2
    masks, ref = ctx.alloc(k * count * words * 8), ctx.alloc(count * words * 8)
    B.encrypt_noise_batch_seeded(pk0, pk1, logQ, 4242, 10, count, masks, nl)
    drawn = B.decrypt_batch(sk1, logQ, masks, nl, count)
    assert drawn[0, 0] == 0 and drawn[1, 0] == 0 and len(set(I(drawn[0]))) > n // 2 and I(drawn[0]) != I(drawn[1])
    got = masks.download((k, count, 2, n, nl))
    for c in range(k):
        B.channel(c).encrypt_noise_batch_seeded(pk0, pk1, logQ, 4242, 10 + c * count, count, ref, nl)
        assert np.array_equal(got[c], ref.download((count, 2, n, nl)))
    per_channel(lambda c, p, off: ctx.ct_add_dev(logQ, View(cb, off), View(masks, c * count * words * 8), 2, nl, 1))
    masked = I(B.decrypt_batch(sk1, logQ, cb, nl, 1)[0])
    assert masked == [MB.centred(int(x) + int(y), Pm) for x, y in zip(b[0], drawn[0])]
    assert masked[0] == int(b[0, 0]) and sum(x != int(y) for x, y in zip(masked, b[0])) > n - 8


@pytest.mark.parametrize("primes,g,word", [([17, 97, 17], 3, "twice"), ([17, 41], 3, "ord_m(p) > 1"), ([17, 33], 3, "not prime"), ([2147483777], 3, "2^31"), ([], 3, "at least one"),
                                           ([17, 97], 7, "mod 8")])
def test_refused_bases_name_the_condition_and_leave_the_context_working(primes, g, word):
    m = 16
    chain, roots = P.chain_for(m, 80, 23)
    ctx = F.Context(m, chain, roots)
    with pytest.raises(F.FhesiError) as e:
        F.SlotBasis.pow2(ctx, primes, g)
    assert word in str(e.value), str(e.value)
    orc = O.Oracle(m, chain, roots)
    x = O.ints_to_limbs(I(np.random.default_rng(m).integers(-50, 50, size=ctx.phim)), 1)
    assert np.array_equal(np.array(F.DoubleCRT.from_poly(ctx, x).rows(), dtype=np.uint64), orc.dcrt_from_poly(x))
    B = F.SlotBasis.pow2(ctx, [17, 97], 3)
    assert I(B.decode(B.embed(np.array([[-800, 824, 3]], dtype=np.int64)), 3)[0]) == [-800, 824, 3]
    del B


def test_a_basis_on_a_ring_above_the_direct_path_is_refused():
    m = 1 << 17
    chain, roots = P.chain_for(m, 64, 23)
    ctx = F.Context(m, chain, roots)
    with pytest.raises(F.FhesiError) as e:
        F.SlotBasis.pow2(ctx, [786433], 3)
    assert "above 2^16" in str(e.value)
