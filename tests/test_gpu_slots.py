"""GPU: plaintext slot packing on the device (fhesi_slots_*, the slot-valued Encrypt / Decrypt, the noise masks) through the C ABI against the
model of tests/slots_model.py, which evaluates at roots and interpolates from the definition.  Exact."""
import functools
import json
import os

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
import slots_model as M
from slots_common import I, make, rand_pk

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P31 = (1 << 31) - 1        # a 31-bit prime = 1 mod 22: 22 p^2 is above 2^59, which forces the two-prime convolution


make = functools.partial(make, F.SlotSpace, M)


@pytest.mark.parametrize("m,p,g", [(4, 5, 3), (9, 19, 2), (50, 101, 3), (22, 23, 7), (22, 67, 7), (2026, 2027, 3), (22, P31, 7)])
def test_embed_and_decode_against_the_model(m, p, g):
    ctx, S, mod = make(m, p, g)
    assert (S.total, S.usable, S.rho0) == (mod.total, mod.usable, mod.rho0)
    assert I(S.exponents()) == mod.exps
    assert S.aux_primes == (2 if p == P31 else 1)
    n = S.total
    rng = np.random.default_rng(m * 31 + p % 1000)
    for count in (1, 3):
        for nvals in sorted({1, S.usable, n}):
            for only_usable in (True, False):
                vals = rng.integers(0, p, size=(count, nvals)).astype(np.int64)
                vals[0, 0] = p - 1
                msg = S.embed(vals, only_usable)
                assert msg.shape == (count, n) and msg.min() >= 0 and msg.max() < p
                for c in range(count if m < 1000 else 1):
                    assert I(msg[c]) == M.embed_slots(mod, I(vals[c]), only_usable), (count, nvals, only_usable, c)
                coef = rng.integers(0, p, size=(count, n)).astype(np.int64)
                got = S.decode(coef, nvals, only_usable)
                for c in range(count if m < 1000 else 1):
                    assert I(got[c]) == M.decode_slots(mod, I(coef[c]), nvals, only_usable), (count, nvals, only_usable, c)
    # negative and unreduced values are taken modulo p
    vals = rng.integers(-(1 << 62), 1 << 62, size=(2, n)).astype(np.int64)
    assert np.array_equal(S.embed(vals, False), S.embed(vals % p, False))
    assert np.array_equal(S.decode(vals, n, False), S.decode(vals % p, n, False))
    with pytest.raises(F.FhesiError):
        S.embed(np.zeros((1, n + 1), dtype=np.int64))


@pytest.mark.parametrize("m,p", [(8422, 8423), (32602, 32603), (65542, 65543)])
def test_large_rings_round_trip_and_sampled_slots(m, p):
    g = M.least_generator(m)
    ctx, S, mod = make(m, p, g)
    assert (S.total, S.usable, S.rho0, S.aux_primes) == (mod.total, mod.usable, mod.rho0, 1)
    n, count = S.total, 3
    rng = np.random.default_rng(m)
    vals = rng.integers(0, p, size=(count, n)).astype(np.int64)
    msg = S.embed(vals, False)
    assert msg.min() >= 0 and msg.max() < p
    assert np.array_equal(S.decode(msg, n, False), vals)
    for j in (0, 1, S.usable - 1, n - 1):          # the polynomial the device produced has the asked values at the model's roots
        assert M.decode_slot(mod, I(msg[1]), j) == vals[1, j]
    coef = rng.integers(0, p, size=(count, n)).astype(np.int64)
    got = S.decode(coef, n, True)
    assert not got[:, S.usable:].any()
    for j in (0, 2, S.usable - 1):
        assert M.decode_slot(mod, I(coef[2]), j) == got[2, j]
    assert np.array_equal(S.embed(got[:, :S.usable], True), S.embed(S.decode(coef, S.usable, True), True))
    # Embed is linear
    a, b = vals[0:1], vals[1:2]
    assert np.array_equal(S.embed((a + b) % p, False), (S.embed(a, False) + S.embed(b, False)) % p)


@pytest.mark.parametrize("m,p,g,logQ", [(50, 101, 3, 90), (2026, 2027, 3, 128), (22, P31, 7, 100)])
def test_device_forms_and_fused_encrypt_decrypt(m, p, g, logQ):
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace(ctx, p, g)
    n, nl, count = S.total, (logQ + 63) // 64, 5
    rng = np.random.default_rng(m + 7)
    for nvals, only_usable in ((S.usable, True), (n, False), (3 if n >= 3 else 1, True)):
        vals = rng.integers(0, p, size=(count, nvals)).astype(np.int64)
        msg = S.embed(vals, only_usable)
        # _dev forms
        d_vals, d_msg = ctx.upload(vals), ctx.alloc(count * n * 8)
        S.embed_dev(d_vals, nvals, count, d_msg, only_usable)
        assert np.array_equal(d_msg.download((count, n), np.int64), msg)
        d_back = ctx.alloc(count * nvals * 8)
        S.decode_dev(d_msg, count, nvals, d_back, only_usable)
        assert np.array_equal(d_back.download((count, nvals), np.int64), S.decode(msg, nvals, only_usable))
        # fused encrypt = embed, then encrypt, bit for bit under the same (seed, index)
        pk0, pk1 = rand_pk(ctx, primes, rng)
        a, b = ctx.alloc(count * 2 * n * nl * 8), ctx.alloc(count * 2 * n * nl * 8)
        S.encrypt_batch_seeded(pk0, pk1, logQ, 0x1234, 77, vals, a, nl, only_usable)
        ctx.encrypt_batch_seeded(pk0, pk1, logQ, p, 0x1234, 77, msg, b, nl)
        assert np.array_equal(a.download((count, 2, n, nl)), b.download((count, 2, n, nl)))
        # fused decrypt = decrypt, then decode (any ciphertext, any key rows)
        cts = ctx.upload(P.rand_limbs(rng, (count, 2, n), nl, logQ))
        plain = ctx.decrypt_batch(pk1, logQ, p, cts, nl, count)
        assert np.array_equal(S.decrypt_batch(pk1, logQ, cts, nl, count, nvals, only_usable), S.decode(plain, nvals, only_usable))


def model_keys(m, logQ, p, seed):
    primes, roots = P.chain_for(m, logQ, p)
    rctx = R.Ctx(m, logQ, p, primes, roots)
    ctx = F.Context(m, primes, roots)
    prng = R.SplitMix64(seed)
    t, pk = R.keygen(rctx, prng)
    nl = (logQ + 63) // 64
    pk0 = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs(pk[0], nl))
    pk1 = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs(pk[1], nl))
    sk1 = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs(t, 1))
    return rctx, ctx, prng, t, pk0, pk1, sk1


@pytest.mark.parametrize("m,p,g,logQ", [(22, 23, 7, 80), (50, 101, 3, 100)])
def test_products_sums_and_noise_through_the_scheme(m, p, g, logQ):
    rctx, ctx, prng, t, pk0, pk1, sk1 = model_keys(m, logQ, p, 5 + m)
    S, mod = F.SlotSpace(ctx, p, g), M.slot_space(m, p, g)
    n, nl, nd, L = S.total, (logQ + 63) // 64, R.ndigits(logQ), len(rctx.primes)
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(1, n)).astype(np.int64)
    b = rng.integers(0, p, size=(1, n)).astype(np.int64)
    ca, cb = ctx.alloc(2 * n * nl * 8), ctx.alloc(2 * n * nl * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, a, ca, nl, False)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 1, b, cb, nl, False)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, ca, nl, 1, n, False), a)
    # Dec(Enc(a) * Enc(b)) decodes to a o b
    ksm = R.key_switch_init_s2(rctx, t, prng)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(np.array([[[I(d[i]) for i in range(L)] for d in ksm[r]] for r in range(2)], dtype=np.uint64))
    prod = ctx.alloc(2 * n * nl * 8)
    ctx.ct_mul_relin_dev(ksk, logQ, p, ca, cb, prod, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, prod, nl, 1, n, False), a * b % p)
    # Dec(Enc(a) + Enc(b)) to a + b
    ctx.ct_add_dev(logQ, ca, cb, 2, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, ca, nl, 1, n, False), (a + b) % p)
    # noise masks: slot 0 is 0, the rest is the model's draw; the fused form equals the explicit one bit for bit
    count = 3
    masks = ctx.alloc(count * 2 * n * nl * 8)
    S.encrypt_noise_batch_seeded(pk0, pk1, logQ, 4242, 10, count, masks, nl)
    want = np.array([M.draw_noise_slots(mod, 4242, 10 + i) for i in range(count)], dtype=np.int64)
    assert not want[:, 0].any() and want[:, 1:].any() and want.max() < p
    assert np.array_equal(S.decrypt_batch(sk1, logQ, masks, nl, count, n, False), want)
    explicit = ctx.alloc(count * 2 * n * nl * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 4242, 10, want, explicit, nl, False)
    assert np.array_equal(masks.download((count, 2, n, nl)), explicit.download((count, 2, n, nl)))
    # a mask added to a ciphertext leaves slot 0 alone and shifts the others by the drawn values
    one = ctx.alloc(2 * n * nl * 8)
    ctx.dev_copy(one.ptr.value, masks.ptr.value, 2 * n * nl * 8)
    ctx.ct_add_dev(logQ, cb, one, 2, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, cb, nl, 1, n, False), (b + want[0:1]) % p)


def test_rotations_and_sum_batched_data_with_the_fixture_keys():
    """Ciphertext >>= g^t plus the automorphism key switch rotates the slots LEFT by t; SumBatchedData leaves the sum of the usable slots in
    slot 0 (keys, ciphertexts and the k sequence of tests/golden/regression.json, m = 22, p = 23, g = 7)."""
    c = json.load(open(os.path.join(G, "regression.json")))["ct_algebra"][0]
    m, logQ, p, g = c["m"], c["logQ"], c["p"], c["g"]
    primes, roots = I(c["primes"]), I(c["roots"])
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace(ctx, p, g)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    sk1 = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs(I(c["t"]), 1))
    ct = ctx.upload(np.stack([O.ints_to_limbs(I(x), nl) for x in c["c2"]]))
    before = S.decrypt_batch(sk1, logQ, ct, nl, 1, n, False)[0]
    assert I(before) == I(S.decode(np.array([c["m2"]], dtype=np.int64), n, False)[0])
    ks = c["ks"]           # g, g^2, g^4 modulo m
    ksks = [F.KeySwitchMatrix(ctx, 2, nd).upload(np.array([[[I(row) for row in col] for col in a[r]] for r in range(2)], dtype=np.uint64))
            for a in c["auto_ksm"]]
    out = ctx.alloc(2 * n * nl * 8)
    for i, (ksk, k) in enumerate(zip(ksks, ks)):
        ctx.ct_automorph_key_switch_dev(ksk, logQ, k, ct, nl, 1, out, nl)
        t = 1 << i
        assert I(S.decrypt_batch(sk1, logQ, out, nl, 1, n, False)[0]) == I(np.roll(before, -t)), t
    cur = ctx.upload(np.stack([O.ints_to_limbs(I(x), nl) for x in c["c2"]]))
    for ksk, k in zip(ksks, ks):
        ctx.ct_automorph_key_switch_dev(ksk, logQ, k, cur, nl, 1, out, nl)
        ctx.ct_add_dev(logQ, cur, out, 2, nl, 1)
    assert int(S.decrypt_batch(sk1, logQ, cur, nl, 1, 1)[0, 0]) == int(before[:S.usable].sum() % p)


@pytest.mark.parametrize("m,p,g,word", [(1 << 15, 23, 3, "ord_m(p) > 1"), (16, 17, 3, "not cyclic"), (22, 23, 3, "generator"),
                                        (22, 4294967311, 7, "2^32"), (22, 45, 7, "not prime")])
def test_refused_rings_name_the_condition_and_leave_the_context_working(m, p, g, word):
    logQ = 80
    primes, roots = P.chain_for(m, logQ, 23)
    ctx = F.Context(m, primes, roots)
    with pytest.raises(F.FhesiError) as e:
        F.SlotSpace(ctx, p, g)
    assert word in str(e.value), str(e.value)
    # the context still multiplies polynomials correctly
    orc = O.Oracle(m, primes, roots)
    n = ctx.phim
    rng = np.random.default_rng(m)
    x = O.ints_to_limbs(I(rng.integers(-50, 50, size=n)), 1)
    d = F.DoubleCRT.from_poly(ctx, x)
    assert np.array_equal(np.array(d.rows(), dtype=np.uint64), orc.dcrt_from_poly(x))
