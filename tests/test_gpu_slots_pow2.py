"""GPU: the two-row slot spaces of the power-of-two rings (fhesi_slots_create_pow2: the direct negacyclic transform modulo p in LDS, the
chirp where the plan picks it) through the C ABI against the model of tests/slots_pow2_model.py, which evaluates at roots and interpolates
from the definition.  Exact."""
import functools
import json
import os

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
import slots_pow2_model as M2
from slots_common import I, device_keys, make, rand_pk

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P31 = 2147473409           # 1 mod 2^10, just below 2^31: lazy values reach 2^32 - 2^15 on the direct path
P32 = 2147493889           # 1 mod 2^10, just above 2^31: chirp, and m p^2 > 2^59 takes two auxiliary primes


make = functools.partial(make, F.SlotSpace.pow2, M2)


@pytest.mark.parametrize("m,p,g", [(8, 17, 3), (16, 17, 5), (32, 97, 3), (64, 257, 5), (128, 257, 3), (256, 7681, 5), (1024, 12289, 3), (1024, P31, 3), (16, P32, 3), (64, P32, 5)])
def test_embed_and_decode_against_the_model(m, p, g):
    ctx, S, mod = make(m, p, g)
    n = S.total
    assert (S.total, S.usable, S.rho0, S.rows, S.cols) == (n, n, mod.rho0, 2, n // 2) and n == m // 2
    assert I(S.exponents()) == mod.exps
    assert S.path == mod.path == (2 if p == P32 else 0)
    rng = np.random.default_rng(m * 31 + p % 1000)
    full = n <= 128
    for count in (1, 3):
        for nvals in sorted({1, 3, n // 2, n}):
            for only_usable in (True, False):
                vals = rng.integers(0, p, size=(count, nvals)).astype(np.int64)
                vals[0, 0] = p - 1
                msg = S.embed(vals, only_usable)
                assert msg.shape == (count, n) and msg.min() >= 0 and msg.max() < p
                for c in range(count if full else 1):
                    assert I(msg[c]) == M2.embed_slots(mod, I(vals[c])), (count, nvals, only_usable, c)
                coef = rng.integers(0, p, size=(count, n)).astype(np.int64)
                coef[0, :] = p - 1
                got = S.decode(coef, nvals, only_usable)
                for c in range(count if full else 1):
                    assert I(got[c]) == M2.decode_slots(mod, I(coef[c]), nvals), (count, nvals, only_usable, c)
    # negative and unreduced values are taken modulo p
    vals = rng.integers(-(1 << 62), 1 << 62, size=(2, n)).astype(np.int64)
    assert np.array_equal(S.embed(vals, False), S.embed(vals % p, False))
    assert np.array_equal(S.decode(vals, n, False), S.decode(vals % p, n, False))
    with pytest.raises(F.FhesiError):
        S.embed(np.zeros((1, n + 1), dtype=np.int64))


@pytest.mark.parametrize("m,p,g,path", [(4096, 65537, 3, 0), (1 << 15, 65537, 5, 0), (1 << 16, 65537, 3, 0), (1 << 17, 786433, 5, 1)])
def test_large_rings_round_trip_and_sampled_slots(m, p, g, path):
    ctx, S, mod = make(m, p, g)
    assert (S.total, S.rho0, S.rows, S.cols, S.path) == (m // 2, mod.rho0, 2, m // 4, path)
    assert I(S.exponents()) == mod.exps
    n, h, count = S.total, S.cols, 3
    rng = np.random.default_rng(m)
    vals = rng.integers(0, p, size=(count, n)).astype(np.int64)
    msg = S.embed(vals)
    assert msg.min() >= 0 and msg.max() < p
    assert np.array_equal(S.decode(msg), vals)
    for j in (0, 1, h - 1, h, h + 1, n - 1):          # the polynomial the device produced has the asked values at the model's roots
        assert M2.decode_slot(mod, I(msg[1]), j) == vals[1, j]
    coef = rng.integers(0, p, size=(count, n)).astype(np.int64)
    got = S.decode(coef)
    for j in (0, 2, h - 1, h, n - 1):
        assert M2.decode_slot(mod, I(coef[2]), j) == got[2, j]
    part = S.decode(coef, 5)
    assert np.array_equal(part, got[:, :5])
    few = S.embed(vals[:, :7])                             # the other slots are zero
    back = S.decode(few)
    assert np.array_equal(back[:, :7], vals[:, :7]) and not back[:, 7:].any()
    if m == 4096:
        assert I(few[0]) == M2.embed_slots(mod, I(vals[0, :7]))
    # Embed is linear
    a, b = vals[0:1], vals[1:2]
    assert np.array_equal(S.embed((a + b) % p), (S.embed(a) + S.embed(b)) % p)
    # the automorphisms on the coefficient side: X -> X^g rotates both rows left, X -> X^(m-1) swaps them
    assert I(S.decode(np.array([M2.automorph(mod, I(msg[0]), g)], dtype=np.int64))[0]) == M2.rotate_rows(mod, I(vals[0]), 1)
    assert I(S.decode(np.array([M2.automorph(mod, I(msg[0]), m - 1)], dtype=np.int64))[0]) == M2.swap_rows(mod, I(vals[0]))


def test_fixtures_on_the_device():
    for c in json.load(open(os.path.join(G, "slots_pow2.json")))["cases"]:
        ctx, S, mod = make(c["m"], c["p"], c["g"])
        assert I(S.embed(np.array([c["vals"]], dtype=np.int64))[0]) == c["msg"]
        assert I(S.decode(np.array([c["msg"]], dtype=np.int64))[0]) == c["vals"]


@pytest.mark.parametrize("m,p,g", [(64, 257, 5), (4096, 65537, 3), (1 << 16, 65537, 3), (1024, P31, 3)])
def test_direct_and_chirp_paths_agree_word_for_word(m, p, g):
    ctx, S, mod = make(m, p, g)
    n, count = S.total, 4
    rng = np.random.default_rng(m + 1)
    vals = rng.integers(0, p, size=(count, n)).astype(np.int64)
    coef = rng.integers(0, p, size=(count, n)).astype(np.int64)
    assert S.path == 0
    direct = (S.embed(vals), S.decode(coef), S.embed(vals[:, :5]), S.decode(coef, 9))
    S.set_path(1)
    assert S.path == (2 if p == P31 else 1)
    chirp = (S.embed(vals), S.decode(coef), S.embed(vals[:, :5]), S.decode(coef, 9))
    S.set_path(0)
    assert S.path == 0
    again = (S.embed(vals), S.decode(coef))
    for a, b in zip(direct, chirp):
        assert np.array_equal(a, b)
    assert np.array_equal(again[0], direct[0]) and np.array_equal(again[1], direct[1])


def test_the_direct_path_is_refused_where_the_plan_does_not_admit_it():
    ctx, S, mod = make(16, P32, 3)
    with pytest.raises(F.FhesiError) as e:
        S.set_path(0)
    assert "2^31" in str(e.value)
    vals = np.arange(8, dtype=np.int64)[None]
    assert np.array_equal(S.decode(S.embed(vals)), vals)
    prim, roots = P.chain_for(50, 64, 101)
    one_row = F.SlotSpace(F.Context(50, prim, roots), 101, 3)
    assert (one_row.rows, one_row.cols, one_row.path) == (1, 20, 1)
    with pytest.raises(F.FhesiError):
        one_row.set_path(0)


@pytest.mark.parametrize("m,p,g,logQ", [(64, 257, 5, 90), (4096, 65537, 3, 128), (16, P32, 3, 100)])
def test_device_forms_and_fused_encrypt_decrypt(m, p, g, logQ):
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    n, nl, count = S.total, (logQ + 63) // 64, 3
    rng = np.random.default_rng(m + 7)
    for nvals, only_usable in ((n, True), (n, False), (3, True)):
        vals = rng.integers(0, p, size=(count, nvals)).astype(np.int64)
        msg = S.embed(vals, only_usable)
        # _dev forms
        d_vals, d_msg = ctx.upload(vals), ctx.alloc(count * n * 8)
        S.embed_dev(d_vals, nvals, count, d_msg, only_usable)
        assert np.array_equal(d_msg.download((count, n), np.int64), msg)
        d_back = ctx.alloc(count * nvals * 8)
        S.decode_dev(d_msg, count, nvals, d_back, only_usable)
        assert np.array_equal(d_back.download((count, nvals), np.int64), vals)
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


def test_products_rotations_row_swap_total_sum_and_noise_through_the_scheme():
    m, logQ, p, g = 4096, 300, 65537, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S, mod = F.SlotSpace.pow2(ctx, p, g), M2.slot_space(m, p, g)
    n, h, nl, nd = S.total, S.cols, (logQ + 63) // 64, R.ndigits(logQ)
    seed, pub = 0xABCDEF12345, 0x5DEECE66D
    sk1, pk0, pk1 = device_keys(ctx, logQ, seed)
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
    ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([one, sk1, sk1.copy().op(sk1, F.OP_MUL)], sk1, logQ, seed, pub, 1000)
    ks = M2.total_sum_exponents(mod)
    assert len(ks) == 11 and ks[-1] == m - 1
    autos = [F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(k)], sk1, logQ, seed, pub, 2000 + 100 * i) for i, k in enumerate(ks)]
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(1, n)).astype(np.int64)
    b = rng.integers(0, p, size=(1, n)).astype(np.int64)
    words = 2 * n * nl
    ca, cb = ctx.alloc(words * 8), ctx.alloc(words * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, a, ca, nl)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 1, b, cb, nl)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, ca, nl, 1), a)
    # Dec(Enc(a) * Enc(b)) decodes to a o b
    prod = ctx.alloc(words * 8)
    ctx.ct_mul_relin_dev(ksk, logQ, p, ca, cb, prod, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, prod, nl, 1), a * b % p)
    # X -> X^g, X -> X^(g^2) rotate both rows left by 1, 2; X -> X^(m-1) swaps the rows
    out = ctx.alloc(words * 8)
    for i, t in ((0, 1), (1, 2)):
        ctx.ct_automorph_key_switch_dev(autos[i], logQ, ks[i], ca, nl, 1, out, nl)
        assert I(S.decrypt_batch(sk1, logQ, out, nl, 1)[0]) == M2.rotate_rows(mod, I(a[0]), t)
    ctx.ct_automorph_key_switch_dev(autos[-1], logQ, m - 1, ca, nl, 1, out, nl)
    assert I(S.decrypt_batch(sk1, logQ, out, nl, 1)[0]) == M2.swap_rows(mod, I(a[0]))
    # the total-sum walk leaves the sum of all n slots in every slot
    cur = ctx.alloc(words * 8)
    ctx.dev_copy(cur.ptr.value, ca.ptr.value, words * 8)
    for ksm, k in zip(autos, ks):
        ctx.ct_automorph_key_switch_dev(ksm, logQ, k, cur, nl, 1, out, nl)
        ctx.ct_add_dev(logQ, cur, out, 2, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, cur, nl, 1), np.full((1, n), int(a.sum() % p)))
    # noise masks: slot 0 is 0, the others uniform; the fused form equals the explicit one; a mask leaves slot 0 of a ciphertext alone
    count = 2
    masks = ctx.alloc(count * words * 8)
    S.encrypt_noise_batch_seeded(pk0, pk1, logQ, 4242, 10, count, masks, nl)
    drawn = S.decrypt_batch(sk1, logQ, masks, nl, count)
    assert not drawn[:, 0].any() and drawn.max() < p and len(set(I(drawn[0]))) > n // 2 and not np.array_equal(drawn[0], drawn[1])
    explicit = ctx.alloc(count * words * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 4242, 10, drawn, explicit, nl, False)
    assert np.array_equal(masks.download((count, 2, n, nl)), explicit.download((count, 2, n, nl)))
    ctx.ct_add_dev(logQ, cb, masks, 2, nl, 1)
    assert np.array_equal(S.decrypt_batch(sk1, logQ, cb, nl, 1), (b + drawn[0:1]) % p)


@pytest.mark.parametrize("m,p,g,word", [(16, 17, 7, "mod 8"), (16, 33, 3, "not prime"), (16, 4294967377, 3, "2^32"), (1 << 15, 23, 3, "ord_m(p) > 1"), (4, 5, 3, "k < 3"),
                                        (22, 23, 7, "power of two")])
def test_refused_rings_name_the_condition_and_leave_the_context_working(m, p, g, word):
    primes, roots = P.chain_for(m, 80, 23)
    ctx = F.Context(m, primes, roots)
    with pytest.raises(F.FhesiError) as e:
        F.SlotSpace.pow2(ctx, p, g)
    assert word in str(e.value), str(e.value)
    if m == 16:                        # ... and the single-generator constructor keeps refusing the ring, word for word
        with pytest.raises(F.FhesiError) as e:
            F.SlotSpace(ctx, 17, 3)
        assert "(Z/m)^* is not cyclic (m = 2^k, k >= 3): no single generator walks all slots" in str(e.value)
    orc = O.Oracle(m, primes, roots)
    n = ctx.phim
    x = O.ints_to_limbs(I(np.random.default_rng(m).integers(-50, 50, size=n)), 1)
    d = F.DoubleCRT.from_poly(ctx, x)
    assert np.array_equal(np.array(d.rows(), dtype=np.uint64), orc.dcrt_from_poly(x))
