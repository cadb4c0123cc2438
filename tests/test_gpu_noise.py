"""GPU: the noise budget (fhesi_ct_noise_batch, fhesi_decrypt_noise_batch, fhesi_ct_noise_int_batch) against tests/noise_model.py: the exact
maximal decryption residual per ciphertext word for word, the budget, and the message of the fused call against fhesi_decrypt_batch's."""
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import noise_model as N
import oracle_lib as O
import params as P
from slots_common import View, device_keys

pytestmark = pytest.mark.gpu


def dcrt_from_rows(ctx, rows):
    d = F.DoubleCRT(ctx)
    for i in range(rows.shape[0]):
        d.set_row(i, np.ascontiguousarray(rows[i]))
    return d


@functools.lru_cache(maxsize=None)
def ring(m, logQ, p):
    """context, model context and a random key row set (parity does not need a valid key), shared by the tests of one ring"""
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    rctx = R.Ctx(m, logQ, p, list(primes), list(roots))
    t_rows = P.rand_rows(np.random.default_rng(m * 7 + logQ), primes, ctx.phim, 1)[0]
    return ctx, rctx, t_rows, dcrt_from_rows(ctx, t_rows), {i: [int(x) for x in t_rows[i]] for i in range(len(primes))}


def model_of(rctx, t_model, ct, nl):
    return N.noise(rctx, t_model, [O.limbs_to_ints(ct[0]), O.limbs_to_ints(ct[1])])


RINGS = [(22, 80, 23), (46, 90, 47), (101, 100, 607), (64, 64, 257), (4096, 511, 65537)] + [(64, lq, 257) for lq in (20, 63, 127, 128, 511, 512, 575, 576, 1024, 1100)]


@pytest.mark.parametrize("m,logQ,p", RINGS)
def test_bit_exact_against_the_model(m, logQ, p):
    ctx, rctx, t_rows, sk1, t_model = ring(m, logQ, p)
    n, nl, nw = ctx.phim, (logQ + 63) // 64, (logQ + 64) // 64
    count = 2 if m > 1000 else 3
    rng = np.random.default_rng(m + logQ)
    cts = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    cts[0, 0, 0] = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0]
    cts[0, 1, 0] = O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    buf = ctx.upload(cts)
    budget, maxres = ctx.noise_budget(sk1, logQ, p, buf, nl, count, maxres=True)
    msg, budget2, maxres2 = ctx.decrypt_noise_batch(sk1, logQ, p, buf, nl, count, maxres=True)
    assert np.array_equal(msg, ctx.decrypt_batch(sk1, logQ, p, buf, nl, count))
    assert np.array_equal(budget, budget2) and maxres == maxres2
    assert np.array_equal(ctx.noise_budget(sk1, logQ, p, buf, nl, count), budget)          # (maxres_host null)
    for c in range(count):
        emsg, emax, ebudget = model_of(rctx, t_model, cts[c], nl)
        print(f"m={m} logQ={logQ} ct {c}: maxres bits {maxres[c].bit_length()} (model {emax.bit_length()}), budget {budget[c]} (model {ebudget})")
        assert N.words_of(maxres[c], nw) == N.words_of(emax, nw), c
        assert int(budget[c]) == ebudget, c
        assert [int(v) for v in msg[c]] == emsg, c


def crafted_batch(n, logQ, p, wave_lanes):
    """-> [(residuals per coefficient, what the case is)]: every residual even, reached by (c0, 0) under any key"""
    q = 1 << logQ
    rng = np.random.default_rng(n + logQ)
    small = lambda: [2 * int(x) for x in rng.integers(-(1 << 40), 1 << 40, size=n)]
    big = (q >> 1) + 2 * int(rng.integers(1 << 40))                     # (top words set, word 0 arbitrary)
    cases = []
    for pos in [0, n - 1] + wave_lanes:
        r = small()
        r[pos] = q - 2 - 2 * pos
        cases.append((r, f"maximum at coefficient {pos}"))
    r = small()
    r[1], r[n - 2] = big, -(big + 2)
    cases.append((r, "two coefficients differ only in word 0"))
    cases.append(([-big] * n, "all coefficients equal"))
    cases.append(([0] * (n - 1) + [-q], "|r| = q: budget 0"))
    cases.append(([0] * n, "r = 0: budget logQ"))
    for j in range(64, logQ, 64):
        cases.append(([(1 << j) - 2] * n, f"2^{j} - 2: budget logQ - {j}"))
        cases.append(([(1 << j) - 2] * (n // 2) + [-(1 << j)] + [(1 << j) - 2] * (n - n // 2 - 1), f"2^{j}: budget logQ - {j} - 1"))
    return cases


@pytest.mark.parametrize("m,logQ,p", [(64, 128, 257), (4096, 511, 65537)])
def test_crafted_residuals(m, logQ, p):
    ctx, rctx, t_rows, sk1, t_model = ring(m, logQ, p)
    n, nl, nw, q = ctx.phim, (logQ + 63) // 64, (logQ + 64) // 64, 1 << logQ
    lanes = [256 + 63, 256 + 127, 256 + 191, 256 + 255] if n > 512 else []      # the last lane of each wave of the second workgroup
    cases = crafted_batch(n, logQ, p, lanes)
    count = len(cases)
    cts = np.zeros((count, 2, n, nl), dtype=np.uint64)
    for c, (res, _) in enumerate(cases):
        cts[c, 0] = O.ints_to_limbs([N.crafted_c0(r, logQ, p) for r in res], nl)
    buf = ctx.upload(cts)
    msg, budget, maxres = ctx.decrypt_noise_batch(sk1, logQ, p, buf, nl, count, maxres=True)
    assert np.array_equal(msg, ctx.decrypt_batch(sk1, logQ, p, buf, nl, count))
    for c, (res, what) in enumerate(cases):
        emax = max(abs(r) for r in res)
        assert maxres[c] == emax and int(budget[c]) == N.budget_of(emax, logQ), what
    by = {what: int(budget[c]) for c, (_, what) in enumerate(cases)}
    assert by["|r| = q: budget 0"] == 0 and by["r = 0: budget logQ"] == logQ
    for j in range(64, logQ, 64):                                               # across a word boundary the budget moves by exactly one
        assert (by[f"2^{j} - 2: budget logQ - {j}"], by[f"2^{j}: budget logQ - {j} - 1"]) == (logQ - j, logQ - j - 1)
    if m == 64:                                                                 # ... and the model through the transforms agrees with the construction
        for c, (res, what) in enumerate(cases):
            assert model_of(rctx, t_model, cts[c], nl)[1:] == (maxres[c], int(budget[c])), what
    # a batch of 5, a different maximum at a different position in each; the budget-only entry point gives the same
    pick = [0, 1, len(lanes) + 2, len(lanes) + 3, count - 1]
    b5, m5 = ctx.noise_budget(sk1, logQ, p, ctx.upload(cts[pick]), nl, 5, maxres=True)
    assert len({maxres[c] for c in pick}) == 5 and m5 == [maxres[c] for c in pick] and [int(b) for b in b5] == [int(budget[c]) for c in pick]


def test_more_ciphertexts_than_one_grid_dimension():
    m, logQ, p = 22, 80, 23
    ctx, rctx, t_rows, sk1, t_model = ring(m, logQ, p)
    n, nl, nw = ctx.phim, 2, 2
    count = 65536 + 3
    cts = P.rand_limbs(np.random.default_rng(65539), (count, 2, n), nl, logQ)
    pick = [0, 32766, 32767, 65535, count - 1]                                   # (the entry point works through batches of 32767)
    for i, c in enumerate(pick):                                                # distinct small residuals at the picked places, so that a misplaced ciphertext shows
        cts[c, 1] = 0
        cts[c, 0] = O.ints_to_limbs([N.crafted_c0(2 * (i + 1) << (10 * i), logQ, p)] * n, nl)
    buf = ctx.upload(cts)
    msg, budget, maxres = ctx.decrypt_noise_batch(sk1, logQ, p, buf, nl, count, maxres=True)
    b5, m5 = ctx.noise_budget(sk1, logQ, p, ctx.upload(cts[pick]), nl, 5, maxres=True)
    for i, c in enumerate(pick):
        emsg, emax, ebudget = model_of(rctx, t_model, cts[c], nl)
        assert emax == 2 * (i + 1) << (10 * i)
        assert (maxres[c], int(budget[c]), [int(v) for v in msg[c]]) == (emax, ebudget, emsg), c
        assert (m5[i], int(b5[i])) == (emax, ebudget), c
    c = 40000                                                                   # ... and an unstructured one in the middle
    assert (maxres[c], int(budget[c])) == model_of(rctx, t_model, cts[c], nl)[1:]
    assert np.array_equal(msg[[1, c]], ctx.decrypt_batch(sk1, logQ, p, ctx.upload(cts[[1, c]]), nl, 2))


def test_valid_keys_fresh_budget_and_squarings():
    m, logQ, p = 64, 100, 257
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    rctx = R.Ctx(m, logQ, p, list(primes), list(roots))
    n, L, nl, nd = ctx.phim, len(primes), 2, R.ndigits(logQ)
    seed = 0x5EED0001
    sk1, pk0, pk1 = device_keys(ctx, logQ, seed)
    t_model = {i: [int(x) for x in sk1.row(i)] for i in range(L)}
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
    ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([one, sk1, sk1.copy().op(sk1, F.OP_MUL)], sk1, logQ, seed, seed ^ 0x5DEECE66D, 1000)
    count = 3
    rng = np.random.default_rng(3)
    msgs = rng.integers(0, p, size=(count, n)).astype(np.int64)
    cur = ctx.alloc(count * 2 * n * nl * 8)
    ctx.encrypt_batch_seeded(pk0, pk1, logQ, p, seed, 50, msgs, cur, nl)
    expect = [[int(v) for v in row] for row in msgs]
    last = None
    for step in range(5):
        msg, budget, maxres = ctx.decrypt_noise_batch(sk1, logQ, p, cur, nl, count, maxres=True)
        host = cur.download((count, 2, n, nl))
        print(f"squarings {step}: budget {[int(b) for b in budget]}")
        for c in range(count):
            assert (maxres[c], int(budget[c])) == model_of(rctx, t_model, host[c], nl)[1:], (step, c)
            if budget[c] > 0:
                assert [int(v) for v in msg[c]] == expect[c], (step, c)
            if last is not None:
                assert budget[c] <= last[c], (step, c)
        if step == 0:
            assert all(b > 0 for b in budget)
        last = [int(b) for b in budget]
        nxt = ctx.alloc(count * 2 * n * nl * 8)
        ctx.ct_mul_relin_dev(ksk, logQ, p, cur, cur, nxt, nl, count)
        cur = nxt
        expect = [[v % p for v in R.poly_mul_mod_phi(rctx, e, e)] for e in expect]


def test_slot_space_and_slot_basis():
    m, logQ, g = 64, 100, 3
    primes_p = [257, 193, 449]
    primes, roots = P.chain_for(m, logQ, 641)
    ctx = F.Context(m, primes, roots)
    n, nl, count, k = ctx.phim, 2, 3, 3
    words = 2 * n * nl * 8
    sk1, pk0, pk1 = device_keys(ctx, logQ, 77)
    B = F.SlotBasis.pow2(ctx, primes_p, g)
    rng = np.random.default_rng(8)
    ct = ctx.alloc(k * count * words)
    B.encrypt_batch_seeded(pk0, pk1, logQ, 77, 200, rng.integers(-1000, 1000, size=(count, n)).astype(np.int64), ct, nl)
    host = ct.download((k, count, 2, n, nl))
    host[:, 1] = P.rand_limbs(rng, (k, 2, n), nl, logQ)                          # one logical ciphertext without structure: budgets near 0
    host[1, 2, 0, 0] = O.ints_to_limbs([int(O.limbs_to_ints(host[1, 2, 0, :1])[0]) + (1 << 90)], nl)[0]      # one channel of another far worse than the rest
    ct.upload(host)
    per, low = B.noise_budget(sk1, logQ, ct, nl, count)
    assert per.shape == (k, count) and low.shape == (count,)
    for c in range(k):
        single = ctx.noise_budget(sk1, logQ, primes_p[c], View(ct, c * count * words), nl, count)
        assert np.array_equal(per[c], single), c
        assert np.array_equal(F.SlotSpace.pow2(ctx, primes_p[c], g).noise_budget(sk1, logQ, View(ct, c * count * words), nl, count), single), c
    assert np.array_equal(low, per.min(axis=0))
    assert per[:, 0].min() > 0 and per[1, 2] < per[0, 2] and low[2] == per[1, 2]


def test_refusals_name_the_condition():
    ctx, _, _, sk1, _ = ring(64, 64, 257)
    other = ring(22, 80, 23)[3]
    n, nl = ctx.phim, 1
    buf = ctx.upload(np.zeros((1, 2, n, nl), dtype=np.uint64))
    with pytest.raises(F.FhesiError, match="another context"):
        ctx.noise_budget(other, 64, 257, buf, nl, 1)
    with pytest.raises(F.FhesiError, match="another context"):
        ctx.decrypt_noise_batch(other, 64, 257, buf, nl, 1)
    with pytest.raises(F.FhesiError, match="modulus out of range"):
        ctx.noise_budget(sk1, 64, 1, buf, nl, 1)
    with pytest.raises(F.FhesiError, match="modulus out of range"):
        ctx.decrypt_noise_batch(sk1, 64, 1 << 62, buf, nl, 1)
    lib = F.Backend.lib()
    msg = np.zeros((1, n), dtype=np.int64)
    budget = np.zeros(1, dtype=np.int32)
    assert lib.fhesi_ct_noise_batch(ctx.h, sk1.h, 64, 257, buf.ptr, nl, 1, None, None) != 0
    assert b"null output" in lib.fhesi_last_error()
    assert lib.fhesi_decrypt_noise_batch(ctx.h, sk1.h, 64, 257, buf.ptr, nl, 1, None, F.binding._p(budget), None) != 0
    assert b"null output" in lib.fhesi_last_error()
    assert lib.fhesi_decrypt_noise_batch(ctx.h, sk1.h, 64, 257, buf.ptr, nl, 1, F.binding._p(msg), None, None) != 0
    assert b"null output" in lib.fhesi_last_error()
    B = F.SlotBasis.pow2(ctx, [257, 193], 3)
    assert lib.fhesi_ct_noise_int_batch(ctx.h, B.h, sk1.h, 64, buf.ptr, nl, 0, None) != 0
    assert b"null output" in lib.fhesi_last_error()
    assert np.array_equal(ctx.noise_budget(sk1, 64, 257, buf, nl, 1), [64])      # (the zero ciphertext: r = 0)
