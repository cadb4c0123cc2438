"""GPU: hoisted rotations (fhesi_ksk_hoist, fhesi_ct_rotations_dev, fhesi_ct_matvec_dev) through the C ABI -- against the CPU model of
tests/hoist_model.py, against the composition of the existing entry points on the derived matrix, against the C oracle, and through the scheme.
Exact throughout.  Keys are made on the device from seeds, as test_gpu_slots_pow2.py makes them."""
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import hoist_model as H
import oracle_lib as O
import params as P
import slots_pow2_model as M2
from slots_common import I, View, device_keys

pytestmark = pytest.mark.gpu
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def rotation_keys(ctx, logQ, ks, seed=SEED):
    """(sk1, pk0, pk1), the matrices W_k of the automorphisms ks (source key (1, s(X^k)), target s) and their derived matrices"""
    n, nd = ctx.phim, R.ndigits(logQ)
    sk1, pk0, pk1 = device_keys(ctx, logQ, seed)
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
    autos = [F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(k)], sk1, logQ, seed, PUB, 2000 + 100 * i) for i, k in enumerate(ks)]
    return (sk1, pk0, pk1), autos, [w.hoist(k) for w, k in zip(autos, ks)]


def reduce_host(a, logQ, nl):
    """centred residue modulo 2^logQ of two's complement limbs, for logQ = 64 nl: the low nl limbs"""
    assert logQ == 64 * nl
    return np.ascontiguousarray(a[..., :nl])


def composition(ctx, hoisted, k, logQ, src, nl, count):
    """the yardstick: the existing key switch with the derived matrix and k = 1, the existing `>>= k`, the reduction on the host"""
    n = ctx.phim
    if hoisted is None:
        return reduce_host(src.download((count, 2, n, nl)), logQ, nl)
    sw, rot = ctx.alloc(count * 2 * n * nl * 8), ctx.alloc(count * 2 * n * (nl + 1) * 8)
    ctx.ct_automorph_key_switch_dev(hoisted, logQ, 1, src, nl, count, sw, nl)
    ctx.ct_automorph_dev(k, sw, 2, nl, count, rot, nl + 1)
    return reduce_host(rot.download((count, 2, n, nl + 1)), logQ, nl)


def rotations(ctx, hoisted, ks, logQ, src, nl, count):
    out = ctx.alloc(len(ks) * count * 2 * ctx.phim * nl * 8)
    ctx.ct_rotations_dev(hoisted, ks, logQ, src, nl, count, out, nl)
    return out.download((len(ks), count, 2, ctx.phim, nl))


def inputs(rng, count, n, nl, logQ):
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    a[0, 0, 0] = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0]
    a[0, 0, 1] = O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    return a


def pyref_matrix(rows):
    """downloaded rows [2][ncol][L][n] -> the model's matrix of DoubleCRT dictionaries"""
    return [[{i: I(col[i]) for i in range(col.shape[0])} for col in row] for row in rows]


@functools.lru_cache(maxsize=None)
def model_case(m, p):
    """one small ring with its device matrices, the same matrices on the model, three ciphertexts and the model's rotations of them"""
    logQ, count = 128, 3
    ks = (3, 9, m - 1)
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    n, nl = ctx.phim, 2
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    rctx = R.Ctx(m, logQ, p, primes, roots)
    w_model = [H.hoist_matrix(rctx, pyref_matrix(w.download()), k) for w, k in zip(autos, ks)]
    a = inputs(np.random.default_rng(m), count, n, nl, logQ)
    cts = [[O.limbs_to_ints(a[i, r]) for r in range(2)] for i in range(count)]
    return ctx, rctx, ks, hoisted, w_model, a, cts


def as_ints(ct):
    return [O.limbs_to_ints(ct[r]) for r in range(2)]


@pytest.mark.parametrize("m,p,form", [(256, 257, 0),          # rows of 128: the per-chain-prime form
                                      (250, 251, 1)])         # 2 x 5^3: the four-prime limb form on folded rows; sigma reduces modulo Phi_m
def test_rotations_equal_the_model_bit_for_bit(m, p, form):
    ctx, rctx, ks, hoisted, w_model, a, cts = model_case(m, p)
    for h, w in zip(hoisted, w_model):                         # the derived matrix itself: the model's sigma_k^-1 of the same rows
        assert pyref_matrix(h.download()) == w
    want = H.rotations(rctx, list(w_model) + [None], list(ks) + [1], cts)
    got = rotations(ctx, list(hoisted) + [None], list(ks) + [1], 128, ctx.upload(a), 2, len(cts))
    assert all(h.form()[0] == form for h in hoisted), [h.form() for h in hoisted]
    for t in range(len(ks) + 1):
        for i in range(len(cts)):
            assert as_ints(got[t, i]) == want[t][i], (t, i)


@pytest.mark.parametrize("m,p", [(256, 257), (250, 251)])
def test_a_derived_matrix_is_an_ordinary_matrix_for_the_existing_key_switch(m, p):
    ctx, rctx, ks, hoisted, w_model, a, cts = model_case(m, p)
    n, count = ctx.phim, len(cts)
    out = ctx.alloc(count * 2 * n * 2 * 8)
    for h, w in zip(hoisted, w_model):
        ctx.ct_automorph_key_switch_dev(h, 128, 1, ctx.upload(a), 2, count, out, 2)
        got = out.download((count, 2, n, 2))
        for i in range(count):
            assert as_ints(got[i]) == R.apply_key_switch_parts(rctx, w, cts[i]), i
        assert h.nbytes == 2 * 2 * rctx.ndigits * rctx.L * n * 8 and h.key_bits()[1] >= 0


RINGS = {4096: (65537, (3, 9, 27, 81, 4095), 2),              # the two largest chain primes, limbs
         1 << 15: (65537, (3, 9, 27, 81, (1 << 15) - 1), 1),  # four 30-bit primes on rows of 2^14: the smallest shape that reaches dot32_kernel2m
         1458: (1459, (5, 25, 125, 625, 1457), 1)}            # 2 x 3^6: four 30-bit primes on folded rows, where W' may take one limb more


@pytest.mark.parametrize("m", sorted(RINGS))
def test_rotations_equal_the_composition_of_the_existing_entry_points(m):
    """counts 1, 3 (a ragged tile) and 9 (past one tile of 8) x 1, 2, 5 matrices x both dot paths where both apply, word for word against
    ct_automorph_key_switch_dev(W', k = 1) + ct_automorph_dev(k) + the reduction, computed once for 9 ciphertexts and all matrices (a
    rotation of ciphertext i does not depend on its neighbours)"""
    p, ks, form = RINGS[m]
    logQ, nl, top = 128, 2, 9
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    n = ctx.phim
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    a = inputs(np.random.default_rng(m), top, n, nl, logQ)
    src = ctx.upload(a)
    want = np.stack([composition(ctx, h, k, logQ, src, nl, top) for h, k in zip(hoisted, ks)])
    ident = composition(ctx, None, 1, logQ, src, nl, top)
    assert all(h.form()[0] == form for h in hoisted), [h.form() for h in hoisted]
    if m == 4096:                                              # ... and the C oracle on the downloaded derived matrix
        w = hoisted[1].download()
        sw = O.Oracle(m, primes, roots).apply_key_switch_parts(w, a[0], logQ, nl)
        assert np.array_equal(reduce_host(O.Oracle(m, primes, roots).ct_automorph(sw, ks[1], nl + 1), logQ, nl), want[1, 0])
    for how in ((1, 2) if form == 1 else (1,)):
        ctx.set_option("hoist_dot", how)
        for count in (1, 3, 9):
            for nk in (1, 2, 5):
                ctx.prof_enable(form == 1)
                got = rotations(ctx, hoisted[:nk] + [None], list(ks[:nk]) + [1], logQ, ctx.upload(a[:count]), nl, count)
                if form == 1:                                  # the kernel that ran: the multi-matrix one with a tile no deeper than the batch, or launch_dot32's
                    name = ctx.prof_kernel_name("dot")
                    ctx.prof_enable(False)
                    tile = {1: 1, 3: 4, 9: 8}[count]
                    assert (f"dot32_kernel2m<{tile}, " in name) if how == 2 else ("dot32_kernel2<8, " in name), (how, count, nk, name)
                assert np.array_equal(got[:nk], want[:nk, :count]), (how, count, nk)
                assert np.array_equal(got[nk], ident[:count]), (how, count, nk)
    ctx.set_option("hoist_dot", 0)
    got = rotations(ctx, hoisted, ks, logQ, src, nl, top)
    assert np.array_equal(got, want)
    # the evaluation-row route of `>>=` closes a rotation with the same bits as the coefficient gather
    ctx.set_option("automorph_rows", 1)
    assert np.array_equal(rotations(ctx, hoisted[:2], ks[:2], logQ, ctx.upload(a[:3]), nl, 3), want[:2, :3])
    ctx.set_option("automorph_rows", 0)


def test_matrices_of_two_limb_shapes_go_in_two_groups():
    """a generated matrix (centred limbs) next to an uploaded matrix of uniform residues (general limbs of the chain product): different limb
    counts, so the multi-matrix kernel runs once per shape"""
    m, logQ, nl, count = 1 << 15, 128, 2, 3
    ks = (3, (1 << 15) - 1, 9)
    primes, roots = P.chain_for(m, logQ, 65537)
    ctx = F.Context(m, primes, roots)
    n, nd = ctx.phim, R.ndigits(logQ)
    _, autos, hoisted = rotation_keys(ctx, logQ, ks[:2])
    rng = np.random.default_rng(5)
    uniform = F.KeySwitchMatrix(ctx, 2, nd).upload(np.stack([P.rand_rows(rng, primes, n, 2 * nd) for _ in range(2)])).hoist(ks[2])
    mats = [hoisted[0], uniform, hoisted[1]]
    order = (ks[0], ks[2], ks[1])
    a = inputs(rng, count, n, nl, logQ)
    src = ctx.upload(a)
    want = np.stack([composition(ctx, h, k, logQ, src, nl, count) for h, k in zip(mats, order)])
    assert mats[0].form()[1] == mats[2].form()[1] != mats[1].form()[1], [h.form() for h in mats]
    for how in (2, 1, 0):
        ctx.set_option("hoist_dot", how)
        assert np.array_equal(rotations(ctx, mats, order, logQ, src, nl, count), want), how


def test_rotations_and_matvec_through_the_scheme():
    m, logQ, p, g = 4096, 128, 65537, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S, mod = F.SlotSpace.pow2(ctx, p, g), M2.slot_space(m, p, g)
    n, nl, count = S.total, 2, 2
    amounts = (1, 2, 3, "swap")
    ks = [S.rotation_k(t) for t in amounts]
    assert ks == [3, 9, 27, m - 1]
    (sk1, pk0, pk1), autos, hoisted = rotation_keys(ctx, logQ, ks)
    rng = np.random.default_rng(m)
    x = rng.integers(0, p, size=(count, n)).astype(np.int64)
    words = 2 * n * nl
    cx = ctx.alloc(count * words * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, x, cx, nl)
    # every rotation decrypts to the rotated rows / the swapped rows, with noise budget left
    rot = ctx.alloc(len(ks) * count * words * 8)
    S.rotations(hoisted, amounts, logQ, cx, nl, count, rot, nl)
    for t, amount in enumerate(amounts):
        got = S.decrypt_batch(sk1, logQ, View(rot, t * count * words * 8), nl, count)
        for i in range(count):
            want = M2.swap_rows(mod, I(x[i])) if amount == "swap" else M2.rotate_rows(mod, I(x[i]), amount)
            assert I(got[i]) == want, (amount, i)
    budget = S.noise_budget(sk1, logQ, rot, nl, len(ks) * count)
    assert (np.asarray(budget) > 0).all(), budget
    # a matrix-vector product by 4 diagonals: sum_t rotate(x, t) o d_t modulo p
    diag_amounts = (0, 1, 2, 3)
    mats = [None] + hoisted[:3]
    d = rng.integers(0, p, size=(len(diag_amounts), n)).astype(np.int64)
    plain = S.plain(d, False)
    out = ctx.alloc(count * words * 8)
    S.matvec(mats, diag_amounts, plain, logQ, cx, nl, count, out)
    got = S.decrypt_batch(sk1, logQ, out, nl, count)
    for i in range(count):
        want = np.zeros(n, dtype=object)
        for t in diag_amounts:
            want = (want + np.array(M2.rotate_rows(mod, I(x[i]), t), dtype=object) * np.array(I(d[t]), dtype=object)) % p
        assert I(got[i]) == I(want), i
    assert (np.asarray(S.noise_budget(sk1, logQ, out, nl, count)) > 0).all()
    # ... bit for bit the rotations into a pool followed by the plaintext sum
    pool = ctx.alloc(len(diag_amounts) * count * words * 8)
    S.rotations(mats, diag_amounts, logQ, cx, nl, count, pool, nl)
    a_idx = [t * count + i for i in range(count) for t in range(len(diag_amounts))]
    b_idx = [t for i in range(count) for t in range(len(diag_amounts))]
    seg = [i * len(diag_amounts) for i in range(count + 1)]
    two = ctx.alloc(count * words * 8)
    ctx.ct_plain_sum_dev(plain, logQ, pool, len(diag_amounts) * count, nl, a_idx, b_idx, seg, two)
    assert np.array_equal(out.download((count, 2, n, nl)), two.download((count, 2, n, nl)))


def test_refusals_name_their_condition_and_leave_the_context_working():
    m, logQ, nl, count = 4096, 128, 2, 2
    ks = (3, 9)
    primes, roots = P.chain_for(m, logQ, 65537)
    ctx = F.Context(m, primes, roots)
    other = F.Context(m, primes, roots)
    n, nd = ctx.phim, R.ndigits(logQ)
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    _, _, foreign = rotation_keys(other, logQ, ks[:1])
    a = inputs(np.random.default_rng(1), count, n, nl, logQ)
    src = ctx.upload(a)
    words = 2 * n * nl
    out = ctx.alloc(len(ks) * count * words * 8)
    good = rotations(ctx, hoisted, ks, logQ, src, nl, count)

    def refused(word, call):
        with pytest.raises(F.FhesiError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(rotations(ctx, hoisted, ks, logQ, src, nl, count), good), word      # a following good call succeeds

    refused("not in Zm*", lambda: autos[0].hoist(2))
    refused("source components", lambda: F.KeySwitchMatrix(ctx, 3, nd).hoist(3))
    refused("not made by fhesi_ksk_hoist", lambda: ctx.ct_rotations_dev([autos[0], hoisted[1]], ks, logQ, src, nl, count, out, nl))
    refused("hoisted for k=3", lambda: ctx.ct_rotations_dev([hoisted[0], hoisted[0]], ks, logQ, src, nl, count, out, nl))
    refused("no matrix", lambda: ctx.ct_rotations_dev([hoisted[0], None], ks, logQ, src, nl, count, out, nl))
    refused("another context", lambda: ctx.ct_rotations_dev([foreign[0], hoisted[1]], ks, logQ, src, nl, count, out, nl))
    refused("digits", lambda: ctx.ct_rotations_dev(hoisted, ks, logQ, src, nl, count, out, nl, decomp_bytes=2))
    refused("cannot hold", lambda: ctx.ct_rotations_dev(hoisted, ks, logQ, src, nl, count, out, 1))
    refused("overlaps", lambda: ctx.ct_rotations_dev(hoisted, ks, logQ, View(out, words * 8), nl, count, out, nl))
    ctx.set_option("hoist_dot", 2)                           # this ring runs the 60-bit limb form
    with pytest.raises(F.FhesiError) as e:
        ctx.ct_rotations_dev(hoisted, ks, logQ, src, nl, count, out, nl)
    assert "hoist_dot" in str(e.value) and "four-prime" in str(e.value), str(e.value)
    ctx.set_option("hoist_dot", 0)
    S = F.SlotSpace.pow2(ctx, 65537, 3)
    one_diag = S.plain(np.ones((1, n), dtype=np.int64), False)
    res = ctx.alloc(count * words * 8)
    refused("prepared diagonals", lambda: ctx.ct_matvec_dev(hoisted, ks, one_diag, logQ, src, nl, count, res))
    refused("overlaps", lambda: ctx.ct_matvec_dev(hoisted[:1], ks[:1], one_diag, logQ, src, nl, count, src))
    ctx.ct_matvec_dev(hoisted[:1], ks[:1], one_diag, logQ, src, nl, count, res)
