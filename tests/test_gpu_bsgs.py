"""GPU: baby-step/giant-step matrix-vector products (fhesi_ct_rot_sum_dev, fhesi_ct_matvec_bsgs_dev) through the C ABI -- the rotated sum against
the composition of the existing entry points and the C oracle without any key, the product word for word against the composition it is defined as,
against the CPU model of tests/bsgs_model.py, and through the scheme.  Exact throughout."""
import functools
import math

import numpy as np
import pytest

import bsgs_model as BM
import fhe_si_amd as F
import fhesi_pyref as R
import hoist_model as H
import oracle_lib as O
import params as P
import slots_pow2_model as M2
from bsgs_common import as_ints, centred, extremes, inputs, pyref_matrix, rotation_keys
from slots_common import I, View

pytestmark = pytest.mark.gpu
CAP = F.binding.ROT_SUM_MAX_TERMS


def ints_of(a):
    """[..][nl] uint64 two's complement limbs -> object array [..] of Python ints"""
    return F.unpack_limbs(np.ascontiguousarray(a).view(np.int64))


def limbs_of(v, nl):
    return F.pack_limbs(v, nl).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the rotated sum, no keys
@pytest.mark.parametrize("m,p,kernel", [(256, 257, True),        # mode 0: m = 2^k
                                        (250, 251, True),        # mode 1: m = 2 q^k
                                        (125, 251, True),        # mode 2: m = q^k
                                        (45, 181, False)])       # two odd prime factors: no signed gather, the library composes
def test_rot_sum_equals_the_composition_and_the_oracle(m, p, kernel):
    """nlimbs 2 / 3 (the sign bit inside a limb) / 9 / 17: every instantiation; 1, 2, CAP and CAP + 1 terms (one launch, a full one, a chain); no base,
    a base, out == base.  Terms 2u and 2u + 1 share their k and every term holds the two extremes at source coefficients 0 and 1, so the sums cross
    the centred boundary in both directions."""
    count, top = 3, CAP + 1
    units = [k for k in range(2, m) if math.gcd(k, m) == 1]
    kset = (units[0], units[len(units) // 2], m - 1)
    ks = [kset[(t // 2) % 3] for t in range(top)]
    for nl, logQ in ((2, 128), (3, 130), (9, 576), (17, 1088)):
        primes, roots = P.chain_for(m, logQ, p)
        ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
        n = ctx.phim
        ctb = 2 * n * nl * 8
        a = P.rand_limbs(np.random.default_rng(m + nl), (top + 1, count, 2, n), nl, logQ)
        a[:, :, :, 0], a[:, :, :, 1] = extremes(logQ, nl)
        pre, base = a[:top], a[top]
        pre_dev, base_dev = ctx.upload(pre), ctx.upload(base)
        # the oracle: Ciphertext >>= k per term, summed as integers
        rot = np.stack([np.stack([ints_of(orc.ct_automorph(pre[t, i], ks[t], nl + 1)) for i in range(count)]) for t in range(top)])
        crossed = False
        # the composition on the device: ct_automorph_dev per term, ct_add_dev
        term = ctx.alloc(count * ctb)
        acc = {False: ctx.upload(np.zeros_like(base)), True: ctx.upload(base)}
        want, run = {}, {False: np.zeros((count, 2, n), dtype=object), True: ints_of(base)}
        for t in range(top):
            ctx.ct_automorph_dev(ks[t], View(pre_dev, t * count * ctb), 2, nl, count, term, nl)
            for with_base in (False, True):
                ctx.ct_add_dev(logQ, acc[with_base], term, 2, nl, count)
                run[with_base] = run[with_base] + rot[t]
            if t + 1 in (1, 2, CAP, top):
                for with_base in (False, True):
                    comp = acc[with_base].download((count, 2, n, nl))
                    crossed |= bool((np.abs(run[with_base]) >= (1 << (logQ - 1))).any())
                    assert np.array_equal(comp, limbs_of(np.vectorize(lambda v: centred(v, logQ), otypes=[object])(run[with_base]), nl)), (nl, t + 1, with_base)
                    want[t + 1, with_base] = comp
        assert crossed
        for nk in (1, 2, CAP, top):
            out = ctx.alloc(count * ctb)
            ctx.ct_rot_sum_dev(ks[:nk], logQ, None, pre_dev, count, nl, out)
            assert np.array_equal(out.download((count, 2, n, nl)), want[nk, False]), (nl, nk, "no base")
            ctx.ct_rot_sum_dev(ks[:nk], logQ, base_dev, pre_dev, count, nl, out)
            assert np.array_equal(out.download((count, 2, n, nl)), want[nk, True]), (nl, nk, "base")
            both = ctx.upload(base)
            ctx.ct_rot_sum_dev(ks[:nk], logQ, both, pre_dev, count, nl, both)
            assert np.array_equal(both.download((count, 2, n, nl)), want[nk, True]), (nl, nk, "out == base")
        if kernel:                                              # the composed form on a ring that has the kernel: the same words
            ctx.set_option("automorph_rows", 1)
            out = ctx.alloc(count * ctb)
            ctx.ct_rot_sum_dev(ks[:2], logQ, base_dev, pre_dev, count, nl, out)
            assert np.array_equal(out.download((count, 2, n, nl)), want[2, True]), nl
            ctx.ct_rot_sum_dev(ks[:2], logQ, None, pre_dev, count, nl, out)
            assert np.array_equal(out.download((count, 2, n, nl)), want[2, False]), nl
            ctx.set_option("automorph_rows", 0)


# ------------------------------------------------------------------------------------------------ the product against its definition
RINGS = {4096: (65537, 3, 2),              # the two largest chain primes, limbs
         1 << 15: (65537, 3, 1),           # four 30-bit primes on rows of 2^14: the smallest shape that reaches dot32_kernel2m
         1458: (1459, 5, 1)}               # 2 x 3^6: four 30-bit primes on folded rows
SHAPES = ((1, 1, 1), (3, 1, 3), (1, 3, 3), (2, 2, 4), (3, 2, 5))


def composition(ctx, mats, gen, B, G, nk, plain, logQ, src, nl, count):
    """fhesi_ct_rotations_dev for the babies, fhesi_ct_plain_sum_dev with G groups per ciphertext, fhesi_ct_rotations_dev with one matrix per giant,
    fhesi_ct_add_dev"""
    n = ctx.phim
    ctb = 2 * n * nl * 8
    nb = min(B, nk)
    kb, kg = [pow(gen, j, ctx.m) for j in range(nb)], [pow(gen, g * B, ctx.m) for g in range(G)]
    pool = ctx.alloc(nb * count * ctb)
    ctx.ct_rotations_dev([mats[k] for k in kb], kb, logQ, src, nl, count, pool, nl)
    a_idx, b_idx, seg = [], [], [0]
    for g in range(G):
        for i in range(count):
            for j in range(B):
                if g * B + j < nk:
                    a_idx.append(j * count + i)
                    b_idx.append(g * B + j)
            seg.append(len(a_idx))
    inner = ctx.alloc(G * count * ctb)
    ctx.ct_plain_sum_dev(plain, logQ, pool, nb * count, nl, a_idx, b_idx, seg, inner)
    acc, rot = ctx.alloc(count * ctb), ctx.alloc(count * ctb)
    for g in range(G):
        ctx.ct_rotations_dev([mats[kg[g]]], [kg[g]], logQ, View(inner, g * count * ctb), nl, count, acc if g == 0 else rot, nl)
        if g:
            ctx.ct_add_dev(logQ, acc, rot, 2, nl, count)
    return acc.download((count, 2, n, nl))


def bsgs(ctx, mats, gen, B, G, nk, plain, logQ, src, nl, count):
    kb, kg = [pow(gen, j, ctx.m) for j in range(B)], [pow(gen, g * B, ctx.m) for g in range(G)]
    out = ctx.alloc(count * 2 * ctx.phim * nl * 8)
    ctx.ct_matvec_bsgs_dev([mats[k] for k in kb], kb, [mats[k] for k in kg], kg, nk, plain, logQ, src, nl, count, out)
    return out.download((count, 2, ctx.phim, nl))


@pytest.mark.parametrize("m", sorted(RINGS))
def test_bsgs_equals_the_composition_of_the_existing_entry_points(m):
    """every shape x counts 1 and 9, word for word; the composition computed once for 9 ciphertexts (ciphertext i does not depend on its neighbours);
    one giant step is fhesi_ct_matvec_dev"""
    p, gen, form = RINGS[m]
    logQ, nl, top = 128, 2, 9
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    n = ctx.phim
    ks = [pow(gen, e, m) for e in (1, 2, 3)]
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    mats = dict(zip(ks, hoisted))
    mats[1] = None
    rng = np.random.default_rng(m)
    a = inputs(rng, top, n, nl, logQ)
    src = ctx.upload(a)
    plain = ctx.plain_from_poly(rng.integers(0, p, size=(5, n)))
    for B, G, nk in SHAPES:
        want = composition(ctx, mats, gen, B, G, nk, plain, logQ, src, nl, top)
        for count in (1, 9):
            got = bsgs(ctx, mats, gen, B, G, nk, plain, logQ, ctx.upload(a[:count]), nl, count)
            assert np.array_equal(got, want[:count]), (B, G, nk, count)
        if G == 1:
            kb = [pow(gen, j, m) for j in range(nk)]
            flat = ctx.alloc(top * 2 * n * nl * 8)
            ctx.ct_matvec_dev([mats[k] for k in kb], kb, plain, logQ, src, nl, top, flat)
            assert np.array_equal(flat.download((top, 2, n, nl)), want), (B, G, nk)
    assert all(h.form()[0] == form for h in hoisted), [h.form() for h in hoisted]
    # the evaluation-row route of `>>=` closes the giants with the same bits as the rotated-sum kernel
    want = composition(ctx, mats, gen, 2, 2, 4, plain, logQ, src, nl, 3)
    ctx.set_option("automorph_rows", 1)
    assert np.array_equal(bsgs(ctx, mats, gen, 2, 2, 4, plain, logQ, src, nl, 3), want)
    ctx.set_option("automorph_rows", 0)


@functools.lru_cache(maxsize=None)
def small_case(m, p):
    """one small ring with the device matrices of k = 3 and 9, the same matrices on the model, and three ciphertexts"""
    logQ, count, ks = 128, 3, (3, 9)
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    rctx = R.Ctx(m, logQ, p, primes, roots)
    w_model = [H.hoist_matrix(rctx, pyref_matrix(w.download()), k) for w, k in zip(autos, ks)]
    a = inputs(np.random.default_rng(m), count, ctx.phim, 2, logQ)
    return ctx, rctx, hoisted, w_model, a


def test_the_launch_chain_is_crossed_through_the_full_call():
    """CAP + 1 giant steps of one (identity) baby step each on m = 256: the rotated sum takes a full launch and a second one with base = out"""
    m, p, logQ, nl = 256, 257, 128, 2
    ctx, rctx, hoisted, w_model, a = small_case(m, p)
    n, count, G = ctx.phim, a.shape[0], CAP + 1
    mats = [None, hoisted[0], hoisted[1]]
    kg = [(1, 3, 9)[g % 3] for g in range(G)]
    gm = [mats[g % 3] for g in range(G)]
    plain = ctx.plain_from_poly(np.random.default_rng(9).integers(0, p, size=(G, n)))
    src = ctx.upload(a)
    ctb = 2 * n * nl * 8
    out = ctx.alloc(count * ctb)
    ctx.ct_matvec_bsgs_dev([None], [1], gm, kg, G, plain, logQ, src, nl, count, out)
    # the definition: one plaintext product per giant, its rotation, the sum
    inner, acc, rot = ctx.alloc(G * count * ctb), ctx.alloc(count * ctb), ctx.alloc(count * ctb)
    pool = ctx.alloc(count * ctb)
    ctx.ct_rotations_dev([None], [1], logQ, src, nl, count, pool, nl)
    ctx.ct_plain_sum_dev(plain, logQ, pool, count, nl, [i for g in range(G) for i in range(count)], [g for g in range(G) for i in range(count)],
                         list(range(G * count + 1)), inner)
    for g in range(G):
        ctx.ct_rotations_dev([gm[g]], [kg[g]], logQ, View(inner, g * count * ctb), nl, count, acc if g == 0 else rot, nl)
        if g:
            ctx.ct_add_dev(logQ, acc, rot, 2, nl, count)
    assert np.array_equal(out.download((count, 2, n, nl)), acc.download((count, 2, n, nl)))


# ------------------------------------------------------------------------------------------------ the model and the scheme
@pytest.mark.parametrize("m,p", [(256, 257), (250, 251)])
def test_bsgs_equals_the_model_bit_for_bit(m, p):
    ctx, rctx, hoisted, w_model, a = small_case(m, p)
    n, count = ctx.phim, 2
    kb, kg, nk = [1, 3], [1, 9], 3                              # the last group ragged
    diags = np.random.default_rng(m + 1).integers(0, p, size=(nk, n))
    out = ctx.alloc(count * 2 * n * 2 * 8)
    ctx.ct_matvec_bsgs_dev([None, hoisted[0]], kb, [None, hoisted[1]], kg, nk, ctx.plain_from_poly(diags), 128, ctx.upload(a[:count]), 2, count, out)
    got = out.download((count, 2, n, 2))
    for i in range(count):
        want = BM.matvec_bsgs(rctx, [None, w_model[0]], kb, [None, w_model[1]], kg, nk, [I(d) for d in diags], as_ints(a[i]))
        assert as_ints(got[i]) == want, i


def test_bsgs_through_the_scheme():
    """16 diagonals as 4 x 4 on the two-row space of (4096, 65537, logQ 128): the slots of the product, and of the flat product"""
    m, logQ, p, g, T, B = 4096, 128, 65537, 3, 16, 4
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S, mod = F.SlotSpace.pow2(ctx, p, g), M2.slot_space(m, p, g)
    n, nl, count = S.total, 2, 2
    assert F.matvec_bsgs_plan(T) == (B, T // B)
    ks = [S.rotation_k(t) for t in range(1, T)]
    (sk1, pk0, pk1), autos, hoisted = rotation_keys(ctx, logQ, ks)
    mats = [None] + hoisted                                     # mats[t]: the derived matrix of g^t
    rng = np.random.default_rng(m)
    x = rng.integers(0, p, size=(count, n)).astype(np.int64)
    d = rng.integers(0, p, size=(T, n)).astype(np.int64)
    assert I(S.rotate_values(x[0], 5)) == M2.rotate_rows(mod, I(x[0]), 5) and I(S.rotate_values(S.rotate_values(x[0], 5), -5)) == I(x[0])
    words = 2 * n * nl
    cx = ctx.alloc(count * words * 8)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, x, cx, nl)
    flat, out = ctx.alloc(count * words * 8), ctx.alloc(count * words * 8)
    S.matvec(mats, range(T), S.plain(d, False), logQ, cx, nl, count, flat)
    S.matvec_bsgs(mats[:B], [mats[i * B] for i in range(T // B)], B, S.plain(S.bsgs_diagonals(d, B), False), logQ, cx, nl, count, out)
    got, ref = S.decrypt_batch(sk1, logQ, out, nl, count), S.decrypt_batch(sk1, logQ, flat, nl, count)
    for i in range(count):
        want = np.zeros(n, dtype=object)
        for t in range(T):
            want = (want + S.rotate_values(x[i], t).astype(object) * d[t].astype(object)) % p
        assert I(got[i]) == I(want) == I(ref[i]), i
    assert (np.asarray(S.noise_budget(sk1, logQ, out, nl, count)) > 0).all()
    assert (np.asarray(S.noise_budget(sk1, logQ, flat, nl, count)) > 0).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_condition_and_leave_the_context_working():
    m, logQ, nl, count = 4096, 128, 2, 2
    ks = (3, 9)
    primes, roots = P.chain_for(m, logQ, 65537)
    ctx, other = F.Context(m, primes, roots), F.Context(m, primes, roots)
    n = ctx.phim
    _, autos, hoisted = rotation_keys(ctx, logQ, ks)
    _, _, foreign = rotation_keys(other, logQ, ks[:1])
    a = inputs(np.random.default_rng(1), 3 * count, n, nl, logQ)
    src = ctx.upload(a[:count])
    words = 2 * n * nl
    out = ctx.alloc(count * words * 8)
    plain = ctx.plain_from_poly(np.ones((4, n), dtype=np.int64))
    one_diag, foreign_plain = ctx.plain_from_poly(np.ones((1, n), dtype=np.int64)), other.plain_from_poly(np.ones((4, n), dtype=np.int64))
    baby, kb, giant, kg = [None, hoisted[0]], [1, 3], [None, hoisted[1]], [1, 9]

    def product(bm=baby, kbs=kb, gmat=giant, kgs=kg, nk=4, w=plain, s=src, o=out, **kw):
        ctx.ct_matvec_bsgs_dev(bm, kbs, gmat, kgs, nk, w, logQ, s, nl, count, o, **kw)
        return o.download((count, 2, n, nl))

    good = product()

    def refused(word, call):
        with pytest.raises(F.FhesiError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(product(), good), word           # a following good call succeeds

    refused("at least 1", lambda: product(bm=[], kbs=[]))
    refused("at least 1", lambda: product(gmat=[], kgs=[]))
    refused("outside (2, 4]", lambda: product(nk=2))
    refused("outside (2, 4]", lambda: product(nk=5))
    refused("not made by fhesi_ksk_hoist", lambda: product(bm=[None, autos[0]]))
    refused("not made by fhesi_ksk_hoist", lambda: product(gmat=[None, autos[1]]))
    refused("hoisted for k=3", lambda: product(gmat=[None, hoisted[0]]))
    refused("no matrix", lambda: product(bm=[None, None]))
    refused("no matrix", lambda: product(gmat=[None, None]))
    refused("another context", lambda: product(bm=[None, foreign[0]]))
    refused("another context", lambda: product(w=foreign_plain))
    refused("digits", lambda: product(decomp_bytes=2))
    refused("prepared diagonals", lambda: product(w=one_diag))
    refused("overlaps", lambda: product(o=src))
    # the rotated sum
    pre = ctx.upload(a)                                         # 3 terms of `count` ciphertexts
    res = ctx.alloc(count * words * 8)
    refused("overlaps pre", lambda: ctx.ct_rot_sum_dev([3, 9, 27], logQ, None, pre, count, nl, View(pre, 2 * count * words * 8)))
    refused("without being base", lambda: ctx.ct_rot_sum_dev([3], logQ, View(pre, words * 8), View(pre, 2 * count * words * 8), count, nl, pre))
    refused("not in Zm*", lambda: ctx.ct_rot_sum_dev([3, 2, 27], logQ, None, pre, count, nl, res))
    refused("not in Zm*", lambda: ctx.ct_rot_sum_dev([3, m + 1, 27], logQ, None, pre, count, nl, res))
    refused("outside the supported 1..32", lambda: ctx.ct_rot_sum_dev([3], logQ, None, pre, count, 33, res))
    refused("outside the supported 1..32", lambda: ctx.ct_rot_sum_dev([3], logQ, None, pre, count, 0, res))
    refused("cannot hold", lambda: ctx.ct_rot_sum_dev([3], logQ, None, pre, count, 1, res))
    refused("0 terms", lambda: ctx.ct_rot_sum_dev([], logQ, None, pre, count, nl, res))
    ctx.ct_rot_sum_dev([3, 9, 27], logQ, None, pre, count, nl, res)
