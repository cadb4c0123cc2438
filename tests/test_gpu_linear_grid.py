"""GPU: dense layers larger than a row of slots (fhesi_linear_grid_*, fhesi_ct_linear_grid_dev) through the C ABI -- the diagonals linear_diag_kernel
writes for a block of a larger matrix against the model of tests/linear_grid_model.py without any key, the call word for word against the composition
of existing entry points it is defined as, through the scheme, and the refusals.  Exact throughout."""
import ctypes

import numpy as np
import pytest

import fhe_si_amd as F
import linear_grid_model as GM
import linear_model as LM
import params as P
from bsgs_common import inputs, rotation_keys
from slots_common import I, View, context
from test_gpu_linear import LOGQ, NL, DevTensor, planted, ring      # ring(): one context and key set per ring for both modules

pytestmark = pytest.mark.gpu


def shape_of(block, grid):
    (Rb, Cb), (nI, nJ) = block, grid
    return Rb, Cb, nI, nJ, nI * Rb, nJ * Cb


# ------------------------------------------------------------------------------------------------ the diagonals, no keys
def check_diagonals(S, cases, seed):
    rng = np.random.default_rng(seed)
    rows, cols = max(S.rows, 1), S.total // max(S.rows, 1)
    for block, grid in cases:
        Rb, Cb, nI, nJ, R, C = shape_of(block, grid)
        M = planted(rng, S.p, R, C)
        if R * C >= 7:
            assert (M < 0).any() and (M == 0).any() and (M == S.p).any() and (abs(M) == 1 << 62).any()
        for baby in (0, 3):
            pl = F.linear_grid_plan(cols, R, C, Rb, Cb, baby)
            assert pl == GM.plan(cols, R, C, Rb, Cb, baby)
            want = np.asarray(GM.prepared(M, Rb, Cb, rows, cols, pl["B"]), dtype=object) % S.p
            got = S.linear_grid_diagonals(M, block, baby)
            assert got.shape == (nI, nJ, pl["T"], S.total) and np.array_equal(got.astype(object), want), (block, grid, baby)


def test_diagonals_equal_the_model_on_a_two_row_ring():
    """m = 64, p = 257, g = 3: two rows of 16.  A wrong origin or leading dimension shows on (4,4) x (2,3) -- every block differs, ld = 12 != Cb --, the
    32 x 32 matrix fills rows it does not fit, (4,16) and (16,4) are wide and tall blocks, (1,1) replicates one entry; baby = 3 gives a ragged last giant
    and a negative wrap of i - g B.  Then the host and the device constructor through a grid that takes no matrix."""
    big, _ = context(64, LOGQ, 257)
    SB = F.SlotSpace.pow2(big, 257, 3)
    assert (SB.rows, SB.cols, SB.total) == (2, 16, 32)
    check_diagonals(SB, [((4, 4), (2, 3)), ((16, 16), (2, 2)), ((4, 16), (3, 1)), ((16, 4), (1, 3)), ((1, 1), (2, 2))], 64)
    # the default block: what the row holds
    M = planted(np.random.default_rng(5), 257, 32, 48)
    assert np.array_equal(SB.linear_grid_diagonals(M), SB.linear_grid_diagonals(M, (16, 16)))
    # (1,1) x (2,2): one diagonal per block, no rotation at all -- out[I] = sum_J M[I][J] in[J] + b[I]
    n, count = big.phim, 2
    M, b = np.array([[-5, 300], [1 << 62, 7]], dtype=np.int64), np.array([300, -1], dtype=np.int64)
    src = big.upload(np.concatenate([inputs(np.random.default_rng(J + 1), count, n, NL, LOGQ) for J in range(2)]))
    outs = []
    for lin in (SB.linear_grid(M, b, (1, 1)), SB.linear_grid(DevTensor(big, M), DevTensor(big, b), (1, 1), device=True)):
        assert (lin.R, lin.C, lin.Rb, lin.Cb, lin.nI, lin.nJ, lin.T, lin.B, lin.G, lin.nfold, lin.amounts, lin.has_bias, lin.key_switches) == \
            (2, 2, 1, 1, 2, 2, 1, 1, 1, 0, [], True, 0)
        out = big.alloc(2 * count * 2 * n * NL * 8)
        lin.apply([], LOGQ, src, NL, count, out)
        outs.append(out.download((2, count, 2, n, NL)))
        lin.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], composition(big, SB, {}, M, b, (1, 1), 0, src, count))


def test_diagonals_equal_the_model_on_a_single_row_ring():
    """m = 257 (prime), p = 1543, g = 3 of order 256: one row of 256 slots through the chirp embedding's space"""
    ctx, _ = context(257, 64, 1543)
    S = F.SlotSpace(ctx, 1543, 3)
    assert (max(S.rows, 1), S.total) == (1, 256)
    check_diagonals(S, [((4, 64), (2, 2))], 257)


# ------------------------------------------------------------------------------------------------ the call against its definition
def composition(ctx, S, mats, M, bias, block, baby, src, count):
    """fhesi_ct_rotations_dev per input block into one pool, ONE fhesi_ct_plain_sum_dev with the groups (I, g, i) and the terms (J, j) over the plaintext
    SlotSpace.plain makes of the model's diagonals, per output block fhesi_ct_rotations_dev of each inner sum by its giant and fhesi_ct_add_dev,
    fhesi_ct_rot_fold_dev, fhesi_ct_add_slots_dev with the block's replicated bias -> [nI][count][2][n][NL]"""
    (Rb, Cb), (R, C) = block, M.shape
    pl = GM.plan(S.cols, R, C, Rb, Cb, baby)
    nI, nJ, T, B, G = pl["nI"], pl["nJ"], pl["T"], pl["B"], pl["G"]
    nb, ctb = min(B, T), 2 * ctx.phim * NL * 8
    w = np.mod(GM.prepared(M, Rb, Cb, S.rows, S.cols, B), S.p).reshape(nI * nJ * T, S.total)
    plain = S.plain(w, False)
    pool = ctx.alloc(nJ * nb * count * ctb)
    for J in range(nJ):
        ctx.ct_rotations_dev([None] + [mats[j] for j in range(1, nb)], [S.rotation_k(j) for j in range(nb)], LOGQ, View(src, J * count * ctb), NL, count,
                             View(pool, J * nb * count * ctb), NL)
    a_idx, b_idx, seg = [], [], [0]
    for Ib in range(nI):
        for g in range(G):
            for i in range(count):
                for J in range(nJ):
                    for j in range(B):
                        if g * B + j < T:
                            a_idx.append((J * nb + j) * count + i)
                            b_idx.append((Ib * nJ + J) * T + g * B + j)
                seg.append(len(a_idx))
    inner = ctx.alloc(nI * G * count * ctb)
    ctx.ct_plain_sum_dev(plain, LOGQ, pool, nJ * nb * count, NL, a_idx, b_idx, seg, inner)
    out, rot = ctx.alloc(nI * count * ctb), ctx.alloc(count * ctb)
    for Ib in range(nI):
        y = View(out, Ib * count * ctb)
        for g in range(G):
            ctx.ct_rotations_dev([mats[g * B] if g else None], [S.rotation_k(g * B)], LOGQ, View(inner, (Ib * G + g) * count * ctb), NL, count, rot if g else y, NL)
            if g:
                ctx.ct_add_dev(LOGQ, y, rot, 2, NL, count)
    folds = pl["amounts"][B - 1 + G - 1:]
    ctx.ct_rot_fold_dev([mats[a] for a in folds], [S.rotation_k(a) for a in folds], LOGQ, out, NL, nI * count, out)
    if bias is not None:
        for Ib in range(nI):
            vals = np.mod(bias[Ib * Rb:(Ib + 1) * Rb], S.p)[np.arange(S.total) % S.cols % Rb][None, :]
            S.ct_add_slots_dev(LOGQ, View(out, Ib * count * ctb), 2, NL, count, vals, only_usable=False)
    plain.close()
    return out.download((nI, count, 2, ctx.phim, NL))


WORDS = [((4, 16), (2, 2)), ((16, 4), (1, 3)), ((8, 8), (3, 2)), ((1, 8), (2, 2))]


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_grid_equals_the_composition_of_existing_calls(m):
    """(4,16) folds twice in a 2 x 2 grid, (16,4) is tall with three input blocks (the planner takes B = 1: giants only), (8,8) square in a 3 x 2 grid,
    (1,8) one diagonal and three folds; the planner's B and B = 3 (ragged); counts 1 and 3; with and without bias; the host and the device constructor"""
    ctx, S, _, mats = ring(m)
    n, top = ctx.phim, 3
    rng = np.random.default_rng(m + 1)
    for block, grid in WORDS:
        Rb, Cb, nI, nJ, R, C = shape_of(block, grid)
        a = np.stack([inputs(rng, top, n, NL, LOGQ) for _ in range(nJ)])                 # [nJ][top]
        src = ctx.upload(a)
        for baby in (0, 3):
            M = rng.integers(-S.p, 2 * S.p, size=(R, C)).astype(np.int64)
            for bias in (None, rng.integers(-S.p, 2 * S.p, size=R).astype(np.int64)):
                want = composition(ctx, S, mats, M, bias, block, baby, src, top)
                host = S.linear_grid(M, bias, block, baby)
                dev = S.linear_grid(DevTensor(ctx, M), None if bias is None else DevTensor(ctx, bias), block, baby, device=True)
                pl = GM.plan(S.cols, R, C, Rb, Cb, baby)
                assert host.amounts == dev.amounts == pl["amounts"] and set(pl["amounts"]) <= {1, 2, 3, 4, 6, 8}
                assert host.has_bias == (bias is not None) and host.key_switches == pl["key_switches"]
                for lin, counts in ((host, (1, top)), (dev, (top,))):
                    for count in counts:
                        out = ctx.alloc(nI * count * 2 * n * NL * 8)
                        lin.apply(mats, LOGQ, ctx.upload(a[:, :count]), NL, count, out)
                        assert np.array_equal(out.download((nI, count, 2, n, NL)), want[:, :count]), (block, grid, baby, bias is not None, lin is dev, count)
                    lin.close()


def test_a_one_by_one_grid_returns_the_words_of_the_layer():
    ctx, S, _, mats = ring(4096)
    n, count = ctx.phim, 3
    rng = np.random.default_rng(88)
    M, b = rng.integers(-S.p, 2 * S.p, size=(8, 8)).astype(np.int64), rng.integers(-S.p, 2 * S.p, size=8).astype(np.int64)
    src = ctx.upload(inputs(rng, count, n, NL, LOGQ))
    outs = []
    for lin in (S.linear(M, b), S.linear_grid(M, b, (8, 8)), S.linear_grid(M, b)):
        out = ctx.alloc(count * 2 * n * NL * 8)
        lin.apply(mats, LOGQ, src, NL, count, out)
        outs.append(out.download((count, 2, n, NL)))
        lin.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ through the scheme
def test_grid_through_the_scheme():
    """(4096, 65537, logQ 128), two-row space, two items: every decrypted slot of every output block = (M x_r + b)[I Rb + (i mod Rb)]; the noise budgets
    of the grid are positive; the budget of one layer per block plus additions on the same inputs is printed beside them"""
    ctx, S, (sk1, pk0, pk1), mats = ring(4096)
    p, n, count = S.p, S.total, 2
    rng = np.random.default_rng(9)
    ctb = 2 * n * NL * 8
    for block, grid in (((8, 8), (2, 2)), ((4, 16), (2, 2))):
        Rb, Cb, nI, nJ, R, C = shape_of(block, grid)
        M, b = rng.integers(0, p, size=(R, C)), rng.integers(0, p, size=R)
        x = rng.integers(0, p, size=(count, S.rows, C))
        xs = S.replicate_blocks(x, Cb)
        assert xs.shape == (nJ, count, n) and all(I(xs[J][1]) == I(GM.replicate_blocks(x[1], Cb, S.rows, S.cols)[J]) for J in range(nJ))
        cx, out = ctx.alloc(nJ * count * ctb), ctx.alloc(nI * count * ctb)
        S.encrypt_batch_seeded(pk0, pk1, LOGQ, 5000 + Rb, 0, xs.reshape(nJ * count, n), cx, NL, only_usable=False)
        lin = S.linear_grid(M, b, block)
        lin.apply(mats, LOGQ, cx, NL, count, out)
        got = S.decrypt_batch(sk1, LOGQ, out, NL, nI * count, only_usable=False).reshape(nI, count, n)
        for i in range(count):
            want = GM.expected_slots(M, b, x[i], Rb, p, S.rows, S.cols)
            for Ib in range(nI):
                assert I(got[Ib][i]) == want[Ib], (block, grid, Ib, i)
        y = S.collect_blocks(got, Rb)
        assert y.shape == (count, S.rows, R) and all(I(y[i][r]) == LM.brute(M, b, x[i], p)[r] for i in range(count) for r in range(S.rows))
        budget = np.asarray(S.noise_budget(sk1, LOGQ, out, NL, nI * count))
        lin.close()
        # one layer per block and the additions between them, on the same inputs
        per, tmp = ctx.alloc(nI * count * ctb), ctx.alloc(count * ctb)
        for Ib in range(nI):
            for J in range(nJ):
                one = S.linear(M[Ib * Rb:(Ib + 1) * Rb, J * Cb:(J + 1) * Cb], b[Ib * Rb:(Ib + 1) * Rb] if J == 0 else None)
                one.apply(mats, LOGQ, View(cx, J * count * ctb), NL, count, tmp if J else View(per, Ib * count * ctb))
                if J:
                    ctx.ct_add_dev(LOGQ, View(per, Ib * count * ctb), tmp, 2, NL, count)
                one.close()
        assert np.array_equal(S.decrypt_batch(sk1, LOGQ, per, NL, nI * count, only_usable=False).reshape(nI, count, n), got)
        per_budget = np.asarray(S.noise_budget(sk1, LOGQ, per, NL, nI * count))
        print("noise budget after the %d x %d matrix in %d x %d blocks of %d x %d: grid" % (R, C, nI, nJ, Rb, Cb), budget, "one layer per block", per_budget)
        assert (budget > 0).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_condition_and_leave_the_context_working():
    ctx, S, _, mats = ring(4096)
    n, count = ctx.phim, 2
    ctb = 2 * n * NL * 8
    rng = np.random.default_rng(3)
    block = (4, 16)
    M, b = rng.integers(0, S.p, size=(8, 32)), rng.integers(0, S.p, size=8)
    lin = S.linear_grid(M, b, block)
    assert lin.amounts == [1, 2, 8, 4] and (lin.nI, lin.nJ) == (2, 2)
    good_mats = [mats[a] for a in lin.amounts]
    src = ctx.upload(np.stack([inputs(rng, count, n, NL, LOGQ) for _ in range(2)]))
    out = ctx.alloc(2 * count * ctb)

    def call(hs=good_mats, s=src, o=out, l=lin, **kw):
        l.apply(hs, LOGQ, s, NL, count, o, **kw)
        return o.download((2, count, 2, n, NL))

    good = call()

    def refused(word, fn):
        with pytest.raises(F.FhesiError) as e:
            fn()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(call(), good), word               # a following good call returns the same words

    ones = lambda R, C: np.ones((R, C), dtype=np.int64)
    # the grid: not whole blocks; a block outside the planner's rules, in the planner's own words; too many diagonals for one handle
    refused("R = 9 is not a multiple", lambda: S.linear_grid(ones(9, 32), block=block))
    refused("C = 40 is not a multiple", lambda: S.linear_grid(ones(8, 40), block=block))
    refused("C = 40 is not a multiple", lambda: S.linear_grid_diagonals(ones(8, 40), block))
    refused("linear_plan: min(R, C) = 3 does not divide max", lambda: S.linear_grid(ones(6, 8), block=(3, 4)))
    refused("linear_plan: max(R, C) = 2048 exceeds the row", lambda: S.linear_grid(ones(4, 4096), block=(4, 2048)))
    refused("linear_plan: C / R = 3 is not a power of two", lambda: F.linear_grid_plan(24, 8, 24, 4, 12))
    refused("at least 1", lambda: S.linear_grid(ones(0, 16), block=block))
    refused("per handle", lambda: F.linear_grid_plan(S.cols, 8 * S.cols, 9 * S.cols, S.cols, S.cols))
    # a null matrix, through the C ABI itself
    lib, h = F.Backend.lib(), ctypes.c_void_p()

    def null_matrix(fn):
        if fn(S.h, None, 8, 32, 4, 16, None, 0, ctypes.byref(h)) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("null matrix", lambda: null_matrix(lib.fhesi_linear_grid_create))
    refused("null matrix", lambda: null_matrix(lib.fhesi_linear_grid_create_dev))
    # the matrices: their count, their order, a missing one
    refused("matrices, the layer takes 4", lambda: call(hs=good_mats[:3]))
    refused("matrices, the layer takes 4", lambda: call(hs=good_mats + [mats[1]]))
    refused("hoisted for k=", lambda: call(hs=[mats[2], mats[1], mats[8], mats[4]]))
    refused("hoisted for k=", lambda: call(hs=[mats[1], mats[2], mats[4], mats[8]]))
    refused("no matrix", lambda: call(hs=[mats[1], None, mats[8], mats[4]]))
    # another context: a matrix, the grid itself
    primes, roots = P.chain_for(4096, LOGQ, S.p)
    other = F.Context(4096, primes, roots)
    SO = F.SlotSpace.pow2(other, S.p, S.generator)
    _, _, foreign = rotation_keys(other, LOGQ, [S.rotation_k(1)])
    foreign_lin = SO.linear_grid(M, b, block)
    refused("another context", lambda: call(hs=[foreign[0]] + good_mats[1:]))

    def foreign_grid():
        arr = (ctypes.c_void_p * 4)(*[x.h for x in good_mats])
        if lib.fhesi_ct_linear_grid_dev(ctx.h, foreign_lin.h, arr, 4, LOGQ, 3, src.ptr, NL, count, out.ptr) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("linear grid belongs to another context", foreign_grid)
    foreign_lin.close()
    # the buffers -- out over the SECOND input block, which a one-block check would miss --, the digits
    refused("overlaps", lambda: call(o=src))
    refused("overlaps", lambda: call(o=View(src, count * ctb)))
    refused("digits", lambda: call(decomp_bytes=2))
    lin.close()


def test_a_sum_past_the_capacity_of_the_chain_is_refused():
    """two primes just below 2^60 on (64, 257), logQ 105: one product needs 118 bits, a sum of 2 needs 119, a sum of 4 needs 120 -- and the chain's 120
    (in double precision) must EXCEED what a sum needs.  Blocks of 1 x 1 take no matrix, and their sums have nJ terms: the 1 x 2 grid runs, the 1 x 4 grid
    is refused before anything is launched"""
    logQ = 105
    primes, roots = P.first_primes(64, 2)
    ctx = F.Context(64, primes, roots)
    S = F.SlotSpace.pow2(ctx, 257, 3)
    n, count = ctx.phim, 2
    assert [int(np.ceil(F.plain_sum_bits(64, logQ, 256, t))) for t in (1, 2, 4)] == [118, 119, 120] and int(sum(np.log2(float(q)) for q in primes)) == 120
    rng = np.random.default_rng(4)
    src = ctx.upload(np.stack([inputs(rng, count, n, NL, logQ) for _ in range(4)]))
    out = ctx.alloc(count * 2 * n * NL * 8)
    two = S.linear_grid(np.array([[3, -4]], dtype=np.int64), None, (1, 1))
    four = S.linear_grid(np.array([[3, -4, 5, 6]], dtype=np.int64), None, (1, 1))

    def run(lin):
        lin.apply([], logQ, src, NL, count, out)
        return out.download((count, 2, n, NL))

    good = run(two)
    with pytest.raises(F.FhesiError, match="a sum of 4 products needs 120 bits, the chain holds 120"):
        run(four)
    assert np.array_equal(run(two), good)
    two.close()
    four.close()
