"""GPU: dense linear layers on packed slots (fhesi_linear_*, fhesi_ct_rot_fold_dev, fhesi_ct_linear_dev) through the C ABI -- the diagonals
linear_diag_kernel writes against the model of tests/linear_model.py without any key, the fold and the layer word for word against the compositions
they are defined as, the layer through the scheme and over a slot basis, and the refusals.  Exact throughout."""
import ctypes
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import linear_model as LM
import params as P
from bsgs_common import inputs, rotation_keys
from slots_common import I, View, context

pytestmark = pytest.mark.gpu
LOGQ, NL = 128, 2
RINGS = {4096: (65537, 3),                 # the two largest chain primes, limbs
         1 << 15: (65537, 3)}              # four 30-bit primes on rows of 2^14
LAYER_AMOUNTS = (1, 2, 3, 4, 6, 8)         # every baby, giant and fold amount of the shapes below with the planner's B and with B = 3


class DevTensor:
    """an int64 array in HBM with the three things SlotSpace.linear(device=True) asks of a tensor"""

    def __init__(self, ctx, a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        self.buf, self.shape, self.dtype = ctx.upload(a), a.shape, "int64"

    def data_ptr(self):
        return self.buf.ptr.value

    def is_contiguous(self):
        return True


def planted(rng, p, R, C):
    """any int64: uniform over a few p either side of 0, with 0, p - 1, p, -1, -p and +-2^62 planted where the matrix has room"""
    M = rng.integers(-3 * p, 3 * p, size=(R, C)).astype(np.int64)
    flat = M.reshape(-1)
    special = [0, p - 1, p, -1, -p, 1 << 62, -(1 << 62)]
    for i, v in zip(rng.permutation(flat.size)[:len(special)], special):
        flat[i] = v
    return M


# ------------------------------------------------------------------------------------------------ the diagonals, no keys
def check_diagonals(S, shapes, seed):
    rng = np.random.default_rng(seed)
    rows, cols = max(S.rows, 1), S.total // max(S.rows, 1)
    for R, C in shapes:
        M = planted(rng, S.p, R, C)
        if R * C >= 7:
            assert (M < 0).any() and (M == 0).any() and (M == S.p).any() and (abs(M) == 1 << 62).any()
        for baby in (0, 3):
            pl = F.linear_plan(cols, R, C, baby)
            assert pl == LM.plan(cols, R, C, baby)
            want = np.asarray(LM.prepared(M, rows, cols, pl["B"]), dtype=object) % S.p
            got = S.linear_diagonals(M, baby)
            assert got.shape == (pl["T"], S.total) and np.array_equal(got.astype(object), want), (R, C, baby)


def test_diagonals_equal_the_model_on_a_two_row_ring():
    """m = 64, p = 257, g = 3: two rows of 16 -- both rows, replication (D < cols) and the full row (D = cols); baby = 3 gives a ragged last giant and
    a negative wrap of i - g B"""
    big, _ = context(64, LOGQ, 257)
    SB = F.SlotSpace.pow2(big, 257, 3)
    assert (SB.rows, SB.cols, SB.total) == (2, 16, 32)
    check_diagonals(SB, [(1, 1), (1, 16), (16, 1), (4, 4), (2, 8), (8, 2), (4, 16), (16, 16)], 64)
    # the host and the device constructor: a layer that takes no matrix (1 x 1: one diagonal, no fold) applied to the same words
    n, count = big.phim, 2
    M, b = np.array([[-5]], dtype=np.int64), np.array([300], dtype=np.int64)
    src = big.upload(inputs(np.random.default_rng(1), count, n, NL, LOGQ))
    outs = []
    for lin in (SB.linear(M, b), SB.linear(DevTensor(big, M), DevTensor(big, b), device=True)):
        assert (lin.R, lin.C, lin.T, lin.B, lin.G, lin.nfold, lin.amounts, lin.has_bias) == (1, 1, 1, 1, 1, 0, [], True)
        out = big.alloc(count * 2 * n * NL * 8)
        lin.apply([], LOGQ, src, NL, count, out)
        outs.append(out.download((count, 2, n, NL)))
        lin.close()
    assert np.array_equal(outs[0], outs[1])
    want = big.alloc(count * 2 * n * NL * 8)
    SB.matvec_bsgs([None], [None], 1, SB.plain(np.full((1, SB.total), (-5) % 257), False), LOGQ, src, NL, count, want)
    SB.ct_add_slots_dev(LOGQ, want, 2, NL, count, np.full((1, SB.total), 300 % 257), only_usable=False)
    assert np.array_equal(outs[0], want.download((count, 2, n, NL)))


def test_diagonals_equal_the_model_on_a_single_row_ring():
    """m = 257 (prime), p = 1543 = 6 * 257 + 1, g = 3 of order 256: one row of 256 slots through the chirp embedding's space"""
    ctx, _ = context(257, 64, 1543)
    S = F.SlotSpace(ctx, 1543, 3)
    assert (max(S.rows, 1), S.total) == (1, 256)
    check_diagonals(S, [(4, 64), (256, 256)], 257)


# ------------------------------------------------------------------------------------------------ the fold against its definition
@pytest.mark.parametrize("m,p", [(64, 257), (250, 251), (4096, 65537)])
def test_fold_equals_rotations_and_additions_per_step(m, p):
    """1, 2 and 5 steps (the fifth list holds a step without a matrix, k = 1: y <- 2 y), counts 1 and 3, the two extremes planted; out == in; and
    the evaluation-row route of `>>=`"""
    primes, roots = P.chain_for(m, LOGQ, p)
    ctx = F.Context(m, primes, roots)
    n, top = ctx.phim, 3
    ctb = 2 * n * NL * 8
    _, autos, hoisted = rotation_keys(ctx, LOGQ, (3, 9))
    mats = {3: hoisted[0], 9: hoisted[1], 1: None}
    a = inputs(np.random.default_rng(m), top, n, NL, LOGQ)
    for ks in ([3], [3, 9], [9, 3, 1, 3, 9]):
        y, rot = ctx.upload(a), ctx.alloc(top * ctb)
        for k in ks:
            ctx.ct_rotations_dev([mats[k]], [k], LOGQ, y, NL, top, rot, NL)
            ctx.ct_add_dev(LOGQ, y, rot, 2, NL, top)
        want = y.download((top, 2, n, NL))
        hs = [mats[k] for k in ks]
        for count in (1, top):
            out = ctx.alloc(count * ctb)
            ctx.ct_rot_fold_dev(hs, ks, LOGQ, ctx.upload(a[:count]), NL, count, out)
            assert np.array_equal(out.download((count, 2, n, NL)), want[:count]), (ks, count)
        both = ctx.upload(a)
        ctx.ct_rot_fold_dev(hs, ks, LOGQ, both, NL, top, both)
        assert np.array_equal(both.download((top, 2, n, NL)), want), (ks, "out == in")
        ctx.set_option("automorph_rows", 1)
        out = ctx.alloc(top * ctb)
        ctx.ct_rot_fold_dev(hs, ks, LOGQ, ctx.upload(a), NL, top, out)
        ctx.set_option("automorph_rows", 0)
        assert np.array_equal(out.download((top, 2, n, NL)), want), (ks, "automorph_rows")
    # no step: the reduced copy
    out = ctx.alloc(top * ctb)
    ctx.ct_rot_fold_dev([], [], LOGQ, ctx.upload(a), NL, top, out)
    assert np.array_equal(out.download((top, 2, n, NL)), a)


# ------------------------------------------------------------------------------------------------ the layer against its definition
@functools.lru_cache(maxsize=None)
def ring(m):
    """one context, its two-row space, keys made on the device and the hoisted matrices by amount; m = 4096 also carries the amounts of a total sum"""
    p, g = RINGS[m]
    primes, roots = P.chain_for(m, LOGQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    amounts = list(LAYER_AMOUNTS)
    if m == 4096:
        amounts += [1 << e for e in range(4, 10)] + ["swap"]
    keys, autos, hoisted = rotation_keys(ctx, LOGQ, [S.rotation_k(a) for a in amounts])
    return ctx, S, keys, dict(zip(amounts, hoisted))


def composition(ctx, S, mats, M, bias, baby, src, count):
    """fhesi_ct_matvec_bsgs_dev with the plaintext SlotSpace.plain makes of the model's diagonals, fhesi_ct_rot_fold_dev over the fold amounts,
    fhesi_ct_add_slots_dev with the replicated bias"""
    R, C = M.shape
    pl = LM.plan(S.cols, R, C, baby)
    B, G = pl["B"], pl["G"]
    e = np.mod(LM.diagonals(M, S.rows, S.cols), S.p)
    plain = S.plain(S.bsgs_diagonals(e, B), False)
    out = ctx.alloc(count * 2 * ctx.phim * NL * 8)
    S.matvec_bsgs([None] + [mats[j] for j in range(1, B)], [None] + [mats[g * B] for g in range(1, G)], B, plain, LOGQ, src, NL, count, out)
    folds = pl["amounts"][B - 1 + G - 1:]
    ctx.ct_rot_fold_dev([mats[a] for a in folds], [S.rotation_k(a) for a in folds], LOGQ, out, NL, count, out)
    if bias is not None:
        S.ct_add_slots_dev(LOGQ, out, 2, NL, count, np.mod(bias, S.p)[np.arange(S.total) % S.cols % R][None, :], only_usable=False)
    plain.close()
    return out.download((count, 2, ctx.phim, NL))


@pytest.mark.parametrize("m", sorted(RINGS))
def test_layer_equals_the_three_call_composition(m):
    """(4,16) folds twice, (16,4) is tall, (8,8) square, (1,8) one diagonal and three folds; the planner's B and B = 3 (ragged); counts 1 and 5; with and
    without bias; the host and the device constructor"""
    ctx, S, _, mats = ring(m)
    n, top = ctx.phim, 5
    rng = np.random.default_rng(m)
    a = inputs(rng, top, n, NL, LOGQ)
    src = ctx.upload(a)
    for R, C in ((4, 16), (16, 4), (8, 8), (1, 8)):
        for baby in (0, 3):
            M = rng.integers(-S.p, 2 * S.p, size=(R, C)).astype(np.int64)
            for bias in (None, rng.integers(-S.p, 2 * S.p, size=R).astype(np.int64)):
                want = composition(ctx, S, mats, M, bias, baby, src, top)
                host = S.linear(M, bias, baby)
                dev = S.linear(DevTensor(ctx, M), None if bias is None else DevTensor(ctx, bias), baby, device=True)
                assert host.amounts == dev.amounts == LM.plan(S.cols, R, C, baby)["amounts"] and host.has_bias == (bias is not None)
                for lin, counts in ((host, (1, top)), (dev, (top,))):
                    for count in counts:
                        out = ctx.alloc(count * 2 * n * NL * 8)
                        lin.apply(mats, LOGQ, ctx.upload(a[:count]), NL, count, out)
                        assert np.array_equal(out.download((count, 2, n, NL)), want[:count]), (R, C, baby, bias is not None, lin is dev, count)
                    lin.close()


# ------------------------------------------------------------------------------------------------ through the scheme
def test_layer_and_total_sum_through_the_scheme():
    """(4096, 65537, logQ 128), two-row space, two ciphertexts: slot (r, i) of the output decrypts to (M x_r + b)[i mod R]; the fold over cols/2 .. 1
    and the row swap leaves the sum of all n slots in every slot"""
    ctx, S, (sk1, pk0, pk1), mats = ring(4096)
    p, n, count = S.p, S.total, 2
    rng = np.random.default_rng(7)
    words = 2 * n * NL
    for R, C in ((4, 16), (16, 4)):
        M, b = rng.integers(0, p, size=(R, C)), rng.integers(0, p, size=R)
        x = rng.integers(0, p, size=(count, S.rows, C))
        xs = S.replicate(x, C)
        assert xs.shape == (count, n) and I(xs[1]) == I(LM.replicate(x[1], C, S.rows, S.cols))
        cx, out = ctx.alloc(count * words * 8), ctx.alloc(count * words * 8)
        S.encrypt_batch_seeded(pk0, pk1, LOGQ, 4096, 0, xs, cx, NL, only_usable=False)
        lin = S.linear(M, b)
        lin.apply(mats, LOGQ, cx, NL, count, out)
        got = S.decrypt_batch(sk1, LOGQ, out, NL, count, only_usable=False)
        for i in range(count):
            assert I(got[i]) == LM.expected_slots(M, b, x[i], p, S.rows, S.cols), (R, C, i)
        budget = np.asarray(S.noise_budget(sk1, LOGQ, out, NL, count))
        print("noise budget after the %d x %d layer:" % (R, C), budget)
        assert (budget > 0).all()
        lin.close()
    # total sums
    v = rng.integers(0, p, size=(count, n))
    cx = ctx.alloc(count * words * 8)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 4097, 0, v, cx, NL, only_usable=False)
    amounts = [S.cols >> e for e in range(1, S.cols.bit_length())] + ["swap"]
    assert amounts[0] == S.cols // 2 and amounts[-2] == 1
    S.fold([mats[a] for a in amounts], amounts, LOGQ, cx, NL, count, cx)
    got = S.decrypt_batch(sk1, LOGQ, cx, NL, count, only_usable=False)
    for i in range(count):
        assert I(got[i]) == [int(v[i].sum()) % p] * n, i
    budget = np.asarray(S.noise_budget(sk1, LOGQ, cx, NL, count))
    print("noise budget after the total sum:", budget)
    assert (budget > 0).all()


def test_a_layer_of_folds_only_in_chunks_of_one_ciphertext():
    """(4096, 65537, logQ 128), R = 1, C = 8 with a bias: B = G = 1 -- no baby, no giant, and every matrix of the run call goes to a fold; two ciphertexts
    in chunks of one ("wave_operands" 1).  The words of the three-call composition, and every decrypted slot the model's."""
    ctx, S, (sk1, pk0, pk1), mats = ring(4096)
    p, n, count = S.p, S.total, 2
    rng = np.random.default_rng(18)
    M, b = rng.integers(0, p, size=(1, 8)), rng.integers(1, p, size=1)
    x = rng.integers(0, p, size=(count, S.rows, 8))
    cx, out = ctx.alloc(count * 2 * n * NL * 8), ctx.alloc(count * 2 * n * NL * 8)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 4200, 0, S.replicate(x, 8), cx, NL, only_usable=False)
    lin = S.linear(M, b)
    assert (lin.T, lin.B, lin.G, lin.nfold, lin.amounts, lin.has_bias) == (1, 1, 1, 3, [4, 2, 1], True)
    want = composition(ctx, S, mats, M, b, 0, cx, count)
    ctx.set_option("wave_operands", 1)
    try:
        lin.apply(mats, LOGQ, cx, NL, count, out)
    finally:
        ctx.set_option("wave_operands", 0)
    assert np.array_equal(out.download((count, 2, n, NL)), want)
    got = S.decrypt_batch(sk1, LOGQ, out, NL, count, only_usable=False)
    for i in range(count):
        assert I(got[i]) == LM.expected_slots(M, b, x[i], p, S.rows, S.cols), i
    lin.close()


def test_layer_over_a_slot_basis():
    """two primes below 2^20 on m = 4096: a (4,16) layer of 12-bit weights and data -- the exact sums exceed either prime and stay inside (-P/2, P/2)"""
    m, g = 4096, 3
    primes = F.slots_basis_plan(m, 30, 20, g)["primes"]
    assert len(primes) == 2
    chain, roots = P.chain_for(m, LOGQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k, count, R, C = B.total, B.k, 2, 4, 16
    S0 = B.channel(0)
    rng = np.random.default_rng(11)
    M, b = rng.integers(0, 1 << 12, size=(R, C)), rng.integers(-(1 << 19), 1 << 19, size=R)
    layers = B.linear(M, b)
    amounts = layers[0].amounts
    assert amounts == [1, 2, 8, 4] and all(l.amounts == amounts for l in layers)
    (sk1, pk0, pk1), autos, hoisted = rotation_keys(ctx, LOGQ, [S0.rotation_k(a) for a in amounts])
    x = rng.integers(0, 1 << 12, size=(count, S0.rows, C))
    exact = [[[sum(int(M[r, c]) * int(x[i, row, c]) for c in range(C)) + int(b[r]) for r in range(R)] for row in range(S0.rows)] for i in range(count)]
    big = max(abs(v) for e in exact for row in e for v in row)
    assert big > max(primes) and big < B.modulus // 2
    words = 2 * n * NL
    cx, out = ctx.alloc(k * count * words * 8), ctx.alloc(k * count * words * 8)
    B.encrypt_batch_seeded(pk0, pk1, LOGQ, 77, 0, S0.replicate(x, C), cx, NL)
    B.linear_apply(layers, dict(zip(amounts, hoisted)), LOGQ, cx, NL, count, out)
    got = B.decrypt_batch(sk1, LOGQ, out, NL, count)
    for i in range(count):
        assert I(got[i]) == [exact[i][row][j % R] for row in range(S0.rows) for j in range(S0.cols)], i
    for l in layers:
        l.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_condition_and_leave_the_context_working():
    ctx, S, _, mats = ring(4096)
    n, count = ctx.phim, 2
    words = 2 * n * NL
    rng = np.random.default_rng(2)
    M, b = rng.integers(0, S.p, size=(4, 16)), rng.integers(0, S.p, size=4)
    lin = S.linear(M, b)
    assert lin.amounts == [1, 2, 8, 4]
    good_mats = [mats[a] for a in lin.amounts]
    src = ctx.upload(inputs(rng, count, n, NL, LOGQ))
    out = ctx.alloc(count * words * 8)

    def layer(hs=good_mats, s=src, o=out, l=lin, **kw):
        l.apply(hs, LOGQ, s, NL, count, o, **kw)
        return o.download((count, 2, n, NL))

    good = layer()

    def refused(word, call):
        with pytest.raises(F.FhesiError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(layer(), good), word             # a following good call returns the same words

    # shapes outside the rules (C / R = 3 2^j cannot meet D | cols on a row of 2^k slots: the planner itself is asked)
    refused("does not divide max", lambda: S.linear(np.ones((3, 4), dtype=np.int64)))
    refused("does not divide the row", lambda: S.linear(np.ones((3, 12), dtype=np.int64)))
    refused("exceeds the row", lambda: S.linear(np.ones((4, 2 * S.cols), dtype=np.int64)))
    refused("at least 1", lambda: S.linear(np.ones((0, 4), dtype=np.int64)))
    refused("at least 1", lambda: S.linear(np.ones((4, 0), dtype=np.int64)))
    refused("not a power of two", lambda: F.linear_plan(24, 4, 12))
    refused("does not divide max", lambda: S.linear_diagonals(np.ones((3, 4), dtype=np.int64)))
    # a null matrix, through the C ABI itself
    lib, h = F.Backend.lib(), ctypes.c_void_p()

    def null_matrix(fn):
        if fn(S.h, None, 4, 16, None, 0, ctypes.byref(h)) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("null matrix", lambda: null_matrix(lib.fhesi_linear_create))
    refused("null matrix", lambda: null_matrix(lib.fhesi_linear_create_dev))
    # the matrices
    refused("matrices, the layer takes 4", lambda: layer(hs=good_mats[:3]))
    refused("matrices, the layer takes 4", lambda: layer(hs=good_mats + [mats[1]]))
    refused("hoisted for k=", lambda: layer(hs=[mats[2], mats[1], mats[8], mats[4]]))
    refused("hoisted for k=", lambda: layer(hs=[mats[1], mats[2], mats[4], mats[8]]))
    refused("no matrix", lambda: layer(hs=[mats[1], None, mats[8], mats[4]]))
    # another context: a matrix, the layer itself
    primes, roots = P.chain_for(4096, LOGQ, S.p)
    other = F.Context(4096, primes, roots)
    SO = F.SlotSpace.pow2(other, S.p, S.generator)
    _, _, foreign = rotation_keys(other, LOGQ, [S.rotation_k(1)])
    foreign_lin = SO.linear(M, b)
    refused("another context", lambda: layer(hs=[foreign[0]] + good_mats[1:]))

    def foreign_layer():
        arr = (ctypes.c_void_p * 4)(*[x.h for x in good_mats])
        if lib.fhesi_ct_linear_dev(ctx.h, foreign_lin.h, arr, 4, LOGQ, 3, src.ptr, NL, count, out.ptr) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("linear layer belongs to another context", foreign_layer)
    foreign_lin.close()
    # the buffers, the digits
    refused("overlaps", lambda: layer(o=src))
    refused("digits", lambda: layer(decomp_bytes=2))
    # the fold refuses as the rotations do
    refused("no matrix", lambda: ctx.ct_rot_fold_dev([None], [S.rotation_k(1)], LOGQ, src, NL, count, out))
    refused("hoisted for k=", lambda: ctx.ct_rot_fold_dev([mats[1]], [S.rotation_k(2)], LOGQ, src, NL, count, out))
    refused("without being in", lambda: ctx.ct_rot_fold_dev([mats[1]], [S.rotation_k(1)], LOGQ, src, NL, 1, View(src, 64)))
    refused("digits", lambda: ctx.ct_rot_fold_dev([mats[1]], [S.rotation_k(1)], LOGQ, src, NL, count, out, decomp_bytes=2))
    lin.close()
