"""GPU: the 64-bit element-wise kernels (kernels_ew.hip: ew_op_kernel, ew_scalar_kernel, ew_exp_kernel, tensor2x2_kernel) and the Barrett
reduction under them (d_barrett128, fhesi_internal.h: its shift counts depend on the bit length of q) on a chain that mixes every admitted prime
size, on rows of extreme residues -- (q - 1) (q - 1), (q - 1) + (q - 1), 0 - (q - 1) -- and fhesi_rows_op_dev, the batched DoubleCRT::Op.
Expected values are plain Python integers (%, pow); the C oracle is asserted in addition where it has the call.  Bit-exact."""
import numpy as np
import pytest

import fhe_si_amd as F
import long_sums_common as C
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu
BITS = (20, 31, 32, 33, 48, 59, 60)
SUBSET = [1, 4, 6]                                  # a proper index set: prime_of_slot is non-null in the kernels
PATTERNS = ("max", "alternating", "ones", "zeros", "single", "uniform")
OPS = {F.OP_ADD: lambda x, y, q: (x + y) % q, F.OP_SUB: lambda x, y, q: (x - y) % q, F.OP_MUL: lambda x, y, q: x * y % q}


def mixed_chain(m):
    pr = [P.first_primes(m, 1, bits) for bits in BITS]
    primes, roots = [x[0][0] for x in pr], [x[1][0] for x in pr]
    assert [q.bit_length() for q in primes] == list(BITS)
    return primes, roots


def pattern_rows(primes, n, rng):
    """name -> [L][n] rows of Python integers (object arrays), following test_tile_rows_across_prime_sizes"""
    rows = {k: np.zeros((len(primes), n), dtype=object) for k in PATTERNS}
    for i, q in enumerate(primes):
        rows["max"][i, :] = q - 1
        rows["alternating"][i, 0::2] = q - 1
        rows["ones"][i, :] = 1
        rows["single"][i, n - 1] = q - 1
        rows["uniform"][i, :] = [int(v) for v in rng.integers(0, q, n)]
    return rows


def u64(rows):
    return np.ascontiguousarray(rows.astype(np.uint64))


def dev(ctx, rows, idx=None):
    """the DoubleCRT over the index set idx whose row of prime i is rows[i]"""
    d = F.DoubleCRT(ctx, idx)
    r = u64(rows)
    for i in (range(ctx.L) if idx is None else idx):
        d.set_row(i, r[i])
    return d


def same(d, want, idx=None):
    return np.array_equal(d.rows(), u64(want)[list(range(want.shape[0])) if idx is None else idx])


def setup(m):
    primes, roots = mixed_chain(m)
    ctx = F.Context(m, primes, roots)
    rows = pattern_rows(primes, ctx.phim, np.random.default_rng(m))
    return ctx, primes, rows


def per_prime(primes, f, *rows):
    """f(x..., q) element by element, prime by prime, on Python integers"""
    out = np.zeros(rows[0].shape, dtype=object)
    for i, q in enumerate(primes):
        out[i] = [f(*xs, q) for xs in zip(*(r[i] for r in rows))]
    return out


@pytest.mark.parametrize("m", [32, 4096])           # n = 16: less than one wave; n = 2048: several blocks per row
def test_op_on_every_ordered_pair_of_extreme_rows(m):
    ctx, primes, rows = setup(m)
    orc = O.Oracle(m, primes, ctx.roots)
    full = {k: dev(ctx, rows[k]) for k in PATTERNS}
    part = {k: dev(ctx, rows[k], SUBSET) for k in PATTERNS}
    for op, f in OPS.items():
        for x in PATTERNS:
            for y in PATTERNS:
                want = per_prime(primes, f, rows[x], rows[y])
                assert same(full[x].copy().op(full[y], op), want), (op, x, y)
                assert same(part[x].copy().op(part[y], op), want, SUBSET), (op, x, y, "subset")
                if (x, y) in (("max", "max"), ("zeros", "max"), ("uniform", "uniform")):
                    assert np.array_equal(orc.dcrt_op(u64(rows[x]), u64(rows[y]), op), u64(want)), (op, x, y, "oracle")
    for k in PATTERNS:                              # the operands themselves were never written
        assert same(full[k], rows[k]) and same(part[k], rows[k], SUBSET)


@pytest.mark.parametrize("m", [32, 4096])
def test_op_scalar_at_the_top_of_every_residue_range(m):
    ctx, primes, rows = setup(m)
    Q = 1
    for q in primes:
        Q *= q
    nlimbs = Q.bit_length() // 64 + 1               # Q - 1 as a non-negative two's complement number
    scalars = (Q - 1, 0, 1, -1)                     # Q - 1 = q_i - 1 modulo every q_i at once (CRT)
    assert all((Q - 1) % q == q - 1 for q in primes)
    for k in PATTERNS:
        bases = [(idx, dev(ctx, rows[k], idx)) for idx in (None, SUBSET)]
        for s in scalars:
            for op, f in OPS.items():
                want = per_prime(primes, lambda x, q: f(x, s % q, q), rows[k])
                for idx, base in bases:
                    assert same(base.copy().op_scalar(s, op, nlimbs), want, idx), (k, s, op, idx)
            want = per_prime(primes, lambda x, q: s % q, rows[k])
            for idx, base in bases:
                assert same(base.copy().op_scalar(s, F.OP_SET, nlimbs), want, idx), (k, s, "set", idx)
        for s in (Q - 1, -1):                       # DoubleCRT /= a scalar that is q_i - 1 modulo every prime
            want = per_prime(primes, lambda x, q: x * pow(s % q, -1, q) % q, rows[k])
            for idx, base in bases:
                assert same(base.copy().op_scalar(s, F.OP_DIV, nlimbs), want, idx), (k, s, "div", idx)
    with pytest.raises(F.FhesiError):
        dev(ctx, rows["max"]).op_scalar(Q, F.OP_DIV, nlimbs)


@pytest.mark.parametrize("m", [32, 4096])
def test_exp_on_extreme_rows(m):
    ctx, primes, rows = setup(m)
    orc = O.Oracle(m, primes, ctx.roots)
    memo = {}

    def power(x, q, e):
        if (x, q) not in memo:
            memo[x, q] = pow(x, e, q)
        return memo[x, q]

    for e in (2, min(primes) - 2, (1 << 63) - 1):
        memo.clear()
        for idx in (None, SUBSET):
            for k in PATTERNS:
                want = per_prime(primes, lambda x, q: power(x, q, e), rows[k])
                assert same(dev(ctx, rows[k], idx).exp(e), want, idx), (e, k, idx)
        assert np.array_equal(orc.dcrt_exp(u64(rows["max"]), e), u64(per_prime(primes, lambda x, q: power(x, q, e), rows["max"]))), e
    # e = -1: the inverse where it exists, NTL's InvMod error where an element is zero
    nonzero = rows["uniform"].copy()
    nonzero[nonzero == 0] = 1
    for idx in (None, SUBSET):
        for name, r in (("max", rows["max"]), ("ones", rows["ones"]), ("nonzero", nonzero)):
            want = per_prime(primes, lambda x, q: pow(x, -1, q), r)
            inv = dev(ctx, r, idx).exp(-1)
            assert same(inv, want, idx), (name, idx)
            assert same(inv.op(dev(ctx, r, idx), F.OP_MUL), rows["ones"], idx), (name, idx)
        for k in ("alternating", "zeros", "single"):
            with pytest.raises(F.FhesiError, match="inverse undefined"):
                dev(ctx, rows[k], idx).exp(-1)


@pytest.mark.parametrize("m", [32, 4096])
def test_rows_op_is_the_batched_op(m):
    """fhesi_rows_op_dev on [count][L][n] buffers: the prime of a row is its index modulo L"""
    ctx, primes, rows = setup(m)
    pairs = [("max", "max"), ("zeros", "max"), ("alternating", "single")]      # (q-1) op (q-1), 0 op (q-1), and two sparse patterns
    dst = np.stack([u64(rows[x]) for x, _ in pairs])
    src = np.stack([u64(rows[y]) for _, y in pairs])
    dsrc = ctx.upload(src)
    for op, f in OPS.items():
        buf = ctx.upload(dst)
        ctx.rows_op(buf, dsrc, len(pairs), op)
        got = buf.download(dst.shape)
        for c, (x, y) in enumerate(pairs):
            assert np.array_equal(got[c], u64(per_prime(primes, f, rows[x], rows[y]))), (op, x, y)
            assert np.array_equal(got[c], dev(ctx, rows[x]).op(dev(ctx, rows[y]), op).rows()), (op, x, y, "object by object")
        assert np.array_equal(dsrc.download(src.shape), src)
    uni = np.stack([u64(rows["uniform"])] * 3)                                 # ... and the same on uniform rows
    buf = ctx.upload(uni)
    ctx.rows_op(buf, dsrc, 3, F.OP_MUL)
    got = buf.download(uni.shape)
    for c, (_, y) in enumerate(pairs):
        assert np.array_equal(got[c], u64(per_prime(primes, OPS[F.OP_MUL], rows["uniform"], rows[y]))), y
    for op in (-1, 3, F.OP_SET):
        with pytest.raises(F.FhesiError):
            ctx.rows_op(buf, dsrc, 3, op)
    assert np.array_equal(buf.download(uni.shape), got)                        # a refused call wrote nothing


@pytest.mark.parametrize("m", [32, 4096])
def test_ct_mul_dev_on_rows_of_q_minus_1(m):
    """tensor2x2_kernel on a chain of two 60-bit primes: ciphertext 0 is the crafted pair of constant polynomials (every evaluation of the lifted
    left operand and of the right operand is q - 1), 1 is the crafted left operand against a random right one, 2 is random"""
    p, logQ, nl = 23, 128, 2
    primes, roots = P.first_primes(m, 2, 60)
    ctx = F.Context(m, primes, roots)
    orc = O.Oracle(m, primes, roots)
    n, L = ctx.phim, 2
    rng = np.random.default_rng(m)
    c, d = C.crafted_constants(p, *primes)
    assert c < 1 << 120
    a = P.rand_limbs(rng, (3, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (3, 2, n), nl, logQ)
    a[0] = a[1] = C.constant_ct(n, nl, c, c)
    b[0] = C.constant_ct(n, nl, d, -1)
    tp = ctx.alloc(3 * 3 * L * n * 8)
    ctx.ct_mul_dev(p, ctx.upload(a), ctx.upload(b), nl, 3, tp)
    got = tp.download((3, 3, L, n))
    for ct in range(3):
        # evaluation rows as Python integers: DoubleCRT(a_i * p) and DoubleCRT(b_j) (Ciphertext.cpp:169-176)
        ea = [orc.dcrt_from_poly(O.ints_to_limbs([v * p for v in O.limbs_to_ints(a[ct, i])], nl + 1)).astype(object) for i in range(2)]
        eb = [orc.dcrt_from_poly(b[ct, j]).astype(object) for j in range(2)]
        if ct < 2:
            assert all((ea[i][r] == q - 1).all() for i in range(2) for r, q in enumerate(primes))
        for r, q in enumerate(primes):
            want = [ea[0][r] * eb[0][r] % q, (ea[0][r] * eb[1][r] + ea[1][r] * eb[0][r]) % q, ea[1][r] * eb[1][r] % q]
            if ct == 0:
                assert [set(w) for w in want] == [{1}, {2}, {1}]              # (q - 1)^2 = 1, the middle part 2 (q - 1)^2 = 2
            for k in range(3):
                assert np.array_equal(got[ct, k, r], want[k].astype(np.uint64)), (ct, k, r)
        assert np.array_equal(got[ct], orc.ct_mul(a[ct], b[ct], p)), ct
