"""GPU: polynomial activations on packed slots (fhesi_ct_lin_comb_dev, fhesi_ct_poly_eval_dev) through the C ABI -- the scalar linear combination bit for
bit against the composition it is defined as (no keys), the evaluation word for word against the composition of public calls that tests/poly_model.py
states, through the scheme against f in every slot and against Horner, a three-layer network, over a slot basis, and the refusals.  Exact throughout."""
import ctypes
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import linear_model as LM
import oracle_lib as O
import params as P
import poly_model as PM
from bsgs_common import inputs, rotation_keys
from slots_common import I, View, context, device_keys

pytestmark = pytest.mark.gpu
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


def s2_matrix(ctx, logQ, sk1, seed):
    """the s^2 -> s matrix of the key sk1, made on the device"""
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (ctx.phim - 1), 1))
    return F.KeySwitchMatrix(ctx, 3, R.ndigits(logQ)).init_batch_seeded([one, sk1, sk1.copy().op(sk1, F.OP_MUL)], sk1, logQ, seed, seed ^ 0x5DEECE66D, 1000)


# ------------------------------------------------------------------------------------------------ the linear combination against its definition, no keys
def composed_lin_comb(ctx, logQ, p, pool, nl, a_idx, coef, seg, konst):
    """a copy of each operand, Ciphertext *= long, Ciphertext += per term; Ciphertext += ZZX with (konst[g], 0, .., 0)"""
    n, ngroups = ctx.phim, len(seg) - 1
    ctb = 2 * n * nl * 8
    acc, tmp = ctx.upload(np.zeros((ngroups, 2, n, nl), dtype=np.uint64)), ctx.alloc(ctb)
    for g in range(ngroups):
        for t in range(seg[g], seg[g + 1]):
            ctx.dev_copy(tmp.ptr.value, pool.ptr.value + int(a_idx[t]) * ctb, ctb)
            ctx.ct_mul_long_dev(logQ, tmp, int(coef[t]), 2, nl, 1)
            ctx.ct_add_dev(logQ, View(acc, g * ctb), tmp, 2, nl, 1)
    if konst is not None:
        poly = np.zeros((ngroups, n), dtype=np.int64)
        poly[:, 0] = konst
        ctx.ct_add_const_dev(logQ, p, acc, 2, nl, ngroups, poly)
    return acc.download((ngroups, 2, n, nl))


def lin_comb_groups(rng, p, npool):
    """empty with and without a constant, one term, 40 terms, an entry twice, every planted coefficient and constant"""
    planted = [0, 1, -1, p - 1, 1 << 62, -(1 << 62), I64MIN, I64MAX]
    groups = [([], p - 1), ([], 0), ([(-1, 0)], p),
              ([(planted[t % len(planted)] if t % 3 else int(rng.integers(-3 * p, 3 * p)), int(rng.integers(0, npool))) for t in range(40)], -1),
              ([(p - 1, 2), (I64MIN, 2), (3, 1)], 0)]
    groups += [([(c, (i + 1) % npool)], (0, p - 1, p, -1)[i % 4]) for i, c in enumerate(planted)]
    a_idx, coef, seg, konst = [], [], [0], []
    for terms, k in groups:
        coef += [c for c, _ in terms]
        a_idx += [i for _, i in terms]
        seg.append(len(a_idx))
        konst.append(k)
    return a_idx, coef, seg, konst


SHAPES = [(100, 2), (128, 2), (191, 3), (512, 8), (513, 9), (1024, 16), (1025, 17), (2047, 32)]       # each limb class at both of its edges


@pytest.mark.parametrize("m,shapes", [(64, SHAPES), (1024, [(128, 2), (513, 9)]), (4096, [(100, 2), (2047, 32)])])
def test_lin_comb_equals_its_composition(m, shapes):
    """m = 64: 32 coefficients, a partial block; 1024 and 4096: two and eight blocks a polynomial"""
    ctx, _ = context(m)
    n, npool = ctx.phim, 6
    for logQ, nl in shapes:
        for p in ((257, 65537) if m == 64 else (65537,)):
            rng = np.random.default_rng(m + logQ)
            pool = ctx.upload(inputs(rng, npool, n, nl, logQ))
            a_idx, coef, seg, konst = lin_comb_groups(rng, p, npool)
            for kn in (konst, None):
                want = composed_lin_comb(ctx, logQ, p, pool, nl, a_idx, coef, seg, kn)
                out = ctx.alloc(want.nbytes)
                ctx.ct_lin_comb_dev(logQ, p, pool, npool, nl, a_idx, coef, seg, kn, out)
                assert np.array_equal(out.download(want.shape), want), (m, logQ, nl, p, kn is None)
            if m == 64 and nl == 2:
                # (without constants the two empty groups are the zero ciphertext)
                assert not want[1].any() and not want[0].any()
    # no group at all, and groups without any term or pool
    out = ctx.alloc(2 * 2 * n * 2 * 8)
    ctx.ct_lin_comb_dev(128, 257, None, 0, 2, [], [], [0], None, out)
    ctx.ct_lin_comb_dev(128, 257, None, 0, 2, [], [], [0, 0, 0], [5, 0], out)
    got = out.download((2, 2, n, 2))
    # the trivial ciphertext of a constant: its scaled quotient in coefficient 0 of part 0 and nothing else
    assert O.limbs_to_ints(got[0, 0]) == [(5 << 128) // 257] + [0] * (n - 1) and not got[1].any() and not got[0, 1].any()


# ------------------------------------------------------------------------------------------------ the evaluation against its definition
LOGQ, NL, P0 = 128, 2, 65537


@functools.lru_cache(maxsize=None)
def ring(m):
    """one context, keys and the s^2 -> s matrix made on the device, three random ciphertexts: 4096 switches keys over limbs, 2^15 over four 30-bit primes"""
    primes, roots = P.chain_for(m, LOGQ, P0)
    ctx = F.Context(m, primes, roots)
    sk1, pk0, pk1 = device_keys(ctx, LOGQ, m)
    ksk = s2_matrix(ctx, LOGQ, sk1, m)
    a = inputs(np.random.default_rng(m), 3, ctx.phim, NL, LOGQ)
    return ctx, ksk, a


def composed_poly_eval(ctx, ksk, logQ, p, nl, coef, baby, src, count):
    """the schedule of the model through Context.ct_mul_sum_relin_dev and Context.ct_lin_comb_dev: entry e of item i at e count + i of one pool"""
    s = PM.schedule([int(c) for c in coef], p, baby)
    B, G = s["B"], s["G"]
    ctb = 2 * ctx.phim * nl * 8
    npowers, ninner = B + G - 2, len(s["inner"])
    entry = {("x", k): PM.pool_entry(k, B) for k in list(range(1, B + 1)) + [g * B for g in range(2, G)]}
    entry.update({("u", g): npowers + i for i, (g, _, _) in enumerate(s["inner"])})
    entry[("W",)] = npowers + ninner
    nent = npowers + ninner + 1
    pool = ctx.alloc(nent * count * ctb)
    ctx.dev_copy(pool.ptr.value, src.ptr.value, count * ctb)
    at = lambda ref, i: entry[ref] * count + i
    for level in s["levels"]:                                               # one wave of single products per level, all items
        ia = [at(("x", a), i) for _, a, _ in level for i in range(count)]
        ib = [at(("x", b), i) for _, _, b in level for i in range(count)]
        ctx.ct_mul_sum_relin_dev(ksk, logQ, p, pool, nl, ia, ib, list(range(len(ia) + 1)), View(pool, entry[("x", level[0][0])] * count * ctb))
    if s["inner"]:
        ia, cf, seg, kn = [], [], [0], []
        for g, terms, konst in s["inner"]:                                  # ALL inner sums in one call
            for i in range(count):
                ia += [at(("x", j), i) for _, j in terms]
                cf += [c for c, _ in terms]
                seg.append(len(ia))
                kn.append(konst)
        ctx.ct_lin_comb_dev(logQ, p, pool, npowers * count, nl, ia, cf, seg, kn, View(pool, npowers * count * ctb))
        ia, ib, seg = [], [], [0]
        for i in range(count):                                              # one group per item: one key switch
            ia += [at(("u", g), i) for g, _ in s["pairs"]]
            ib += [at(("x", k), i) for _, k in s["pairs"]]
            seg.append(len(ia))
        ctx.ct_mul_sum_relin_dev(ksk, logQ, p, pool, nl, ia, ib, seg, View(pool, entry[("W",)] * count * ctb))
    terms, konst = s["final"]
    ia, cf, seg = [], [], [0]
    for i in range(count):
        ia += [at(ref, i) for _, ref in terms]
        cf += [c for c, _ in terms]
        seg.append(len(ia))
    out = ctx.alloc(count * ctb)
    ctx.ct_lin_comb_dev(logQ, p, pool, nent * count, nl, ia, cf, seg, [konst] * count, out)
    return out.download((count, 2, ctx.phim, nl))


def check_poly_eval(m, cases):
    ctx, ksk, a = ring(m)
    n, top = ctx.phim, 3
    src = ctx.upload(a)
    for coef, baby, chunked in cases:
        want = composed_poly_eval(ctx, ksk, LOGQ, P0, NL, coef, baby, src, top)
        for count in (1, top):
            out = ctx.alloc(count * 2 * n * NL * 8)
            ctx.ct_poly_eval_dev(ksk, LOGQ, P0, coef, ctx.upload(a[:count]), NL, count, out, baby)
            assert np.array_equal(out.download((count, 2, n, NL)), want[:count]), (coef, baby, count)
        if chunked:                                                         # few operands a pass: the items go in chunks, the outer sum in pieces
            ctx.set_option("wave_operands", chunked)
            out = ctx.alloc(top * 2 * n * NL * 8)
            ctx.ct_poly_eval_dev(ksk, LOGQ, P0, coef, src, NL, top, out, baby)
            ctx.set_option("wave_operands", 0)
            assert np.array_equal(out.download((top, 2, n, NL)), want), (coef, baby, "chunks")


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_poly_eval_equals_the_composition_of_public_calls(m):
    """degrees 1, 2, 3, 7, 8, 16 with the planner's B, B = 1 (powers only), B = 3 (ragged) and B = d (one group); counts 1 and 3"""
    rng = np.random.default_rng(m + 1)
    cases = []
    for d in (1, 2, 3, 7, 8, 16):
        coef = [int(c) for c in rng.integers(-P0, 2 * P0, size=d + 1)]
        coef[rng.integers(0, d + 1)] = (1 << 62, -(1 << 62), I64MIN, I64MAX, -1, P0 - 1)[d % 6]
        for baby in sorted({0, 1, 3, d}):
            if baby <= d:
                cases.append((coef, baby, 0))
    check_poly_eval(m, cases)


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_poly_eval_zero_patterns_and_chunks(m):
    """a single monomial, c_d = 0 given as p, a middle group that is a constant alone, all zero; few operands a pass"""
    rng = np.random.default_rng(m + 2)
    dense7 = [int(c) for c in rng.integers(1, P0, size=8)]
    mid = [int(c) for c in rng.integers(1, P0, size=9)]
    mid[4] = mid[5] = 0                                                     # d = 8, B = 3: group 1 is c_3 alone
    cases = [([0] * 8 + [1], 0, 0), ([0] * 8 + [1], 3, 0), (dense7[:7] + [P0], 0, 0), (mid, 3, 5), ([0, P0, -P0, 0], 0, 0), (dense7, 0, 6), (dense7, 2, 4)]
    s = PM.schedule(mid, P0, 3)
    assert [g for g, _, _ in s["inner"]] == [2] and (mid[3], ("x", 3)) in [(c % P0, ref) for c, ref in s["final"][0]]
    check_poly_eval(m, cases)


# ------------------------------------------------------------------------------------------------ through the scheme
def f_of(coef, v, p):
    return sum(int(c) * pow(int(v), k, p) for k, c in enumerate(coef)) % p


def horner(ctx, ksk, logQ, p, nl, coef, x, count):
    """y = c_d x + c_(d-1), then y = y x + c_k: d - 1 dependent products, composed from public calls"""
    n, d = ctx.phim, len(coef) - 1
    ctb = 2 * n * nl * 8
    y, nxt = ctx.alloc(count * ctb), ctx.alloc(count * ctb)
    ctx.ct_lin_comb_dev(logQ, p, x, count, nl, list(range(count)), [coef[d]] * count, list(range(count + 1)), [coef[d - 1]] * count, y)
    for k in range(d - 2, -1, -1):
        ctx.ct_mul_relin_dev(ksk, logQ, p, y, x, nxt, nl, count)
        y, nxt = nxt, y
        poly = np.zeros((1, n), dtype=np.int64)
        poly[0, 0] = coef[k]
        ctx.ct_add_const_dev(logQ, p, y, 2, nl, count, poly)
    return y


@pytest.mark.parametrize("m,p,degrees", [(64, 257, (15,)), (4096, 65537, (7, 15))])
def test_poly_eval_through_the_scheme_against_f_and_horner(m, p, degrees):
    """every decrypted slot of every item equals f(v) mod p with a positive budget; Horner decrypts correctly wherever its budget is positive and at
    degree 15 has strictly less of it (the Python model of the scheme: 169 against 63 at m = 64, 95 against 0 at 4096)"""
    logQ, nl, count, g = 256, 4, 2, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    n = S.total
    sk1, pk0, pk1 = device_keys(ctx, logQ, 0xAC71 + m)
    ksk = s2_matrix(ctx, logQ, sk1, 0xAC71 + m)
    rng = np.random.default_rng(m)
    vals = rng.integers(0, p, size=(count, n))
    vals[0, :3] = [0, 1, p - 1]
    ctb = 2 * n * nl * 8
    x = ctx.alloc(count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 31, 0, vals, x, nl, only_usable=False)
    print(f"m = {m}, p = {p}, logQ = {logQ}: fresh budget", I(S.noise_budget(sk1, logQ, x, nl, count)))
    for d in degrees:
        coef = [int(c) for c in rng.integers(1, p, size=d + 1)]
        want = [[f_of(coef, v, p) for v in row] for row in vals]
        out = ctx.alloc(count * ctb)
        S.poly_eval(ksk, coef, logQ, x, nl, count, out)
        got = S.decrypt_batch(sk1, logQ, out, nl, count, only_usable=False)
        budget = I(S.noise_budget(sk1, logQ, out, nl, count))
        plan = F.poly_eval_plan(d)
        print(f"  degree {d}: B = {plan['B']}, {plan['nks']} key switches, depth {plan['depth']}: budget {budget}")
        for i in range(count):
            assert I(got[i]) == want[i], (d, i)
        assert min(budget) > 0
        hy = horner(ctx, ksk, logQ, p, nl, coef, x, count)
        hgot = S.decrypt_batch(sk1, logQ, hy, nl, count, only_usable=False)
        hbudget = I(S.noise_budget(sk1, logQ, hy, nl, count))
        print(f"  degree {d}: Horner, {d - 1} key switches, depth {d - 1}: budget {hbudget}")
        for i in range(count):
            if hbudget[i] > 0:
                assert I(hgot[i]) == want[i], (d, i, "Horner")
        if d == 15:
            assert max(hbudget) < min(budget)


def test_three_layer_network():
    """(4096, 65537, logQ 256): a 16 x 64 layer, the activation x^3 + 3 x + 5, a 4 x 16 layer -- the first layer's output is the second's replicated
    input as it is; every slot decrypts to the numpy model, with a positive budget"""
    m, p, g, logQ, nl, count = 4096, 65537, 3, 256, 4, 2
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    n = S.total
    rng = np.random.default_rng(5)
    M1, b1 = rng.integers(0, p, size=(16, 64)), rng.integers(0, p, size=16)
    M2, b2 = rng.integers(0, p, size=(4, 16)), rng.integers(0, p, size=4)
    l1, l2 = S.linear(M1, b1), S.linear(M2, b2)
    amounts = sorted(set(l1.amounts) | set(l2.amounts))
    (sk1, pk0, pk1), _, hoisted = rotation_keys(ctx, logQ, [S.rotation_k(a) for a in amounts])
    mats = dict(zip(amounts, hoisted))
    ksk = s2_matrix(ctx, logQ, sk1, 99)
    coef = [5, 3, 0, 1]
    xin = rng.integers(0, p, size=(count, S.rows, 64))
    ctb = 2 * n * nl * 8
    c0, c1, c2, c3 = (ctx.alloc(count * ctb) for _ in range(4))
    S.encrypt_batch_seeded(pk0, pk1, logQ, 12, 0, S.replicate(xin, 64), c0, nl, only_usable=False)
    l1.apply(mats, logQ, c0, nl, count, c1)
    S.poly_eval(ksk, coef, logQ, c1, nl, count, c2)
    l2.apply(mats, logQ, c2, nl, count, c3)
    got = S.decrypt_batch(sk1, logQ, c3, nl, count, only_usable=False)
    for i in range(count):
        h = [[f_of(coef, int(v), p) for v in (M1.astype(object) @ xin[i, r].astype(object) + b1) % p] for r in range(S.rows)]
        assert I(got[i]) == LM.expected_slots(M2, b2, np.array(h), p, S.rows, S.cols), i
    budget = I(S.noise_budget(sk1, logQ, c3, nl, count))
    print("noise budget after layer, activation, layer:", budget, "after the activation:", I(S.noise_budget(sk1, logQ, c2, nl, count)))
    assert min(budget) > 0
    l1.close()
    l2.close()


def test_poly_eval_over_a_slot_basis():
    """two primes below 2^20 on m = 4096: f(x) = x^3 - 4096 x^2 + 5 x - 7 on 12-bit data leaves either prime behind and stays inside (-P/2, P/2)"""
    m, g, logQ, nl, count = 4096, 3, 192, 3, 2
    primes = F.slots_basis_plan(m, 30, 20, g)["primes"]
    assert len(primes) == 2
    chain, roots = P.chain_for(m, logQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k = B.total, B.k
    sk1, pk0, pk1 = device_keys(ctx, logQ, 41)
    ksk = s2_matrix(ctx, logQ, sk1, 41)
    rng = np.random.default_rng(13)
    x = rng.integers(0, 1 << 12, size=(count, n))
    x[0, :2] = [0, 4095]
    coef = [-7, 5, -4096, 1]
    exact = [[sum(c * int(v) ** e for e, c in enumerate(coef)) for v in row] for row in x]
    big = max(abs(v) for row in exact for v in row)
    assert big > max(primes) and big < B.modulus // 2 and min(v for row in exact for v in row) < 0
    ctb = 2 * n * nl * 8
    cx, out = ctx.alloc(k * count * ctb), ctx.alloc(k * count * ctb)
    B.encrypt_batch_seeded(pk0, pk1, logQ, 78, 0, x, cx, nl)
    B.poly_eval(ksk, coef, logQ, cx, nl, count, out)
    got = B.decrypt_batch(sk1, logQ, out, nl, count)
    for i in range(count):
        assert I(got[i]) == exact[i], i
    budget = B.noise_budget(sk1, logQ, out, nl, count)[1]
    print("noise budget over the basis:", I(budget))
    assert min(I(budget)) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_condition_and_leave_the_context_working():
    ctx, ksk, a = ring(4096)
    n, count, npool = ctx.phim, 3, 3
    ctb = 2 * n * NL * 8
    pool, out = ctx.upload(a), ctx.alloc(count * ctb)
    coef = [3, -1, 0, 2, 7]
    lib = F.Backend.lib()

    def good():
        ctx.ct_poly_eval_dev(ksk, LOGQ, P0, coef, pool, NL, count, out)
        y = out.download((count, 2, n, NL))
        ctx.ct_lin_comb_dev(LOGQ, P0, pool, npool, NL, [0, 1], [2, -3], [0, 2], [1], out)
        return y, out.download((1, 2, n, NL))

    first = good()

    def refused(word, call):
        with pytest.raises(F.FhesiError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        again = good()
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), word

    def raw(fn, *args):
        if fn(*args) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())

    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    lc = lambda logQ=LOGQ, p=P0, pl=pool, npl=npool, nl=NL, ia=(0, 1), cf=(2, -3), sg=(0, 2), kn=(1,), o=out: \
        ctx.ct_lin_comb_dev(logQ, p, pl, npl, nl, list(ia), list(cf), list(sg), None if kn is None else list(kn), o)
    # ---- fhesi_ct_lin_comb_dev
    refused("overlaps pool", lambda: lc(o=View(pool, ctb)))
    refused("out of range", lambda: lc(ia=(0, 3)))
    refused("out of range", lambda: lc(ia=(-1, 1)))
    refused("must start at 0", lambda: lc(sg=(1, 2)))
    refused("not non-decreasing", lambda: lc(ia=(0, 1, 2), cf=(1, 1, 1), sg=(0, 2, 1, 3), kn=(0, 0, 0)))
    refused("outside the supported 1..32", lambda: lc(nl=0))
    refused("outside the supported 1..32", lambda: lc(nl=33, logQ=2100))
    refused("cannot hold logQ", lambda: lc(logQ=129))
    refused("cannot hold logQ", lambda: lc(logQ=0))
    refused("plaintext modulus", lambda: lc(p=1))
    refused("null argument", lambda: raw(lib.fhesi_ct_lin_comb_dev, ctx.h, LOGQ, P0, None, npool, NL, i32([0]), i64([1]), i32([0, 1]), None, 1, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_lin_comb_dev, ctx.h, LOGQ, P0, pool.ptr, npool, NL, None, i64([1]), i32([0, 1]), None, 1, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_lin_comb_dev, ctx.h, LOGQ, P0, pool.ptr, npool, NL, i32([0]), None, i32([0, 1]), None, 1, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_lin_comb_dev, ctx.h, LOGQ, P0, pool.ptr, npool, NL, i32([0]), i64([1]), None, None, 1, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_lin_comb_dev, ctx.h, LOGQ, P0, pool.ptr, npool, NL, i32([0]), i64([1]), i32([0, 1]), None, 1, None))
    # ---- fhesi_ct_poly_eval_dev
    pe = lambda k=ksk, logQ=LOGQ, p=P0, cf=coef, s=pool, nl=NL, o=out, baby=0, db=3: ctx.ct_poly_eval_dev(k, logQ, p, cf, s, nl, count, o, baby, db)
    primes, roots = P.chain_for(4096, LOGQ, P0)
    other = F.Context(4096, primes, roots)
    osk, _, _ = device_keys(other, LOGQ, 5)
    refused("context mismatch", lambda: pe(k=s2_matrix(other, LOGQ, osk, 5)))
    refused("digits", lambda: pe(db=2))
    refused("decompSize", lambda: pe(db=8))
    refused("cannot hold logQ", lambda: pe(nl=1))
    two = F.KeySwitchMatrix(ctx, 2, R.ndigits(LOGQ))
    refused("3 source components", lambda: pe(k=two))
    refused("degree", lambda: pe(cf=[1] * 4098))
    refused("degree", lambda: raw(lib.fhesi_ct_poly_eval_dev, ctx.h, ksk.h, LOGQ, P0, 3, i64([1]), 0, 0, pool.ptr, NL, count, out.ptr))
    refused("baby", lambda: pe(baby=5))
    refused("baby", lambda: pe(baby=-1))
    refused("plaintext modulus", lambda: pe(p=1))
    refused("out overlaps in", lambda: pe(o=View(pool, 64)))
    refused("out overlaps in", lambda: pe(o=pool))
    refused("null coefficients", lambda: raw(lib.fhesi_ct_poly_eval_dev, ctx.h, ksk.h, LOGQ, P0, 3, None, 4, 0, pool.ptr, NL, count, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_poly_eval_dev, ctx.h, ksk.h, LOGQ, P0, 3, i64(coef), 4, 0, None, NL, count, out.ptr))
    refused("null argument", lambda: raw(lib.fhesi_ct_poly_eval_dev, ctx.h, ksk.h, LOGQ, P0, 3, i64(coef), 4, 0, pool.ptr, NL, count, None))
    refused("context mismatch", lambda: raw(lib.fhesi_ct_poly_eval_dev, ctx.h, None, LOGQ, P0, 3, i64(coef), 4, 0, pool.ptr, NL, count, out.ptr))
