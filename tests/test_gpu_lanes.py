"""GPU: option lanes = 2 of fhesi_ct_mul_relin_batch_dev (capi_pipeline.hip) -- the second half of a batch on a second stream with a second
workspace set between fork and join events -- gives the bits of one lane and of the oracle: on the first call of a cold context (every derived
table the halves share is built inside that call), on the warm context, staggered, chunked inside a lane, at an even count, below the
threshold, with a generated matrix, through the host-buffer entry, and on a ring where the option is ignored.  Work enqueued after the call is
ordered after both halves.  Also here: fhesi_ksk_upload_dev invalidates the tables derived from the matrix it replaces.
Every comparison is bit-exact, every context is made inside its test."""
import functools

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu
# the per-prime form of the key switch; n = 2^11: limbs over the two largest chain primes; n = 2^14: the 30-bit tensor half and limbs over the
# four 30-bit auxiliary primes (KeySwitchMatrix.FORMS)
SMALL, MID, BIG = (256, 128, 23), (4096, 128, 23), (32768, 128, 23)
RINGS = [SMALL, MID, BIG]
FORM = {SMALL: (0,), MID: (2, 3), BIG: (1,)}
COUNT = 9                                          # split 5 + 4


def operands(ring, count=COUNT, seed=0):
    """the two extremes of the centred range in ciphertext 0 and in the last one: one in each half"""
    m, logQ, p = ring
    n, nl = m // 2, (logQ + 63) // 64
    rng = np.random.default_rng(m + seed)
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    lo, hi = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0], O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    for c in (0, count - 1):
        a[c, 0, 0], a[c, 1, 1], b[c, 0, 0], b[c, 1, 1] = lo, hi, hi, lo
    return a, b


def context(ring, **options):
    m, logQ, p = ring
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    for name, v in options.items():                # before anything else has run on the context
        ctx.set_option(name, v)
    return ctx


def mul_dev(ctx, ksk, ring, a, b, sync=True):
    m, logQ, p = ring
    da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc(a.nbytes)
    ctx.ct_mul_relin_dev(ksk, logQ, p, da, db, out, a.shape[-1], a.shape[0])
    return out.download(a.shape) if sync else (out, da, db)


@functools.lru_cache(maxsize=None)
def reference(ring):
    """(ksm, a, b, one-lane result) on a context of its own -- computed once per ring, never written to"""
    m, logQ, p = ring
    ctx = context(ring, lanes=1)
    nd = R.ndigits(logQ)
    ksm = np.stack([P.rand_rows(np.random.default_rng(3 + m), ctx.primes, ctx.phim, 3 * nd) for _ in range(2)])
    a, b = operands(ring)
    ref = mul_dev(ctx, F.KeySwitchMatrix(ctx, 3, nd).upload(ksm), ring, a, b)
    for x in (ksm, a, b, ref):
        x.setflags(write=False)
    return ksm, a, b, ref


@functools.lru_cache(maxsize=None)
def oracle(ring):
    """one per ring (host only)"""
    m, logQ, p = ring
    return O.Oracle(m, *P.chain_for(m, logQ, p))


def oracle_mul(ring, ksm, a, b):
    m, logQ, p = ring
    return oracle(ring).ct_mul_relin(ksm, a, b, logQ, p)


@pytest.mark.parametrize("ring", RINGS)
def test_cold_two_lane_call_then_warm_then_ordered(ring):
    m, logQ, p = ring
    ksm, a, b, ref = reference(ring)
    ctx = context(ring, lanes=2)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    cold = mul_dev(ctx, ksk, ring, a, b)           # the key's derived tables, the CRT tables and the tensor half's prime tables are built in here
    assert ctx.get_option("lanes") == 2
    assert ksk.form()[0] in FORM[ring], ksk.form()
    for c in range(COUNT):
        assert np.array_equal(cold[c], ref[c]), ("cold", c)
    warm = mul_dev(ctx, ksk, ring, a, b)
    for c in range(COUNT):
        assert np.array_equal(warm[c], ref[c]), ("warm", c)
    for c in ((0, COUNT - 1) if ring == BIG else range(COUNT)):      # (n = 2^14: the one-lane reference stands in for ciphertexts 1 .. 7)
        assert np.array_equal(ref[c], oracle_mul(ring, ksm, a[c], b[c])), ("oracle", c)
    # stream semantics: work enqueued right after the call, without a synchronisation, is ordered after both halves
    zero = ctx.upload(np.zeros_like(a))
    out, da, db = mul_dev(ctx, ksk, ring, a, b, sync=False)
    ctx.ct_add_dev(logQ, zero, out, 2, nl, COUNT)
    added = zero.download(a.shape)
    for c in range(COUNT):
        assert np.array_equal(added[c], ref[c]), ("ordered", c)


@pytest.mark.parametrize("variant,options,count", [("stagger", {"stagger": 1}, COUNT),
                                                   ("chunk2", {"batch_chunk": 2}, COUNT),      # three and two chunks per lane, each lane reusing its workspace
                                                   ("count8", {}, 8),
                                                   ("count7", {}, 7)])                         # below the threshold: one lane
@pytest.mark.parametrize("ring", RINGS)
def test_two_lane_variants(ring, variant, options, count):
    m, logQ, p = ring
    ksm, a, b, ref = reference(ring)
    ctx = context(ring, lanes=2, **options)
    ksk = F.KeySwitchMatrix(ctx, 3, R.ndigits(logQ)).upload(ksm)
    for attempt in ("cold", "warm"):
        got = mul_dev(ctx, ksk, ring, a[:count], b[:count])      # ciphertexts are independent: the first `count` of the reference
        for c in range(count):
            assert np.array_equal(got[c], ref[c]), (variant, attempt, c)


def test_generated_matrix_built_inside_the_two_lane_call():
    """a matrix made by fhesi_keyswitch_init_batch_seeded on n = 2^14: its centred-limb tables are measured and built inside the first two-lane call"""
    ring = BIG
    m, logQ, p = ring
    _, a, b, _ = reference(ring)
    nd = R.ndigits(logQ)

    def generated(ctx):
        one = np.zeros((ctx.phim, 1), dtype=np.uint64)
        one[0, 0] = 1
        t = F.DoubleCRT(ctx).sample(0, 64, 77, 1)
        t2 = t.copy().op(t, F.OP_MUL)
        return F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([F.DoubleCRT.from_poly(ctx, one), t, t2], t, logQ, 77, 78, 100, 3)

    one_lane = context(ring, lanes=1)
    k1 = generated(one_lane)
    ref = mul_dev(one_lane, k1, ring, a, b)
    ctx = context(ring, lanes=2)
    k2 = generated(ctx)
    got = mul_dev(ctx, k2, ring, a, b)
    assert k2.form()[0] == 1 and k2.key_bits()[0], (k2.form(), k2.key_bits())
    assert k2.key_bits() == k1.key_bits()
    for c in range(COUNT):
        assert np.array_equal(got[c], ref[c]), c
    assert np.array_equal(mul_dev(ctx, k2, ring, a, b), ref)
    ksm = k1.download()
    assert np.array_equal(k2.download(), ksm)
    assert np.array_equal(ref[COUNT - 1], oracle_mul(ring, ksm, a[COUNT - 1], b[COUNT - 1]))


@pytest.mark.parametrize("ring", RINGS)
def test_host_buffer_entry_with_two_lanes(ring):
    """fhesi_ct_mul_relin_batch in stages of 8 (two lanes inside a stage) with a last stage of 1 (one lane)"""
    m, logQ, p = ring
    ksm = reference(ring)[0]
    a, b = operands(ring, 17, seed=1)
    outs = []
    for lanes in (1, 2):
        ctx = context(ring, lanes=lanes, host_chunk=8)
        ksk = F.KeySwitchMatrix(ctx, 3, R.ndigits(logQ)).upload(ksm)
        outs.append(ctx.ct_mul_relin(ksk, logQ, p, a, b))
    for c in range(17):
        assert np.array_equal(outs[1][c], outs[0][c]), c
    assert np.array_equal(outs[0][16], oracle_mul(ring, ksm, a[16], b[16]))


def test_option_is_ignored_off_the_power_of_two_rings():
    ring = (46, 128, 47)
    m, logQ, p = ring
    ctx = context(ring, lanes=2)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    rng = np.random.default_rng(46)
    ksm = np.stack([P.rand_rows(rng, ctx.primes, n, 3 * nd) for _ in range(2)])
    a = P.rand_limbs(rng, (COUNT, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (COUNT, 2, n), nl, logQ)
    got = mul_dev(ctx, F.KeySwitchMatrix(ctx, 3, nd).upload(ksm), ring, a, b)
    for c in range(COUNT):
        assert np.array_equal(got[c], oracle_mul(ring, ksm, a[c], b[c])), c


@pytest.mark.parametrize("ring", RINGS)
def test_ksk_upload_dev_replaces_the_matrix_and_its_derived_tables(ring):
    m, logQ, p = ring
    ctx = context(ring)
    n, nd = ctx.phim, R.ndigits(logQ)
    rng = np.random.default_rng(m + 5)
    A, B = (np.stack([P.rand_rows(rng, ctx.primes, n, 3 * nd) for _ in range(2)]) for _ in range(2))
    a, b = operands(ring, 2, seed=2)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(A)
    got_a = mul_dev(ctx, ksk, ring, a, b)
    assert ksk.form()[0] in FORM[ring], ksk.form()  # MID, BIG: forms with tables derived from the matrix, which upload_dev has to invalidate
    assert np.array_equal(got_a[0], oracle_mul(ring, A, a[0], b[0]))
    staged = ctx.upload(B)                         # the staging buffer of a broadcast
    ksk.upload_dev(staged.ptr.value)
    got_b = mul_dev(ctx, ksk, ring, a, b)
    assert not np.array_equal(got_b, got_a)
    for c in range(2):
        assert np.array_equal(got_b[c], oracle_mul(ring, B, a[c], b[c])), c
    assert np.array_equal(ksk.download(), B)
    fresh = F.KeySwitchMatrix(ctx, 3, nd)          # a handle filled by upload_dev alone
    fresh.upload_dev(staged.ptr.value)
    assert np.array_equal(mul_dev(ctx, fresh, ring, a, b), got_b)


@pytest.mark.parametrize("options", [{}, {"stagger": 1}], ids=["together", "staggered"])
def test_each_lane_keeps_its_own_clean_up_flags(options):
    """The chain shape of 18 primes at logQ = 512 converts through the sum-form CRT (kernels_crt.hip), whose first kernel flags the workgroups
    the exact kernel has to redo (one workgroup per polynomial on this ring).  Ciphertexts with coefficients whose rounding in ScaleDown sits
    on the edge (test_sum_form_crt_undecided_coefficients) alternate with random ones, 9 + 8: the crafted ones are the even places of the
    first half and the odd places of the second, in a part of the product that changes from one to the next -- no flag of one lane's launch
    equals the other lane's flag at the same index, so a flag written across lanes is a missed or a spurious clean-up.  A flag one lane's
    kernel set must still stand when that lane's clean-up reads it."""
    ring = (64, 512, 23)
    m, logQ, p = ring
    count = 17
    ctx = context(ring, lanes=2, **options)
    assert ctx.L == 18
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    mod = 1 << logQ
    inv_p = pow(p, -1, mod)
    deltas = [0, 1, -1, 2, -2, 3, -3, 5, -5, 7, -7, 8, -8, 100, -100]      # x = p A with (x + 2^(logQ-1)) mod 2^logQ = delta
    A = [((d - (mod >> 1)) * inv_p + (mod >> 1)) % mod - (mod >> 1) for d in deltas]
    rng = np.random.default_rng(64)
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    crafted = list(range(0, count, 2))             # 0 2 4 6 8 of the first half (places 0 .. 8), 1 3 5 7 of the second (places 9 .. 16)
    for c in crafted:
        ia, ib = [(0, 0), (0, 1), (1, 1)][(c // 2) % 3]       # the edge values in part 0, 1 or 2 of the tensor product: A times the constant 1
        a[c], b[c] = 0, 0
        a[c, ia] = O.ints_to_limbs((A[c % len(A):] + A[:c % len(A)] + [0] * n)[:n], nl)
        b[c, ib, 0, 0] = 1
    ksm = np.stack([P.rand_rows(rng, ctx.primes, n, 3 * nd) for _ in range(2)])
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    want = np.stack([oracle_mul(ring, ksm, a[c], b[c]) for c in range(count)])
    for attempt in ("cold", "warm", "again"):
        got = mul_dev(ctx, ksk, ring, a, b)
        for c in range(count):
            assert np.array_equal(got[c], want[c]), (attempt, c)
    ctx.set_option("crt_skip_cleanup", 1)          # the crafted inputs really need the clean-up, in both halves; the random ones do not
    got = mul_dev(ctx, ksk, ring, a, b)
    for c in range(count):
        assert np.array_equal(got[c], want[c]) == (c not in crafted), c
