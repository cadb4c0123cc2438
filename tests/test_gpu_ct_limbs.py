"""GPU: every limb-class instantiation of the coefficient-domain ciphertext kernels (fhe-si_amd/csrc/kernels_ct.hip) through the public entries,
bit for bit against Python integers.

The kernels are compiled per limb class: 2 / 8 / 16 / 32 limbs for +=, *= long, the rotated sum, Encrypt's message add and the key-generation
combine; 4 / 8 / 16 / 34 (the class of nl + 2) for += ZZX; 2 / 9 / 17 / 32 words of logQ + 1 bits for Decrypt's rounding and the noise kernels.
The entries take any logQ / limb count whatever the chain, so the rings are tiny: m = 32 (n = 16, less than one wave) at both ends of every
class, m = 1024 (n = 512, two workgroups) once per class; logQ at 64 nl, 64 nl - 1, 64 (nl - 1) + 1 and in between: the shift counts 0, 63 and 1
of the sign bit and of the top limb's mask.  Operands: all ones (-1), the two extremes of the centred range, 0 and random values.

Which existing test reaches which keyed (kernel, class) cell -- the classes of the decrypt kernels count words nw = floor(logQ / 64) + 1:
  decrypt_round, decrypt_noise, noise_budget   2, 9, 17, 32: test_gpu_noise.py::test_bit_exact_against_the_model at m = 64, logQ = 20 .. 127 (nw <= 2),
                                               128 .. 575 (3 .. 9), 576 and 1024 (10, 17), 1100 (18)
  add_scaled_msg     2, 8: test_gpu_encrypt.py::test_encrypt_decrypt_vs_oracle (logQ = 64 .. 128, 511);   16, 32: nothing -> test_keyed_cells here
  keygen_combine     2, 8: test_gpu_encrypt.py::test_keyswitch_init_batch_vs_oracle (logQ = 80 .. 128, 512);  16: test_gpu_configs.py (logQ = 1024, seeded,
                     n = 2^15, checked through a multiplication only);   32: nothing -> test_keyed_cells here, both against the C oracle directly"""
import functools
import math

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P

pytestmark = pytest.mark.gpu
CAP = F.binding.ROT_SUM_MAX_TERMS
ENDS = (1, 2, 3, 8, 9, 16, 17, 32)                 # both ends of the classes 2 / 8 / 16 / 32
SHAPES = [(32, nl) for nl in ENDS] + [(1024, nl) for nl in (2, 5, 12, 32)]


def logqs(nl):
    return sorted({64 * nl, 64 * nl - 1, 64 * (nl - 1) + 1, 64 * (nl - 1) + 33})


def centred(v, logQ):
    h = 1 << (logQ - 1)
    return ((v + h) % (1 << logQ)) - h


def ints_of(a):
    return F.unpack_limbs(np.ascontiguousarray(a).view(np.int64))


def limbs_of(v, nl):
    return F.pack_limbs(np.asarray(v, dtype=object), nl).view(np.uint64)


def cen(v, logQ, nl):
    """the centred residues of an object array, as limbs"""
    return limbs_of(np.vectorize(lambda x: centred(int(x), logQ), otypes=[object])(v), nl)


def operands(seed, shape, nl, logQ):
    """centred values [..][n]: -1, the two extremes, 0 and 1 at coefficients 0 .. 4 of every polynomial, random elsewhere"""
    v = ints_of(P.rand_limbs(np.random.default_rng(seed), shape, nl, logQ))
    lo = -(1 << (logQ - 1))
    for j, s in enumerate((-1, lo, -lo - 1, 0, min(1, -lo - 1))):
        v[..., j] = s
    return v


@functools.lru_cache(maxsize=None)
def context(m, nprimes=1):
    return F.Context(m, *P.first_primes(m, nprimes))


def rotate(a, k, m, phi):
    """a(X^k) mod Phi_m over the integers: the exponents modulo m, then the long division by the monic Phi_m"""
    n = len(phi) - 1
    b = [0] * m
    for j in range(n):
        b[j * k % m] += int(a[j])
    for d in range(m - 1, n - 1, -1):
        c = b[d]
        if c:
            for i in range(n + 1):
                b[d - n + i] -= c * phi[i]
    return b[:n]


def rotate_ct(ct, k, m, phi):
    """[..][n] object array -> the same shape"""
    out = np.empty(ct.shape, dtype=object)
    for idx in np.ndindex(ct.shape[:-1]):
        out[idx] = rotate(ct[idx], k, m, phi)
    return out


@pytest.mark.parametrize("m,nl", SHAPES)
def test_add_and_mul_long(m, nl):
    ctx = context(m)
    n, count = ctx.phim, 1
    for logQ in logqs(nl):
        a, b = operands(m + logQ, (count, 2, n), nl, logQ), operands(m + logQ + 7777, (count, 2, n), nl, logQ)
        b[..., 5], b[..., 6] = a[..., 1], a[..., 2]              # extreme + the same extreme, extreme + (-1)
        a[..., 5], a[..., 6], b[..., 7] = a[..., 1], a[..., 2], a[..., 1]
        a[..., 7] = -1
        da, db = ctx.upload(limbs_of(a, nl)), ctx.upload(limbs_of(b, nl))
        ctx.ct_add_dev(logQ, da, db, 2, nl, count)
        assert np.array_equal(da.download((count, 2, n, nl)), cen(a + b, logQ, nl)), (logQ, "+=")
        for l in (1, -1, 2, 3, (1 << 63) - 1, -(1 << 63), -(1 << 62) - 12345):      # magnitudes 1, 2^63 - 1 and 2^63 among them
            da = ctx.upload(limbs_of(a, nl))
            ctx.ct_mul_long_dev(logQ, da, l, 2, nl, count)
            assert np.array_equal(da.download((count, 2, n, nl)), cen(a * l, logQ, nl)), (logQ, "*=", l)


@pytest.mark.parametrize("m,nl", SHAPES + [(32, nl) for nl in (6, 7, 14, 15)])      # (the class boundaries of nl + 2 within 8 and 16)
def test_add_const(m, nl):
    ctx = context(m)
    n, count, lim = ctx.phim, 2, 1 << 63
    for logQ in logqs(nl):
        a = operands(m + logQ, (count, 2, n), nl, logQ)
        for p in (2, 23, lim - 25):
            rng = np.random.default_rng(logQ + p % 1000)
            poly = rng.integers(-lim, lim, size=(count, n), dtype=np.int64)
            poly[0, :8] = [0, 1, -1, -p if p < lim else -1, -2 * p if 2 * p <= lim else -3, lim - 1, -lim, p - 1]      # negative with and without a remainder
            poly[1, :4] = [-(p - 1), p - 1, -(p + 1) if p + 1 <= lim else -5, 7]
            for npoly in (1, count):
                da = ctx.upload(limbs_of(a, nl))
                ctx.ct_add_const_dev(logQ, p, da, 2, nl, count, poly[:npoly])
                want = a.copy()
                for c in range(count):
                    want[c, 0] = [x + ((int(v) << logQ) // p) for x, v in zip(a[c, 0], poly[c % npoly])]
                assert np.array_equal(da.download((count, 2, n, nl)), cen(want, logQ, nl)), (logQ, p, npoly)


@pytest.mark.parametrize("m", [32, 18, 27, 25, 1024])      # mode 0; 2 x 3^2 (mode 1, stride 3); 3^3 and 5^2 (mode 2, strides 9 and 5); two workgroups
def test_automorph_gather(m):
    """Ciphertext >>= k as the signed gather (the chain is long enough that the entry takes it): the integers a(X^k) mod Phi_m, sign-extended to more
    limbs and truncated to the input's"""
    ctx = context(m, 5)
    n, count, phi = ctx.phim, 2, R.cyclotomic(m)
    units = [k for k in range(1, m) if math.gcd(k, m) == 1]
    ks = units if m < 100 else [units[1], units[len(units) // 2], m - 1]
    for nl in (1, 2, 3):
        logQ = 64 * nl
        a = operands(m + nl, (count, 2, n), nl, logQ)
        a[..., n - 1] = a[..., 1]
        src = ctx.upload(limbs_of(a, nl))
        for k in ks:
            want = rotate_ct(a, k, m, phi)
            for nlo in (nl + 1, nl):
                out = ctx.alloc(count * 2 * n * nlo * 8)
                ctx.ct_automorph_dev(k, src, 2, nl, count, out, nlo)
                assert np.array_equal(out.download((count, 2, n, nlo)), cen(want, 64 * nlo, nlo)), (nl, k, nlo)


def rot_sum_case(m, nl, logQ):
    ctx = context(m)
    n, count, top, phi = ctx.phim, 1, CAP + 1, R.cyclotomic(m)
    units = [k for k in range(2, m) if math.gcd(k, m) == 1]
    ks = [units[(5 * t) % len(units)] for t in range(top)]
    a = operands(m + logQ, (top + 1, count, 2, n), nl, logQ)
    pre, base = a[:top], a[top]
    pre_dev, base_dev = ctx.upload(limbs_of(pre, nl)), ctx.upload(limbs_of(base, nl))
    run = np.zeros((count, 2, n), dtype=object)
    for t in range(top):
        run = run + rotate_ct(pre[t], ks[t], m, phi)
        nk = t + 1
        if nk not in (1, CAP, top):
            continue
        dev = pre_dev                                             # (the terms lie count = 1 ciphertexts apart: a shorter call reads a prefix)
        out = ctx.alloc(count * 2 * n * nl * 8)
        ctx.ct_rot_sum_dev(ks[:nk], logQ, None, dev, count, nl, out)
        assert np.array_equal(out.download((count, 2, n, nl)), cen(run, logQ, nl)), (logQ, nk, "no base")
        ctx.ct_rot_sum_dev(ks[:nk], logQ, base_dev, dev, count, nl, out)
        assert np.array_equal(out.download((count, 2, n, nl)), cen(run + base, logQ, nl)), (logQ, nk, "base")
        both = ctx.upload(limbs_of(base, nl))
        ctx.ct_rot_sum_dev(ks[:nk], logQ, both, dev, count, nl, both)
        assert np.array_equal(both.download((count, 2, n, nl)), cen(run + base, logQ, nl)), (logQ, nk, "out == base")


@pytest.mark.parametrize("m,nl", SHAPES + [(18, 3), (27, 3), (25, 3), (18, 9)])
def test_rot_sum(m, nl):
    """1, CAP and CAP + 1 terms (the last one chains two launches); no base, a base, out == base"""
    for logQ in (logqs(nl) if m == 32 else (64 * nl - 1, 64 * nl)):
        rot_sum_case(m, nl, logQ)


def test_automorph_refuses_more_polynomials_than_one_grid_dimension():
    ctx = context(32, 2)
    n, count = ctx.phim, 32768
    src, out = ctx.alloc(count * 2 * n * 8), ctx.alloc(count * 2 * n * 8)
    with pytest.raises(F.FhesiError, match="more than 65535"):
        ctx.ct_automorph_dev(3, src, 2, 1, count, out, 1)
    ctx.ct_automorph_dev(3, src, 2, 1, 4, out, 1)                # the context is usable afterwards


@pytest.mark.parametrize("logQ", [1024, 1100])                   # 16 and 18 limbs: the classes 16 and 32
def test_keyed_cells(logQ):
    """Encrypt's message add and the key-generation combine at the limb classes no other test reaches, m = 32 with the shortest chain that holds logQ,
    against the C oracle with the same explicit randomness"""
    m, p = 32, 23
    primes, roots = P.chain_for(m, logQ, p)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    n, L, nd, nl = ctx.phim, len(primes), R.ndigits(logQ), (logQ + 63) // 64
    rng = np.random.default_rng(logQ)

    def dcrt(rows):
        d = F.DoubleCRT(ctx)
        for i in range(L):
            d.set_row(i, np.ascontiguousarray(rows[i]))
        return d

    count = 2
    pk_rows = P.rand_rows(rng, primes, n, 2)
    rand = np.zeros((count, 3, n), dtype=np.int64)
    rand[:, 0] = rng.integers(0, 2, size=(count, n))
    rand[:, 1:] = np.rint(rng.normal(0, 3.2, size=(count, 2, n))).astype(np.int64)
    msg = rng.integers(0, p, size=(count, n)).astype(np.int64)
    msg[0, :2] = [0, p - 1]
    out = ctx.alloc(count * 2 * n * nl * 8)
    ctx.encrypt_batch(dcrt(pk_rows[0]), dcrt(pk_rows[1]), logQ, p, rand, msg, out, nl)
    got = out.download((count, 2, n, nl))
    for c in range(count):
        assert np.array_equal(got[c], orc.encrypt(pk_rows, rand[c, 0], rand[c, 1:], msg[c], logQ, p, nl)), c

    W = L + 2
    t = rng.choice([-1, 0, 1], size=n).astype(np.int64)
    t_rows = orc.dcrt_from_poly(O.ints_to_limbs([int(x) for x in t], W))
    one_rows = orc.dcrt_from_poly(O.ints_to_limbs([1] + [0] * (n - 1), W))
    src_rows = [one_rows, t_rows]
    ncol = 2 * nd
    a = P.rand_limbs(rng, (ncol, n), nl, logQ)
    a[0, 0] = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0]
    a[0, 1] = O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    err = np.rint(rng.normal(0.0, 3.2, size=(ncol, n))).astype(np.int64)
    want = orc.keyswitch_init(np.stack(src_rows), t_rows, logQ, a, err)
    src = [dcrt(r) for r in src_rows]
    got = F.KeySwitchMatrix(ctx, 2, nd).init_batch(src, src[1], logQ, a, err).download()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
