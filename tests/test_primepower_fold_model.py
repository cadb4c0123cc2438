"""CPU: the specification of the prime-power rings m = q^k and 2 q^k (q an odd prime) on the fused 30-bit paths (no GPU).
(1) The strided fold of a linear product S (degree <= 2 phi - 2) into the ring, with s = q^(k-1), phi = (q - 1) s, Q = q^k:
        m = Q:    out_j = S_j + S_(j+m) - S_(phi + j mod s)
        m = 2Q:   out_j = S_j - S_(j+Q) - (-1)^floor(j/s) S_(phi + j mod s)
    (g32_fold, the position tables of ks_recombine_centred_kernel, crt32_scale_generic_kernel) against the schoolbook remainder modulo Phi_m.
(2) The coefficient gather of a(X^k) mod Phi_m (ct_automorph_parts_kernel): R_e = sum of +-a_j over j k = e, folded the same way.
(3) The classification (hm::prime_power_ring, fhesi_ctx_lin_class): which m take the fold, with which offset, stride and row length.
Phi_m is built as tests/test_phi_reduction_model.py builds it (binomial products and exact divisions)."""
import math
import random

import pytest

import fhe_si_amd as F
from test_phi_reduction_model import phi_and_psi


def rem_phi(f, phi):
    """schoolbook remainder of the integer polynomial f by the monic phi"""
    n = len(phi) - 1
    g = list(f)
    for k in range(len(g) - 1, n - 1, -1):
        c = g[k]
        if c:
            for j in range(n + 1):
                g[k - n + j] -= c * phi[j]
    return (g + [0] * n)[:n]


def ring(q, k, even):
    Q = q ** k
    s = Q // q
    return (2 * Q if even else Q), Q, s, Q - s


def fold(S, m, Q, s, n):
    """the three-term fold, every read unconditional with a masked value as in the kernels"""
    at = lambda e: S[e] if e < len(S) else 0
    out = []
    for j in range(n):
        top = n + j % s
        if m & 1:
            out.append(at(j) + at(j + m) - at(top))
        else:
            out.append(at(j) - at(j + Q) - (-1) ** (j // s) * at(top))
    return out


def automorph(a, kk, m, Q, s, n):
    """at most two signed source coefficients per output (modes 1 and 2 of ct_automorph_parts_kernel)"""
    mod = m if m & 1 else Q
    kinv = pow(kk, -1, mod)

    def term(e):
        j = e * kinv % mod
        if j >= n:
            return 0
        return -a[j] if (not m & 1 and j * kk % m >= Q) else a[j]
    out = []
    for i in range(n):
        t = term(n + i % s)
        out.append(term(i) - (t if m & 1 else (-1) ** (i // s) * t))
    return out


SHAPES = [(q, k) for q in (3, 5, 7, 11) for k in (1, 2, 3)] + [(3, 4)]


@pytest.mark.parametrize("even", [False, True])
@pytest.mark.parametrize("q,k", SHAPES)
def test_strided_fold_equals_the_remainder_modulo_phi_m(q, k, even):
    m, Q, s, n = ring(q, k, even)
    phi, _ = phi_and_psi(m)
    assert len(phi) - 1 == n
    rng = random.Random(m)
    for trial in range(3):
        S = [rng.randrange(-10 ** 6, 10 ** 6) for _ in range(2 * n - 1)]
        if trial == 0:
            S = [1 << 40] * len(S)                      # every term at its largest, one sign
        assert fold(S, m, Q, s, n) == rem_phi(S, phi)
    # the fourth position of the 2 x prime form, phi + j mod s + Q, lies beyond degree 2 phi - 2 on every ring of the family
    assert n + Q > 2 * n - 2
    # each output is a sum of three entries: the bound of ks_limb_plan (factor 4) and of the tensor window (+2) holds unchanged
    assert max(abs(v) for v in fold([1] * (2 * n - 1), m, Q, s, n)) <= 3


def test_stride_one_is_the_form_of_the_prime_and_two_prime_rings():
    for q in (3, 11, 23):
        for even in (False, True):
            m, Q, s, n = ring(q, 1, even)
            assert s == 1 and n == Q - 1
            S = list(range(1, 2 * n))
            at = lambda e: S[e] if e < len(S) else 0
            old = [at(j) + at(j + m) - at(m - 1) for j in range(n)] if m & 1 else [at(j) - at(j + Q) - (-1) ** j * at(Q - 1) for j in range(n)]
            assert fold(S, m, Q, s, n) == old


@pytest.mark.parametrize("even", [False, True])
@pytest.mark.parametrize("q,k", SHAPES)
def test_automorphism_gather_equals_the_remainder_of_the_substitution(q, k, even):
    m, Q, s, n = ring(q, k, even)
    phi, _ = phi_and_psi(m)
    rng = random.Random(7 * m)
    units = [e for e in range(1, m) if math.gcd(e, m) == 1]
    ks = units if m <= 54 else sorted({units[1], units[len(units) // 2], m - 1, *rng.sample(units, 4)})
    for kk in ks:
        a = [rng.randrange(-10 ** 6, 10 ** 6) for _ in range(n)]
        sub = [0] * m                                   # a(X^k) modulo X^m - 1, a multiple of Phi_m
        for j, v in enumerate(a):
            sub[j * kk % m] += v
        assert automorph(a, kk, m, Q, s, n) == rem_phi(sub, phi), kk


RECOGNISED = {9: (3, 2), 18: (3, 2), 25: (5, 2), 27: (3, 3), 49: (7, 2), 50: (5, 2), 54: (3, 3), 121: (11, 2), 1458: (3, 6), 2187: (3, 7),
              15625: (5, 6), 16807: (7, 5), 39366: (3, 9), 59049: (3, 10)}


def lin_lg(n):
    lg = 14
    while (1 << lg) < 2 * n - 1:
        lg += 1
    return lg


@pytest.mark.parametrize("m", sorted(RECOGNISED))
def test_family_is_recognised_with_its_offset_stride_and_row_length(m):
    q, k = RECOGNISED[m]
    mm, Q, s, n = ring(q, k, m % 2 == 0)
    assert mm == m
    off, st, lg = F.lin_class(m)
    assert (off, st, lg) == (m if m & 1 else Q, s, lin_lg(n))
    assert 14 <= lg <= 20


@pytest.mark.parametrize("m", [45, 36, 4, 8, 64, 1024, 1 << 15, 4 * 9, 225, 4 * 27, 2 * 45, 15, 21])
def test_other_rings_stay_on_their_paths(m):
    assert F.lin_class(m) == (0, 0, 0)


@pytest.mark.parametrize("m,want", [(22, (11, 1, 14)), (101, (101, 1, 14)), (3, (3, 1, 14)), (6, (3, 1, 14)), (8422, (4211, 1, 14)), (32602, (16301, 1, 15)),
                                    (65537, (65537, 1, 17)), (131074, (65537, 1, 17))])
def test_prime_and_two_prime_rings_keep_their_fields(m, want):
    """k = 1: the offset and row length of the parent classification (m / 2 or m prime; 2 phi(m) - 1 <= 2^lin_lg), stride 1"""
    assert F.lin_class(m) == want


def test_decrypt_predicate_holds_on_the_model_after_one_product_and_one_rotation():
    """The choice of logQ in tests/test_gpu_primepower.py (slots end to end), reproduced on the CPU model at (m, p, g, logQ) = (50, 101, 3, 200):
    decrypt(rotate(enc a * enc b)) == rotate(a o b) slot by slot -- the reference's own predicate (Test_AddMul.cpp:84-86).  The same run at
    (1458, 1459, least generator, 256) holds too; it takes a quarter of an hour of Python big integers and is not repeated here."""
    import fhesi_pyref as R
    import params as P
    import slots_model as M
    m, p, g, logQ, trot = 50, 101, 3, 200, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, primes, roots)
    rng = R.SplitMix64(7 + m)
    t, pk = R.keygen(ctx, rng)
    S = M.slot_space(m, p, g)
    n = ctx.phim
    a, b = [(3 * i + 1) % p for i in range(n)], [(5 * i + 2) % p for i in range(n)]
    ca, cb = R.encrypt(ctx, pk, M.embed_slots(S, a, False), rng), R.encrypt(ctx, pk, M.embed_slots(S, b, False), rng)
    prod = R.ct_mul_relin(ctx, R.key_switch_init_s2(ctx, t, rng), ca, cb)
    k = pow(g, trot, m)
    rot = R.apply_key_switch_parts(ctx, R.key_switch_init_automorph(ctx, t, k, rng), R.ct_automorph(ctx, prod, k))
    want = [x * y % p for x, y in zip(a, b)]
    assert M.decode_slots(S, R.decrypt(ctx, t, prod), n, False) == want
    assert M.decode_slots(S, R.decrypt(ctx, t, rot), n, False) == want[trot:] + want[:trot]
