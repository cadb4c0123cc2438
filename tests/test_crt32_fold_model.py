"""CPU: an integer model of the tensor half's CRT on rows of 2^14 (fhe-si_amd/csrc/kernels_tensor32.hip) since the CRT constant travels with the
inverse transform's closing multiplication and the fast pass forms its words from bit logQ - 64 upwards.

  * closing stage (ntt32_inv_kernel3, last stage): (X + Y) c and (X - Y + 2p)(w c) with c = (M / p_i)^-1 / n through mulc (any 32-bit value -> [0, 2p))
    and one min(v, v - p): the row value is y_i = x (M / p_i)^-1 mod p_i, below p.  The ranges are those of the 1/n pair (test_arith32_models.py): only
    the constant differs.
  * the fold loader of crt32_scale_generic_kernel: three values below p added with their signs, at most 3p, made canonical by two range steps.
  * window (t32_j0): the first word J0 is the largest for which everything below it is provably less than 2^(logQ - 28); the fast pass is undecided
    when bits logQ-28 .. logQ-1 of its rounding limb read 0111...1.  Whenever it is NOT undecided its limbs equal the exact rounding, the exact pass
    (every word) always does, and no 64-bit accumulator overflows.

crafted() are the inputs tests/test_gpu_crt_fold.py puts on the device: what the model says about them is asserted here, without a GPU."""
import random

import pytest

import test_arith32_models as A

M32, M64 = A.M32, A.M64
WIN = 28
SHAPES = {512: (28, 38, 62), 1024: (26, 82, 76)}      # logQ: word bits R, table words WT, the most primes the table is built for


def t32_j0(LQ, R, np_max):
    tb = 0
    while (1 << tb) < np_max + 1:
        tb += 1
    return 0 if LQ < WIN + 30 + tb else (LQ - WIN - 30 - tb) // R


def test_window_start_is_the_largest_provable_one():
    for LQ, (R, WT, np_max) in SHAPES.items():
        J0 = t32_j0(LQ, R, np_max)
        assert J0 == {512: 16, 1024: 36}[LQ]
        # every dropped word position holds np_max + 1 terms (value below 2^30) x (table word below 2^R)
        dropped = (np_max + 1) * ((1 << 30) - 1) * ((1 << (R * J0)) - 1)
        assert dropped < 1 << (LQ - WIN)
        assert (np_max + 1) * ((1 << 30) - 1) * ((1 << (R * (J0 + 1))) - 1) >= 1 << (LQ - WIN), "one word later the bound no longer holds"
        assert R * J0 <= LQ - 64, "the rounding limb (bits logQ-64 .. logQ-1) is formed"
    for LQ in range(64, 513):                        # the generic kernel's run-time window
        J0 = t32_j0(LQ, 28, 62)
        assert J0 >= 0 and 28 * J0 <= LQ - 64 and (J0 == 0 or 63 * (1 << 30) * (1 << (28 * J0)) <= 1 << (LQ - WIN))


def tables(primes, R, WT):
    M = 1
    for p in primes:
        M *= p
    Mi = [M // p for p in primes]
    cinv = [pow(mi % p, -1, p) for mi, p in zip(Mi, primes)]
    inv57 = [(1 << 57) // p for p in primes]
    word = lambda v, l: (v >> (R * l)) & ((1 << R) - 1)
    Mw = [[word(mi, l) for l in range(WT)] for mi in Mi]
    N = ((1 << (R * WT)) - M) & ((1 << (R * WT)) - 1)
    return M, cinv, inv57, Mw, [word(N, l) for l in range(WT)]


def crt32_scale(y, primes, tb, LQ, R, exact, np_max):
    """crt32_scale_kernel<LQ, exact, R, WT, 0> on row values y_i = x (M / p_i)^-1 mod p_i -> (round(x / 2^LQ) mod 2^LQ, undecided, kappa)"""
    M, _, inv57, Mw, Nw = tb
    WU = (2 * LQ + R - 1) // R
    J0 = 0 if exact else t32_j0(LQ, R, np_max)
    NW = WU - J0
    acc, fsum = [0] * NW, 0
    for i, p in enumerate(primes):
        assert y[i] < p
        fsum = (fsum + ((y[i] * inv57[i]) >> 32)) & M32
        for l in range(NW):
            acc[l] += y[i] * Mw[i][J0 + l]
            assert acc[l] <= M64
    kappa = ((fsum + (1 << 24)) & M32) >> 25
    carry = 0
    for l in range(NW):
        v = acc[l] + kappa * Nw[J0 + l]
        assert v <= M64
        v += carry
        assert v <= M64
        acc[l], carry = v & ((1 << R) - 1), v >> R

    def limb(B):
        l0, o = B // R - J0, B % R
        assert l0 >= 0
        v = 0
        for k in range(4):
            if l0 + k < NW and k * R - o < 64:
                v |= (acc[l0 + k] << (k * R)) >> o
        return v & M64
    G = limb(LQ - 64)
    undecided = (not exact) and (G >> (64 - WIN)) == (1 << (WIN - 1)) - 1
    c, out = G >> 63, 0
    for i in range(LQ // 64):
        v = (limb(LQ + 64 * i) + c) & M64
        c = 1 if (c and v == 0) else 0
        out |= v << (64 * i)
    return out, undecided, kappa


def expected(x, LQ):
    return ((x + (1 << (LQ - 1))) >> LQ) & ((1 << LQ) - 1)


def mulc(y, w, p):
    """the closing multiplication of ntt32_inv_kernel3: quotient estimate, y w - Q p in 32 bits -> [0, 2p), then min(v, v - p)"""
    v = A.mul_lazy32(y, w, (w << 32) // p, p)
    assert v < 2 * p
    return v - p if v >= p else v


@pytest.mark.parametrize("primes", [A.primes_below_2_30(35, 1 << 15), A.primes_below_2_29(36, 1 << 15)], ids=["30-bit", "29-bit"])
def test_closing_stage_leaves_the_crt_residue(primes):
    """the last inverse stage with c = (M / p_i)^-1 / n: any sum below 4p (8p: primes below 2^29) comes out as its canonical product"""
    rng = random.Random(14)
    _, cinv, _, _, _ = tables(primes, 28, 38)
    for p, ci in zip(primes, cinv):
        c = ci * pow(1 << 14, -1, p) % p
        w = rng.randrange(1, p)
        lim = 4 * p if p >> 29 else 8 * p
        for v in [0, 1, p - 1, p, 2 * p, lim - 1] + [rng.randrange(lim) for _ in range(40)]:
            assert v <= M32
            assert mulc(v, c, p) == v * c % p and mulc(v, c * w % p, p) == v * c * w % p


@pytest.mark.parametrize("p", A.primes_below_2_30(35, 1 << 15)[-2:] + A.primes_below_2_29(36, 1 << 15)[:1] + A.GENERIC_PRIMES[:1])
def test_fold_loader_keeps_the_value_canonical(p):
    """crt32_scale_generic_kernel, S = 0 with a fold, on rows already multiplied by the CRT constant: r + (p - b) + (c | p - c) (m = 2Q) and
    r + b + (p - c) (m odd), b = 0 when its position lies beyond the row; two range steps"""
    rng = random.Random(p)
    twop = 2 * p
    ext = [0, 1, p - 1, p // 2]
    for r in ext + [rng.randrange(p) for _ in range(6)]:
        for b in ext + [rng.randrange(p)]:
            for c in ext + [rng.randrange(p)]:
                for s, want in ((r + (p - b) + c, r - b + c), (r + (p - b) + (p - c), r - b - c), (r + b + (p - c), r + b - c)):
                    assert s <= 3 * p and s <= M32
                    s = min(s, (s - twop) & M32)
                    s = min(s, (s - p) & M32)
                    assert s < p and s == want % p


def boundary_values(rng, LQ, bound):
    """x ON the rounding boundary: x + 2^(LQ-1) = t 2^LQ + delta with delta from a few units to beyond the dropped part, both signs"""
    xs = []
    for _ in range(25):
        t = rng.randrange(-(bound >> (LQ + 1)), bound >> (LQ + 1))
        for delta in (0, 1, rng.randrange(1 << 60), rng.randrange(1 << (LQ - 120)), rng.randrange(1 << (LQ - 82)), rng.randrange(1 << (LQ - 64)),
                      rng.randrange(1 << (LQ - 40)), rng.randrange(1 << (LQ - 30)), (1 << (LQ - 28)) - 1, 1 << (LQ - 28), rng.randrange(1 << (LQ - 20))):
            xs += [t * (1 << LQ) - (1 << (LQ - 1)) - 1 - delta, t * (1 << LQ) - (1 << (LQ - 1)) + delta]
    return xs


@pytest.mark.parametrize("LQ,primes", [(512, A.primes_below_2_30(35, 1 << 15)), (512, A.primes_below_2_29(36, 1 << 15)), (1024, A.primes_below_2_30(70, 1 << 16))],
                         ids=["512-30bit", "512-29bit", "1024-30bit"])
def test_crt32_scale_window_and_flag(LQ, primes):
    R, WT, np_max = SHAPES[LQ]
    tb = tables(primes, R, WT)
    M = tb[0]
    rng = random.Random(LQ)
    bound = M // 8 if primes[0] >> 29 else M * 9 // 25          # what t32_plan leaves: |x / M| < 1/8 (0.36: primes below 2^29)
    h = 1 << (LQ - 1)
    xs = [0, 1, -1, bound - 1, -(bound - 1), h, h - 1, -h, -h - 1] + boundary_values(rng, LQ, bound) + [rng.randrange(-bound + 1, bound) for _ in range(60)]
    nflag = wrong_without_cleanup = 0
    for x in xs:
        assert abs(x) < bound
        y = [x * c % p for c, p in zip(tb[1], primes)]
        o_fast, und, kappa = crt32_scale(y, primes, tb, LQ, R, False, np_max)
        o_exact, _, kappa_e = crt32_scale(y, primes, tb, LQ, R, True, np_max)
        assert kappa == kappa_e and sum(yi * (M // p) for yi, p in zip(y, primes)) - kappa * M == x
        assert o_exact == expected(x, LQ)
        if und:
            nflag += 1
            wrong_without_cleanup += o_fast != expected(x, LQ)
        else:
            assert o_fast == expected(x, LQ), hex(x)
    assert nflag > 0 and wrong_without_cleanup > 0, "the boundary cases must exercise the flag, and the exact pass must matter"


# ---------------------------------------------------------------------------------------------- the device test's crafted coefficients
METRIC_PRIMES = A.primes_below_2_30(35, 1 << 15)        # logQ = 512 on m = 2^15
# delta = (x + 2^511) mod 2^512, centred.  OLD: within the reach of the former window too (words from bit 392: dropped part below 2^429).
OLD_DELTAS = [0, 1, -1, 2, -3, 100, -100, 1 << 40, -(1 << 40), (1 << 390) + 12345, -(1 << 391)]
# NEW_ONES: the rounding limb (bits 448..511 of x + 2^511) has bits 484..511 all ones and a zero somewhere in bits 448..483 -- undecided under the
# window from bit 448 only.  NEW_CROSS: just ABOVE the boundary by more than the former window dropped and less than this one does, so the formed
# value falls below the boundary: without the exact pass these round wrong.
NEW_ONES = [-(1 << 448) - 1, -(1 << 460) - 12345, -(1 << 483) - (1 << 470), -(1 << 484) + 1, -(1 << 449)]
NEW_CROSS = [1 << 430, (1 << 450) + 77, 1 << 470, (1 << 478) + (1 << 300)]


def crafted(deltas, p, LQ=512):
    """coefficients A with (p A + 2^(LQ-1)) mod 2^LQ = delta (A centred modulo 2^LQ): coefficient j of (p a0) . 1 is x = p A_j"""
    mod = 1 << LQ
    inv_p = pow(p, -1, mod)
    out = []
    for d in deltas:
        v = (d - (mod >> 1)) * inv_p % mod
        out.append(v - mod if v >= mod // 2 else v)
    return out


def rounding_limb(x, LQ=512):
    return ((x + (1 << (LQ - 1))) >> (LQ - 64)) & M64


def test_crafted_coefficients_sit_where_they_should():
    p, LQ = 23, 512
    tb = tables(METRIC_PRIMES, 28, 38)

    def run(x):
        y = [x * c % q for c, q in zip(tb[1], METRIC_PRIMES)]
        return crt32_scale(y, METRIC_PRIMES, tb, LQ, 28, False, 62)
    for Aj in crafted(NEW_ONES, p):
        G = rounding_limb(p * Aj)
        assert G >> 36 == (1 << 28) - 1 and G & ((1 << 36) - 1) != (1 << 36) - 1
        assert run(p * Aj)[0] == expected(p * Aj, LQ) or run(p * Aj)[1]
    for Aj, d in zip(crafted(NEW_CROSS, p), NEW_CROSS):
        x = p * Aj
        assert (x + (1 << 511)) % (1 << 512) == d and (1 << 429) < d < (1 << 484)
        o, und, _ = run(x)
        assert und and o != expected(x, LQ), "formed from bit 448, the value lies below the boundary: flagged, and wrong without the exact pass"
    for Aj, d in zip(crafted(OLD_DELTAS, p), OLD_DELTAS):
        x = p * Aj
        G = rounding_limb(x)
        assert G == (M64 if d < 0 else 0)
        o, und, _ = run(x)
        assert und and (o != expected(x, LQ)) == (d >= 0), d      # (d = 0 is the half that rounds up: the formed value lies below it)
