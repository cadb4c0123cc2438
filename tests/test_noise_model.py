"""CPU: the noise budget's definitions (include/fhesi_hip.h) on Python integers, and the replay of the kernel's word arithmetic
(tests/noise_model.py after fhe-si_amd/csrc/kernels_ct.hip) against them."""
import json
import os
import random
import re

import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import noise_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = [23, 257, 65537, (1 << 31) - 1]
# nw = 1 | full top word | one top bit in a second word | ... : every MAXNL instantiation (2 / 9 / 17 / 32) and both sides of each dispatch boundary
LOGQS = [20, 63, 64, 127, 128, 511, 512, 575, 576, 1024, 1100]


@pytest.mark.parametrize("logQ", [20, 63, 64, 65, 127, 128, 512])
@pytest.mark.parametrize("p", PS)
def test_identities(logQ, p):
    q = 1 << logQ
    rng = random.Random(logQ * 131 + p)
    zs = [rng.randrange(-(q << 70), q << 70) for _ in range(200)] + [0, 1, -1, q, -q, q - 1]
    for z in zs:
        r = N.residual(z, logQ, p)
        assert -q <= r < q
        assert 2 * p * z + q == 2 * q * ((2 * p * z + q) // (2 * q)) + (r + q)
        assert N.message(z, logQ, p) == ((2 * p * z + q) // (2 * q)) % p
        assert N.residual(z % (2 * q), logQ, p) == r and N.message(z % (2 * q), logQ, p) == N.message(z, logQ, p)      # only z mod 2q matters
        P = r + q
        assert abs(r) == (P - q if P >> logQ & 1 else q - P) and abs(r).bit_length() <= logQ + 1
    for mx in [0, 1, 2, 3, q - 1, q, q >> 1, (q >> 1) - 1] + [rng.randrange(q) for _ in range(50)]:
        b = N.budget_of(mx, logQ)
        assert 0 <= b <= logQ and (b == 0 or mx << b < q) and (mx << (b + 1) >= q or mx == 0)
    assert N.budget_of(0, logQ) == logQ and N.budget_of(q, logQ) == 0


@pytest.mark.parametrize("logQ", [20, 63, 64, 65, 127, 128, 512])
@pytest.mark.parametrize("p", PS)
def test_every_even_boundary_residual_is_reached_by_c0_alone(logQ, p):
    q = 1 << logQ
    rng = random.Random(logQ + p)
    for r in N.boundary_residuals(logQ) + [2 * rng.randrange(-(q >> 1), q >> 1) for _ in range(50)]:
        c0 = N.crafted_c0(r, logQ, p)
        assert -(q >> 1) <= c0 < (q >> 1)
        assert N.residual(c0, logQ, p) == r


@pytest.mark.parametrize("logQ", LOGQS)
def test_kernel_words_equal_the_big_integer_model(logQ):
    q, nw = 1 << logQ, (logQ + 1 + 63) // 64
    rng = random.Random(logQ)
    for p in PS + [2, (1 << 62) - 57]:
        zs = [rng.randrange(-(1 << (64 * nw - 1)), 1 << (64 * nw - 1)) for _ in range(40)] + [0, -1, 1, q - 1, q, -q, 2 * q - 1, q >> 1, -(q >> 1)]
        if p % 2:
            zs += [N.crafted_c0(r, logQ, p) for r in N.boundary_residuals(logQ)]
        for z in zs:
            msg, a = N.kernel_coefficient(N.words_of(z, nw), logQ, p)
            assert msg == N.message(z, logQ, p), (p, z)
            assert N.int_of(a) == abs(N.residual(z, logQ, p)), (p, z)
    p = 65537
    zs = [rng.randrange(-q, q) for _ in range(300)]                        # two blocks, the second partly filled
    msgs, mx, budget = N.kernel_noise(zs, logQ, p)
    assert msgs == [N.message(z, logQ, p) for z in zs]
    assert (N.int_of(mx), budget) == N.noise_of_z(zs, logQ, p)
    for r in (0, 2, q - 2, -q):                                             # all coefficients equal: budget logQ ... 0
        zs = [N.crafted_c0(r, logQ, p)] * 70
        assert N.kernel_noise(zs, logQ, p)[1:] == (N.words_of(abs(r), nw), N.budget_of(abs(r), logQ))


def test_limb_elimination_maximum():
    rng = random.Random(5)
    for nw in (1, 2, 3, 9):
        W = lambda v: N.words_of(v, nw)
        top = rng.randrange(1 << 63) << (64 * (nw - 1))
        lists = [
            [top + rng.randrange(1 << 40) for _ in range(256)],                                  # equal top words
            [rng.randrange(1 << (64 * nw)) for _ in range(256)],
            [(1 << (64 * nw)) - 1] + [rng.randrange(1 << (64 * nw - 1)) for _ in range(255)],    # the maximum first
            [rng.randrange(1 << (64 * nw - 1)) for _ in range(255)] + [(1 << (64 * nw)) - 1],    # ... and last
            [12345 << (64 * (nw - 1))] * 256,                                                    # all equal
            [0] * 256,
            [5, 4, 5, 3],                                                                        # a tie
        ]
        for vals in lists:
            assert N.int_of(N.limb_max([W(v) for v in vals], nw)) == max(vals)


def test_golden_fixture():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "noise.json")))
    ctx = R.Ctx(d["m"], d["logQ"], d["p"], [int(x) for x in d["primes"]], [int(x) for x in d["roots"]])
    t = R.dcrt_from_poly(ctx, d["t"])
    assert len(d["cases"]) == 3
    for case in d["cases"]:
        parts = [[int(c) for c in part] for part in case["parts"]]
        msg, mx, budget = N.noise(ctx, t, parts)
        assert (msg, mx, budget) == (case["message"], int(case["maxres"]), case["budget"])
        assert msg == R.decrypt(ctx, d["t"], parts)
        zs = N.z_of(ctx, t, parts)
        kmsg, kmx, kbudget = N.kernel_noise(zs, ctx.logQ, ctx.p)
        assert (kmsg, N.int_of(kmx), kbudget) == (msg, mx, budget)


def test_entry_points_declared():
    src = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("fhesi_ct_noise_batch", "fhesi_decrypt_noise_batch", "fhesi_ct_noise_int_batch"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in F.binding.ABI_SYMBOLS, name
    assert F.binding.ABI_VERSION == 9 and re.search(r"#define\s+FHESI_ABI_VERSION\s+9\b", src)
