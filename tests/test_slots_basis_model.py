"""CPU: the slot-basis model (tests/slots_basis_model.py) has the properties the scheme relies on, the library's host half
(fhesi_slots_basis_plan / fhesi_slots_basis_check: no device) agrees with it and refuses what is out of scope naming the condition, the
binding packs signed big integers into limbs as the model does, and the stored fixtures pin the convention."""
import json
import os
import random

import numpy as np
import pytest

import fhe_si_amd as F
import slots_basis_model as MB
import slots_pow2_model as M2

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("m,primes,g", [(8, [17, 41], 3), (16, [97, 17, 113], 5), (32, [193, 97, 257], 3), (64, [257, 193, 449, 577, 641], 5)])
def test_model_properties(m, primes, g):
    B, rnd = MB.SlotBasis(m, primes, g), random.Random(m + len(primes))
    P, n, half = B.modulus, B.total, (B.modulus - 1) // 2
    assert P % 2 == 1 and B.limbs == 1
    a = [half, -half, -1] + [rnd.randint(-half, half) for _ in range(n - 3)]
    b = [rnd.randint(-half, half) for _ in range(n)]
    ea, eb = MB.embed(B, a), MB.embed(B, b)
    assert MB.decode(B, ea) == a and MB.decode(B, ea, 3) == a[:3]
    # channel by channel: the operations of the two-row space act on the integers modulo P
    prod = [M2.poly_mul(B.channel(c), ea[c], eb[c]) for c in range(B.k)]
    assert MB.decode(B, prod) == [MB.centred(x * y, P) for x, y in zip(a, b)]
    rot = [M2.automorph(B.channel(c), ea[c], pow(g, 1, m)) for c in range(B.k)]
    assert MB.decode(B, rot) == M2.rotate_rows(B.channel(0), a, 1)
    swp = [M2.automorph(B.channel(c), ea[c], m - 1) for c in range(B.k)]
    assert MB.decode(B, swp) == M2.swap_rows(B.channel(0), a)
    # the order of the primes does not matter to the value
    B2 = MB.SlotBasis(m, primes[::-1], g)
    assert MB.decode(B2, MB.embed(B2, a)) == a


@pytest.mark.parametrize("m", [8, 16, 64, 1024, 4096, 1 << 15, 1 << 16])
@pytest.mark.parametrize("bits,prime_bits", [(20, 31), (73, 31), (73, 24), (200, 31), (600, 30), (900, 31)])
def test_plan_agrees_with_the_model(m, bits, prime_bits):
    try:
        exp = MB.plan(m, bits, prime_bits, 3)
    except ValueError as e:
        with pytest.raises(F.FhesiError) as got:
            F.slots_basis_plan(m, bits, prime_bits, 3)
        assert str(e) in str(got.value), str(got.value)
        return
    pl = F.slots_basis_plan(m, bits, prime_bits, 3)
    P = int(np.prod([int(p) for p in exp], dtype=object))
    assert pl["primes"] == exp and pl["limbs"] == MB.limbs_of(P)
    assert P > 1 << (bits + 1) and all(p < 1 << prime_bits and p % m == 1 for p in exp) and exp == sorted(exp, reverse=True)
    chk = F.slots_basis_check(m, exp, 3)
    assert (chk["limbs"], chk["modulus"]) == (pl["limbs"], P)


def test_plan_refusals():
    assert len(F.slots_basis_plan(1 << 16, 900, 31, 3)["primes"]) <= 32
    for args, word in [((1 << 16, 400, 20, 3), "not enough primes"), ((16, 400, 12, 3), "more than 32 primes"), ((64, 992, 31, 3), "more than 32 primes"), ((64, 993, 31, 3), "bits"), ((1 << 17, 64, 31, 3), "above 2^16"),
                       ((24, 64, 31, 3), "power of two"), ((4, 64, 31, 3), "k < 3"), ((64, 64, 31, 7), "mod 8"), ((64, 64, 32, 3), "prime_bits"), ((64, 0, 31, 3), "bits")]:
        with pytest.raises(F.FhesiError) as e:
            F.slots_basis_plan(*args)
        assert word in str(e.value), (args, str(e.value))


P31 = 2147473409           # the largest prime below 2^31 that is 1 mod 2^10
P32 = 2147493889           # the least prime above 2^31 that is 1 mod 2^10


@pytest.mark.parametrize("m,primes,g,word", [(16, [17, 97, 17], 3, "twice"), (32, [97, 17], 3, "ord_m(p) > 1"), (16, [17, 33], 3, "not prime"), (16, [289], 3, "not prime"),
                                             (1 << 10, [P31, P32], 3, "2^31"), (1 << 17, [786433], 3, "above 2^16"), (16, [], 3, "at least one"),
                                             (8, MB.plan(8, 500, 16, 3) + [17], 3, "more than 32 primes"), (16, [17, 97], 7, "mod 8"), (16, [17, 97], 1, "mod 8"),
                                             (24, [73], 5, "power of two"), (4, [5], 3, "k < 3")])
def test_refusals_name_the_condition(m, primes, g, word):
    assert MB.refusal(m, primes, g) == word
    with pytest.raises(F.FhesiError) as e:
        F.slots_basis_check(m, primes, g)
    assert word in str(e.value), str(e.value)


def test_check_accepts_what_the_model_accepts():
    for m, primes, g in [(16, [17], 3), (16, [97, 17, 113], 5), (1 << 10, [P31, 12289], 3), (8, MB.plan(8, 500, 16, 3), 5), (1 << 16, [65537, 786433], 3)]:
        B = MB.SlotBasis(m, primes, g)
        chk = F.slots_basis_check(m, primes, g)
        assert (chk["limbs"], chk["modulus"]) == (B.limbs, B.modulus)
    # the single-prime constructors are untouched: they still refuse / accept as before
    with pytest.raises(F.FhesiError):
        F.slots_plan(16, 17, 3)
    assert F.slots_plan_pow2(16, 17, 3)["path"] == 0


def test_limb_packing_of_signed_values():
    rnd = random.Random(7)
    for L in (1, 2, 3, 16):
        top = 1 << (64 * L - 1)
        vals = [0, 1, -1, top - 1, -top, -(1 << 64 * (L - 1)), (1 << 64 * (L - 1)) - 1] + [rnd.randint(-top, top - 1) for _ in range(20)]
        packed = F.pack_limbs(np.array(vals, dtype=object), L)
        assert packed.shape == (len(vals), L) and packed.dtype == np.int64
        assert [[int(x) & 0xFFFFFFFFFFFFFFFF for x in row] for row in packed] == [MB.to_limbs(v, L) for v in vals]
        assert [int(x) for x in F.unpack_limbs(packed)] == vals == [MB.from_limbs(row) for row in packed]
    # int64 arrays: one limb as they are, sign-extended when more are asked for
    a = np.array([[-5, 7, -(1 << 63), (1 << 63) - 1]], dtype=np.int64)
    assert np.array_equal(F.pack_limbs(a)[..., 0], a) and F.pack_limbs(a).shape == (1, 4, 1)
    assert [int(x) for x in F.unpack_limbs(F.pack_limbs(a, 3))[0]] == [int(x) for x in a[0]]
    assert F.pack_limbs(np.array([1 << 64, -1], dtype=object)).shape == (2, 2)
    with pytest.raises(ValueError):
        F.pack_limbs(np.array([1 << 64], dtype=object), 1)


def test_fixtures_pin_the_convention():
    cases = json.load(open(os.path.join(G, "slots_basis.json")))["cases"]
    assert len(cases) >= 5 and any(c["limbs"] > 1 for c in cases)
    for c in cases:
        B = MB.SlotBasis(c["m"], c["primes"], c["g"])
        vals = [int(v) for v in c["vals"]]
        assert (str(B.modulus), B.limbs) == (c["modulus"], c["limbs"])
        assert MB.embed(B, vals) == c["msg"]
        assert MB.decode(B, c["msg"]) == vals
        for ch in range(B.k):
            assert F.slots_plan_pow2(c["m"], c["primes"][ch], c["g"])["rho0"] == B.channel(ch).rho0
        chk = F.slots_basis_check(c["m"], c["primes"], c["g"])
        assert (str(chk["modulus"]), chk["limbs"]) == (c["modulus"], c["limbs"])
