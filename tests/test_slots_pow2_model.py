"""CPU: the two-row slot model of the power-of-two rings (tests/slots_pow2_model.py) has the properties the scheme relies on, the library's
host half (fhesi_slots_plan_pow2: no device) agrees with it and refuses what is out of scope, the single-generator constructor keeps refusing
these rings, and the stored fixtures pin the convention."""
import json
import os
import random

import pytest

import fhe_si_amd as F
import slots_pow2_model as M2

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P31 = 2147473409           # the largest prime below 2^31 that is 1 mod 2^10
P32 = 2147493889           # the least prime above 2^31 that is 1 mod 2^10
RINGS = [(8, 17, 3), (8, 17, 5), (16, 17, 3), (16, 97, 5), (32, 97, 3), (32, 193, 13), (64, 257, 5), (64, 257, 11), (128, 257, 3), (256, 257, 5), (256, 7681, 3)]


@pytest.mark.parametrize("m,p,g", RINGS)
def test_model_properties(m, p, g):
    S = M2.slot_space(m, p, g)
    n, h, rnd = S.total, S.cols, random.Random(m * p + g)
    assert (S.rows, S.cols, S.usable) == (2, m // 4, n)
    assert pow(S.rho0, n, p) == p - 1 and all(pow(x, n, p) != p - 1 for x in range(1, S.rho0))
    a = [rnd.randrange(p) for _ in range(n)]
    b = [rnd.randrange(p) for _ in range(n)]
    # 1. round trip, linearity, slot-wise products modulo X^n + 1
    ea, eb = M2.embed_slots(S, a), M2.embed_slots(S, b)
    assert M2.decode_slots(S, ea) == a
    assert M2.embed_slots(S, [(3 * x + y) % p for x, y in zip(a, b)]) == [(3 * x + y) % p for x, y in zip(ea, eb)]
    assert M2.decode_slots(S, M2.poly_mul(S, ea, eb)) == [x * y % p for x, y in zip(a, b)]
    assert M2.decode_slots(S, M2.embed_slots(S, a[:3])) == a[:3] + [0] * (n - 3)
    # 2. X -> X^(g^t) rotates BOTH rows left by t; X -> X^(m - 1) swaps the rows
    for t in (1, 2, h - 1):
        assert M2.decode_slots(S, M2.automorph(S, ea, pow(g, t, m))) == M2.rotate_rows(S, a, t)
    assert M2.decode_slots(S, M2.automorph(S, ea, m - 1)) == M2.swap_rows(S, a)
    # 3. the total-sum walk: log2 n automorphisms leave the sum of all slots in EVERY slot
    ks, cur = M2.total_sum_exponents(S), ea
    assert len(ks) == n.bit_length() - 1 and 1 not in ks and ks[-1] == m - 1
    for k in ks:
        cur = [(x + y) % p for x, y in zip(cur, M2.automorph(S, cur, k))]
    assert M2.decode_slots(S, cur) == [sum(a) % p] * n


@pytest.mark.parametrize("m,p,g", RINGS + [(4096, 65537, 3), (1 << 16, 65537, 5), (1 << 17, 786433, 3), (1 << 10, P31, 3), (1 << 10, P32, 5)])
def test_library_host_half_agrees_with_the_model(m, p, g):
    S, pl = M2.slot_space(m, p, g), F.slots_plan_pow2(m, p, g)
    assert (pl["total"], pl["rows"], pl["cols"], pl["rho0"], pl["path"]) == (S.total, 2, S.cols, S.rho0, S.path)
    assert [int(x) for x in pl["exps"]] == S.exps


def test_the_plan_picks_the_path_at_the_boundaries():
    assert F.slots_plan_pow2(1 << 16, 65537, 3)["path"] == 0           # n = 2^15: the row still fits one workgroup's LDS
    assert F.slots_plan_pow2(1 << 17, 786433, 3)["path"] == 1          # n = 2^16: chirp, one auxiliary prime
    assert F.slots_plan_pow2(1 << 10, P31, 3)["path"] == 0             # p < 2^31: lazy values below 2p fit a word
    assert F.slots_plan_pow2(1 << 10, P32, 3)["path"] == 2             # p >= 2^31: chirp; 2^10 p^2 > 2^59 takes two primes
    assert F.slots_plan_pow2(1 << 20, 7340033, 3)["path"] == 2          # every m up to 2^20 has a path


@pytest.mark.parametrize("m,p,g,word", [(4, 5, 3, "k < 3"), (2, 3, 1, "k < 3"), (24, 73, 5, "power of two"), (22, 23, 7, "power of two"), (16, 33, 3, "not prime"),
                                        (16, 289, 3, "not prime"), (16, 4294967377, 3, "2^32"), (1 << 15, 23, 3, "ord_m(p) > 1"), (32, 17, 3, "ord_m(p) > 1"),
                                        (16, 17, 7, "mod 8"), (16, 17, 1, "mod 8"), (16, 17, 15, "mod 8"), (16, 17, 4, "mod 8"), (1 << 21, 23068673, 3, "2^20")])
def test_refusals_name_the_condition(m, p, g, word):
    with pytest.raises(F.FhesiError) as e:
        F.slots_plan_pow2(m, p, g)
    assert word in str(e.value), str(e.value)
    assert m > 1 << 20 or M2.refusal(m, p, g) is not None


def test_the_single_generator_constructor_still_refuses_these_rings():
    for m, p, g in [(16, 17, 3), (4096, 65537, 3), (1 << 16, 65537, 5)]:
        with pytest.raises(F.FhesiError) as e:
            F.slots_plan(m, p, g)
        assert "not cyclic" in str(e.value)
    assert F.slots_plan(4, 5, 3)["total"] == 2


def test_fixtures_pin_the_convention():
    cases = json.load(open(os.path.join(G, "slots_pow2.json")))["cases"]
    assert len(cases) >= 5
    for c in cases:
        S = M2.slot_space(c["m"], c["p"], c["g"])
        assert (S.rho0, S.exps) == (c["rho0"], c["exps"])
        assert M2.embed_slots(S, c["vals"]) == c["msg"]
        assert M2.decode_slots(S, c["msg"]) == c["vals"]
        pl = F.slots_plan_pow2(c["m"], c["p"], c["g"])
        assert pl["rho0"] == c["rho0"] and [int(x) for x in pl["exps"]] == c["exps"]
