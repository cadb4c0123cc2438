"""CPU: the slot-packing model (tests/slots_model.py) has the properties every observable of the reference depends on, the two identities the
device kernels rest on hold, the library's host half (fhesi_slots_plan: no device) agrees with the model and refuses the rings out of
scope, and the stored fixtures pin the slot convention."""
import json
import os
import random

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import slots_model as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RINGS = [(2, 3, 1), (4, 5, 3), (9, 19, 2), (22, 23, 7), (22, 67, 7), (46, 47, 5), (50, 101, 3), (25, 101, 2), (27, 109, 2), (54, 109, 5)]


@pytest.mark.parametrize("m,p,g", RINGS)
def test_model_properties(m, p, g):
    S = M.slot_space(m, p, g)
    n, rnd = S.total, random.Random(m * p)
    assert M.order_mod(S.rho0, p) == m and all(M.order_mod(x, p) != m for x in range(1, S.rho0))
    assert sorted(S.exps) == [x for x in range(1, m) if np.gcd(x, m) == 1] or m == 2
    a = [rnd.randrange(p) for _ in range(n)]
    b = [rnd.randrange(p) for _ in range(n)]
    # 1. round trip, linearity, slot-wise products
    assert M.decode_slots(S, M.embed_slots(S, a, False), n, False) == a
    ea, eb = M.embed_slots(S, a, False), M.embed_slots(S, b, False)
    assert M.embed_slots(S, [(3 * x + y) % p for x, y in zip(a, b)], False) == [(3 * x + y) % p for x, y in zip(ea, eb)]
    assert M.decode_slots(S, M.poly_mul_mod_phi(S, ea, eb), n, False) == [x * y % p for x, y in zip(a, b)]
    # 2. X -> X^(g^t) rotates left by t
    for t in (1, 2, n - 1):
        assert M.decode_slots(S, M.automorph_mod_phi(S, ea, pow(g, t, m)), n, False) == a[t % n:] + a[:t % n]
    # 3. only_usable
    assert S.usable == 1 << (n.bit_length() - 1)
    assert M.decode_slots(S, M.embed_slots(S, a, True), n, False) == a[:S.usable] + [0] * (n - S.usable)
    assert M.decode_slots(S, ea, n, True) == a[:S.usable] + [0] * (n - S.usable)
    assert M.decode_slots(S, M.embed_slots(S, a[:1], True), n, False) == a[:1] + [0] * (n - 1)
    # 4. SumBatchedData: automorphisms g, g^2, g^4, ... leave the sum of the usable slots in slot 0
    cur, k = M.embed_slots(S, a, True), g
    for _ in R.automorph_generators(m, g, S.usable):
        cur = [(x + y) % p for x, y in zip(cur, M.automorph_mod_phi(S, cur, k))]
        k = k * k % m
    assert M.decode_slot(S, cur, 0) == sum(a[:S.usable]) % p


@pytest.mark.parametrize("m,p,g", RINGS)
def test_triangular_chirp_and_phi_fold(m, p, g):
    """i k = T(k) + T'(i) - T(k - i) turns the DFT into one convolution with m-th roots only; the remainder modulo Phi_m of the admitted
    rings is a fold of at most four coefficients (against poly_rem_monic)."""
    S = M.slot_space(m, p, g)
    rnd = random.Random(m + p)
    rho = S.rho0
    T = lambda x: x * (x - 1) // 2
    Tp = lambda i: i * (i + 1) // 2
    a = [rnd.randrange(p) for _ in range(S.total)]
    for k in range(m):
        direct = sum(c * pow(rho, i * k, p) for i, c in enumerate(a)) % p
        chirp = pow(rho, T(k) % m, p) * sum(c * pow(rho, Tp(i) % m, p) * pow(rho, (-T(k - i)) % m, p) for i, c in enumerate(a)) % p
        assert direct == chirp
    f = [rnd.randrange(p) for _ in range(m)]
    fs = sorted(set(R.factorize(m)))
    if len(fs) == 1:
        q = fs[0]
        s = m // q
        out = [(f[i * s + r] - f[(q - 1) * s + r]) % p for i in range(q - 1) for r in range(s)]
    else:
        q = fs[1]
        Q, s = m // 2, m // 2 // q
        h = [(f[j] - f[j + Q]) % p for j in range(Q)]
        out = [(h[i * s + r] - (-1) ** i * h[(q - 1) * s + r]) % p for i in range(q - 1) for r in range(s)]
    assert out == R.poly_rem_monic(list(f), S.phi, p)


@pytest.mark.parametrize("m,p,g", RINGS + [(2026, 2027, 3), (8422, 8423, 3), (22, (1 << 31) - 1, 7)])
def test_library_host_half_agrees_with_the_model(m, p, g):
    if m == 8422:
        g = M.least_generator(m)
    S, pl = M.slot_space(m, p, g), F.slots_plan(m, p, g)
    assert (pl["total"], pl["usable"], pl["rho0"]) == (S.total, S.usable, S.rho0)
    assert [int(x) for x in pl["exps"]] == S.exps
    assert pl["aux_primes"] == (1 if m * p * p < 1 << 59 else 2)


@pytest.mark.parametrize("m,p,g,word", [(1 << 15, 23, 3, "ord_m(p) > 1"), (16, 17, 3, "not cyclic"), (15, 31, 2, "not cyclic"), (22, 23, 3, "generator"),
                                        (22, 23, 11, "generator"), (22, 4294967311, 7, "2^32"), (22, 45, 7, "not prime"), (22, 529, 7, "not prime")])
def test_refusals_name_the_condition(m, p, g, word):
    with pytest.raises(F.FhesiError) as e:
        F.slots_plan(m, p, g)
    assert word in str(e.value)
    assert M.refusal(m, p, g) is not None


def test_fixtures_pin_the_convention():
    cases = json.load(open(os.path.join(G, "slots.json")))["cases"]
    assert len(cases) >= 5
    for c in cases:
        S = M.slot_space(c["m"], c["p"], c["g"])
        assert (S.rho0, S.exps) == (c["rho0"], c["exps"])
        assert M.embed_slots(S, c["vals"], False) == c["msg"]
        assert M.decode_slots(S, c["msg"], S.total, False) == c["vals"]
        pl = F.slots_plan(c["m"], c["p"], c["g"])
        assert pl["rho0"] == c["rho0"] and [int(x) for x in pl["exps"]] == c["exps"]
