"""CPU (no GPU): the model of the polynomial evaluation on packed slots (tests/poly_model.py) -- its schedule evaluates to f(v) mod p for every degree
and every baby step, its planner is the brute-force minimum, the library's host-only planner (fhesi_poly_eval_plan) equals it, the header declares the
three entry points at ABI revision 9, and the schedule runs end to end through the Python model of the scheme (oracle/fhesi_pyref.py) at
(64, 257, logQ 256): decryption equals f in every slot and the noise budget is positive."""
import os
import random
import re

import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import noise_model as NM
import params as P
import poly_model as PM
import slots_pow2_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f_of(coef, v, p):
    return sum(int(c) * pow(v, k, p) for k, c in enumerate(coef)) % p


def patterns(rng, d, p):
    """coefficient lists of degree d: dense with the planted values, a random zero pattern, c_d = 0 (given as p), all = 0 (mod p), the monomial x^8"""
    dense = [rng.randrange(-3 * p, 3 * p) for _ in range(d + 1)]
    special = [0, p - 1, p, -1, -p, 1 << 62, -(1 << 62)]
    for i, v in zip(rng.sample(range(d + 1), min(d + 1, len(special))), special):
        dense[i] = v
    sparse = [c if rng.random() < 0.4 else rng.choice((0, p, -p)) for c in dense]
    top0 = dense[:d] + [p]
    zero = [rng.choice((0, p, -p)) for _ in range(d + 1)]
    out = [dense, sparse, top0, zero]
    if d >= 8:
        out.append([0] * 8 + [1] + [0] * (d - 8))
    return out


@pytest.mark.parametrize("p", [257, 65537])
def test_schedule_evaluates_to_f_for_every_degree_and_baby_step(p):
    rng = random.Random(p)
    for d in range(1, 65):
        pats = patterns(rng, d, p)
        vs = [0, 1, p - 1, rng.randrange(p), rng.randrange(p)]
        for B in range(1, d + 1):
            for coef in pats:
                s = PM.schedule(coef, p, B)
                assert (s["B"], s["G"]) == (B, d // B + 1)
                for v in vs:
                    assert PM.evaluate(s, v, p) == f_of(coef, v, p) == PM.horner(coef, v, p), (d, B, coef, v)
    # the planner's B
    for d in (1, 2, 3, 7, 15, 31, 64):
        coef = [rng.randrange(p) for _ in range(d + 1)]
        s = PM.schedule(coef, p)
        assert s["B"] == PM.plan(d)["B"] and PM.evaluate(s, 5, p) == f_of(coef, 5, p)


def schedule_counts(s):
    """products, key switches and multiplicative depth counted on the schedule itself"""
    depth = {1: 0}
    for level in s["levels"]:
        for k, a, b in level:
            depth[k] = max(depth[a], depth[b]) + 1
    nprod = sum(len(level) for level in s["levels"]) + len(s["pairs"])
    final_refs = [ref[1] for _, ref in s["final"][0] if ref[0] == "x"]
    dd = max([depth[k] for k in final_refs] + [max(max(depth[j] for _, j in terms), depth[k]) + 1 for (g, terms, _), (_, k) in zip(s["inner"], s["pairs"])] + [0])
    return {"B": s["B"], "G": s["G"], "nprod": nprod, "nks": PM.key_switches(s), "depth": dd}


def test_counts_are_the_schedules_and_the_planner_is_the_brute_force_minimum():
    for d in range(1, 97):
        dense = [1] * (d + 1)
        every = [schedule_counts(PM.schedule(dense, 257, B)) for B in range(1, d + 1)]
        for B, c in enumerate(every, 1):
            want = PM.counts(d, B)
            # (the stated depth is that of the top giant behind a pair; where B divides d the top giant has no pair and the schedule may be one shallower)
            assert c["depth"] <= want["depth"] and (c["depth"] == want["depth"] or (d % B == 0 and B >= 2 and d // B >= 2)), (d, B)
            assert {**c, "depth": want["depth"]} == want, (d, B)
        assert PM.plan(d) == min((PM.counts(d, B) for B in range(1, d + 1)), key=lambda c: (c["nks"], c["depth"], -c["B"])), d
    assert PM.plan(15) == {"B": 4, "G": 4, "nprod": 8, "nks": 6, "depth": 5}
    # every power is there whatever the zero pattern, every level reads earlier levels only, destinations of a level are consecutive pool entries
    for d, B in ((16, 3), (15, 4), (7, 1), (8, 8)):
        s = PM.schedule([0] * (d + 1), 257, B)
        assert sorted(k for level in s["levels"] for k, _, _ in level) == list(range(2, B + 1)) + [g * B for g in range(2, d // B + 1)]
        have = {1}
        for level in s["levels"]:
            assert all(a in have and b in have and a + b == k for k, a, b in level)
            e = [PM.pool_entry(k, B) for k, _, _ in level]
            assert e == list(range(e[0], e[0] + len(e)))
            have |= {k for k, _, _ in level}
        assert not s["inner"] and not s["pairs"] and s["final"] == ([], 0)


def test_refused_shapes():
    for d, B in ((0, 0), (4097, 0), (5, 6), (5, -1)):
        with pytest.raises(ValueError):
            PM.plan(d, B)


def test_library_planner_equals_the_model():
    for d in range(1, 257):
        for baby in sorted({0, 1, min(3, d), d}):
            assert F.poly_eval_plan(d, baby) == PM.plan(d, baby), (d, baby)
    assert F.poly_eval_plan(4096)["B"] == PM.plan(4096)["B"]
    for d, baby, word in ((0, 0, "degree"), (4097, 0, "degree"), (5, 6, "baby"), (5, -1, "baby")):
        with pytest.raises(F.FhesiError) as e:
            F.poly_eval_plan(d, baby)
        assert word in str(e.value)


def test_header_declares_the_entry_points_at_revision_9():
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    assert re.search(r"#define FHESI_ABI_VERSION 9\b", text)
    for name in ("fhesi_ct_lin_comb_dev", "fhesi_poly_eval_plan", "fhesi_ct_poly_eval_dev"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in F.binding.ABI_SYMBOLS
    assert F.binding.ABI_VERSION == 9


# ------------------------------------------------------------------------------------------------ through the Python model of the scheme
def lin_comb(ctx, terms, konst):
    """the composition fhesi_ct_lin_comb_dev is defined as: Ciphertext *= long and += per term, += ZZX with (konst, 0, .., 0)"""
    n = ctx.phim
    acc = [[0] * n, [0] * n]
    for c, parts in terms:
        acc = R.ct_add(ctx, acc, R.ct_mul_long(ctx, parts, c))
    return R.ct_add_const(ctx, acc, [konst] + [0] * (n - 1))


def run_schedule(ctx, ksm, s, x):
    pw = {1: x}
    for level in s["levels"]:
        pw.update({k: R.ct_mul_relin(ctx, ksm, pw[a], pw[b]) for k, a, b in level})
    u = {g: lin_comb(ctx, [(c, pw[j]) for c, j in terms], konst) for g, terms, konst in s["inner"]}
    W = None
    if s["pairs"]:
        tp = None
        for g, k in s["pairs"]:
            t = R.ct_mul(ctx, u[g], pw[k])
            tp = t if tp is None else R.tprod_add(ctx, tp, t)
        W = R.apply_key_switch(ctx, ksm, tp)                                # one key switch for the whole outer sum
    terms, konst = s["final"]
    return lin_comb(ctx, [(c, W if ref[0] == "W" else pw[ref[1]]) for c, ref in terms], konst)


@pytest.mark.parametrize("d", [7, 15])
def test_schedule_through_the_scheme_model(d):
    m, p, logQ, g = 64, 257, 256, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, list(primes), list(roots))
    rng = R.SplitMix64(0xC0FFEE + d)
    t, pk = R.keygen(ctx, rng)
    ksm = R.key_switch_init_s2(ctx, t, rng)
    S = SM.slot_space(m, p, g)
    rnd = random.Random(d)
    vals = [rnd.randrange(p) for _ in range(ctx.phim)]
    vals[:3] = [0, 1, p - 1]
    coef = [rnd.randrange(-p, 2 * p) for _ in range(d + 1)]
    x = R.encrypt(ctx, pk, SM.embed_slots(S, vals, only_usable=False), rng)
    s = PM.schedule(coef, p)
    assert s["B"] == PM.plan(d)["B"]
    y = run_schedule(ctx, ksm, s, x)
    msg, _, budget = NM.noise(ctx, R.dcrt_from_poly(ctx, t), y)
    print(f"degree {d}: B = {s['B']}, {PM.key_switches(s)} key switches, model budget {budget} of {logQ}")
    assert SM.decode_slots(S, msg, only_usable=False) == [f_of(coef, v, p) for v in vals]
    assert msg == R.decrypt(ctx, t, y)
    assert budget > 0
