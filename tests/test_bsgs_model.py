"""CPU: the baby-step/giant-step identity in slot terms (numpy) and on the model (tests/bsgs_model.py over tests/hoist_model.py and
oracle/fhesi_pyref.py), the planner against brute force, and the symbols the feature adds to the header and the binding.  Exact."""
import os
import re

import numpy as np
import pytest

import bsgs_model as B
import fhesi_pyref as R
import hoist_model as H
import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fhesi_ct_rot_sum_dev", "fhesi_matvec_bsgs_plan", "fhesi_ct_matvec_bsgs_dev")


@pytest.mark.parametrize("rows,total", [(1, 6), (1, 100), (2, 8), (2, 128)])
def test_the_slot_identity_for_every_split_of_up_to_twelve_diagonals(rows, total):
    """sum_g roll( sum_j roll(d_{gB+j}, +gB) o roll(x, -j), -gB ) = sum_t d_t o roll(x, -t) in every row, for every (B, G) with B G >= T -- ragged last
    groups, B = 1, G = 1, and rotations past a row's length included"""
    p = 65537
    rng = np.random.default_rng(total)
    x = rng.integers(0, p, size=total)
    cols = total // rows
    assert np.array_equal(B.rotate_values(x, 1, rows).reshape(rows, cols), np.roll(x.reshape(rows, cols), -1, axis=1))
    assert np.array_equal(B.rotate_values(B.rotate_values(x, 5, rows), -5, rows), x)
    for T in range(1, 13):
        d = rng.integers(0, p, size=(T, total))
        want = B.slot_matvec(d, x, p, rows)
        direct = np.zeros(total, dtype=object)
        for t in range(T):
            direct = (direct + d[t].astype(object) * np.roll(x.reshape(rows, cols), -t, axis=1).reshape(-1).astype(object)) % p
        assert list(want) == list(direct), T
        for b in range(1, T + 1):
            assert list(B.slot_matvec_bsgs(d, x, b, p, rows)) == list(want), (T, b)
        assert list(B.slot_matvec_bsgs(d, x, T + 3, p, rows)) == list(want), T      # one ragged group


@pytest.mark.parametrize("m,p,gen", [(256, 257, 3),        # power of two: sigma is a signed permutation of the coefficients
                                     (250, 251, 3)])       # 2 x 5^3: sigma reduces modulo Phi_m
def test_the_model_decrypts_like_the_flat_product_and_is_it_when_there_is_one_giant(m, p, gen):
    logQ = 128
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, primes, roots)
    rng = R.SplitMix64(4000 + m)
    t, pk = R.keygen(ctx, rng)
    n = ctx.phim
    msg = [(5 * i * i + 2 * i + 1) % p for i in range(n)]
    ct = R.encrypt(ctx, pk, msg, rng)
    T, b = 5, 2                                                                      # G = 3, the last group ragged
    G = -(-T // b)
    ks = [pow(gen, e, m) for e in range(T)]
    mats = {1: None}
    for k in set(ks) | {pow(gen, g * b, m) for g in range(G)}:
        if k != 1:
            mats[k] = H.hoist_matrix(ctx, R.key_switch_init_automorph(ctx, t, k, rng), k)
    diags = [[(3 * j + 7 * i + 1) % p for i in range(n)] for j in range(T)]
    flat = H.matvec(ctx, [mats[k] for k in ks], ks, diags, ct)
    kb, kg = ks[:b], [pow(gen, g * b, m) for g in range(G)]
    got = B.matvec_bsgs(ctx, [mats[k] for k in kb], kb, [mats[k] for k in kg], kg, T, B.bsgs_polys(ctx, diags, kg, b), ct)
    want = [0] * n
    for k, w in zip(ks, diags):
        want = [(a + c) % p for a, c in zip(want, R.poly_mul_mod_phi(ctx, H.automorph_message(ctx, msg, k), w))]
    assert R.decrypt(ctx, t, got) == want == R.decrypt(ctx, t, flat)
    assert got != flat                                                               # other key switches, other words
    # one giant step, the identity: the flat product itself
    assert B.matvec_bsgs(ctx, [mats[k] for k in ks], ks, [None], [1], T, diags, ct) == flat
    assert B.matvec_bsgs(ctx, [mats[k] for k in ks] + [None], ks + [1], [None], [1], T, diags, ct) == flat      # ragged: a baby past nk is not run


def test_the_planner_is_the_brute_force_minimum():
    import fhe_si_amd as F
    for nk in range(1, 301):
        b, g = F.matvec_bsgs_plan(nk)
        assert (b, g) == B.plan(nk), nk
        assert (g - 1) * b < nk <= g * b
        assert all(b + g <= bb + -(-nk // bb) for bb in range(1, nk + 1)), nk
    assert F.matvec_bsgs_plan(16) == (4, 4) and F.matvec_bsgs_plan(64) == (8, 8) and F.matvec_bsgs_plan(1024) == (32, 32)
    assert F.matvec_bsgs_plan(2) == (2, 1) and F.matvec_bsgs_plan(12) == (4, 3)      # ties go to the larger B
    for bad in (0, -3, (1 << 20) + 1):
        with pytest.raises(F.FhesiError, match="matvec_bsgs_plan"):
            F.matvec_bsgs_plan(bad)


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert int(re.search(r"#define\s+FHESI_ROT_SUM_MAX_TERMS\s+(\d+)", src).group(1)) == F.binding.ROT_SUM_MAX_TERMS
    for name in ("ct_rot_sum_dev", "ct_matvec_bsgs_dev"):
        assert hasattr(F.Context, name)
    for name in ("rotate_values", "bsgs_diagonals", "matvec_bsgs"):
        assert hasattr(F.SlotSpace, name)
    assert hasattr(F.SlotBasis, "matvec_bsgs")
