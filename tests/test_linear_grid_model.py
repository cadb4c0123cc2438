"""CPU: the block-grid identity in slot terms (tests/linear_grid_model.py) against brute force M x + b, the host-only planner fhesi_linear_grid_plan
against the model's over every admitted block shape, its tie rule, the 1 x 1 grid against fhesi_linear_plan, the key-switch counts and the refusals.
Exact."""
import os
import re

import numpy as np
import pytest

import linear_grid_model as GM
import linear_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, P = 2, 16, 257
# (Rb, Cb) x (nI, nJ)
SHAPES = [((4, 4), (2, 3)), ((16, 16), (2, 2)), ((4, 16), (3, 1)), ((4, 16), (2, 2)), ((16, 4), (1, 3)), ((1, 1), (2, 2)), ((8, 8), (3, 2)),
          ((1, 8), (2, 2)), ((8, 8), (1, 1))]
SYMBOLS = ("fhesi_linear_grid_plan", "fhesi_linear_grid_create", "fhesi_linear_grid_create_dev", "fhesi_linear_grid_free", "fhesi_linear_grid_info",
           "fhesi_linear_grid_diagonals", "fhesi_ct_linear_grid_dev")


def blocks(cols):
    return [(R, C) for R in range(1, cols + 1) for C in range(1, cols + 1) if LM.admitted(cols, R, C) is None]


@pytest.mark.parametrize("block,grid", SHAPES)
def test_the_grid_is_the_matrix_vector_product(block, grid):
    """every slot of every row of every output block = (M x_r + b)[I Rb + (i mod Rb)]: the planner's B and B = 3 (ragged, a negative wrap), with bias"""
    (Rb, Cb), (nI, nJ) = block, grid
    rng = np.random.default_rng(Rb * 1000 + Cb * 10 + nI)
    M = rng.integers(0, P, size=(nI * Rb, nJ * Cb))
    x = rng.integers(0, P, size=(ROWS, nJ * Cb))
    xs = GM.replicate_blocks(x, Cb, ROWS, COLS)
    assert xs.shape == (nJ, ROWS * COLS)
    for baby in (0, 3):
        for bias in (None, rng.integers(0, P, size=nI * Rb)):
            got = GM.grid(M, bias, xs, Rb, Cb, P, ROWS, baby)
            want = GM.expected_slots(M, bias, x, Rb, P, ROWS, COLS)
            assert [list(y) for y in got] == want, (block, grid, baby, bias is not None)


def test_a_one_by_one_grid_is_the_layer():
    """the model's 1 x 1 grid computes what linear_model.layer computes, and its prepared diagonals are the layer's"""
    rng = np.random.default_rng(1)
    for Rb, Cb in blocks(COLS):
        M, b = rng.integers(0, P, size=(Rb, Cb)), rng.integers(0, P, size=Rb)
        xs = GM.replicate_blocks(rng.integers(0, P, size=(ROWS, Cb)), Cb, ROWS, COLS)
        for baby in (0, 3):
            assert list(GM.grid(M, b, xs, Rb, Cb, P, ROWS, baby)[0]) == list(LM.layer(M, b, xs[0], P, ROWS, baby)), (Rb, Cb, baby)
            B = LM.plan(COLS, Rb, Cb, baby)["B"]
            assert np.array_equal(GM.prepared(M, Rb, Cb, ROWS, COLS, B)[0][0], LM.prepared(M, ROWS, COLS, B))


def test_the_planner_equals_the_model_on_every_block_and_grid():
    import fhe_si_amd as F
    todo = blocks(COLS)
    assert len(todo) == 25
    for Rb, Cb in todo:
        for nI in range(1, 5):
            for nJ in range(1, 5):
                for baby in (0, 3):
                    got = F.linear_grid_plan(COLS, nI * Rb, nJ * Cb, Rb, Cb, baby)
                    assert got == GM.plan(COLS, nI * Rb, nJ * Cb, Rb, Cb, baby), (Rb, Cb, nI, nJ, baby)
        for baby in (0, 1, 3, 7, 5000):                          # one block plans as the layer does
            got = F.linear_grid_plan(COLS, Rb, Cb, Rb, Cb, baby)
            want = F.linear_plan(COLS, Rb, Cb, baby)
            assert {k: got[k] for k in want} == want and (got["nI"], got["nJ"]) == (1, 1), (Rb, Cb, baby)
    # rows the tests of the device run on: 1024 and 16384 slots
    for cols, Rb, Cb, nI, nJ in ((1024, 64, 64, 4, 4), (1024, 1024, 1024, 2, 2), (16384, 64, 64, 4, 4), (1024, 16, 1024, 3, 2)):
        assert F.linear_grid_plan(cols, nI * Rb, nJ * Cb, Rb, Cb) == GM.plan(cols, nI * Rb, nJ * Cb, Rb, Cb)


def test_the_tie_rule_takes_the_larger_baby_step():
    """every square block of T diagonals in every grid up to 4 x 4: the B of least cost, and where several B cost the same -- found by search -- the
    largest of them; one tie written out"""
    import fhe_si_amd as F
    ties = 0
    for T in (1, 2, 4, 8, 16):
        for nI in range(1, 5):
            for nJ in range(1, 5):
                costs = {B: GM.cost(nI, nJ, T, B) for B in range(1, T + 1)}
                least = min(costs.values())
                best = [B for B, c in costs.items() if c == least]
                ties += len(best) > 1
                got = F.linear_grid_plan(COLS, nI * T, nJ * T, T, T)
                assert got["B"] == max(best) and got["G"] == -(-T // got["B"]), (T, nI, nJ, best, got)
    assert ties >= 5
    # written out: T = 4 in a 1 x 2 grid -- B = 1 costs 0 + 3 giants, B = 2 costs 2 babies + 1 giant, B = 4 costs 6 babies: 3, 3, 6 -> B = 2
    assert (GM.cost(1, 2, 4, 1), GM.cost(1, 2, 4, 2), GM.cost(1, 2, 4, 4)) == (3, 3, 6) and F.linear_grid_plan(COLS, 4, 8, 4, 4)["B"] == 2


def test_the_key_switch_counts():
    """nJ (B - 1) + nI (G - 1) + nI nfold against nI nJ (B + G - 2 + nfold): the three cases of the design note, and never more than per block"""
    import fhe_si_amd as F
    for (Rb, Cb), (nI, nJ), shared, each in (((8, 8), (3, 2), 9, 24), ((16, 16), (2, 2), 12, 24), ((4, 16), (2, 2), 8, 16)):
        pl = F.linear_grid_plan(COLS, nI * Rb, nJ * Cb, Rb, Cb)
        assert pl["key_switches"] == shared == pl["nJ"] * (pl["B"] - 1) + pl["nI"] * (pl["G"] - 1) + pl["nI"] * pl["nfold"], (Rb, Cb, nI, nJ, pl)
        assert GM.per_block_key_switches(COLS, nI * Rb, nJ * Cb, Rb, Cb) == each
    for Rb, Cb in blocks(COLS):
        for nI in range(1, 5):
            for nJ in range(1, 5):
                pl = GM.plan(COLS, nI * Rb, nJ * Cb, Rb, Cb)
                assert pl["key_switches"] <= GM.per_block_key_switches(COLS, nI * Rb, nJ * Cb, Rb, Cb)
                assert len(pl["amounts"]) == pl["B"] - 1 + pl["G"] - 1 + pl["nfold"]


@pytest.mark.parametrize("cols,R,C,Rb,Cb", [(16, 9, 8, 8, 8), (16, 8, 12, 8, 8),                       # not a multiple of the block
                                            (16, 0, 8, 8, 8), (16, 8, 0, 8, 8), (16, 8, 8, 0, 8),      # zero sizes
                                            (16, 64, 8, 32, 8), (24, 32, 8, 16, 4), (24, 16, 24, 8, 12), (24, 8, 24, 4, 12),      # the block's shape
                                            (1 << 16, 1 << 17, 1 << 16, 1 << 16, 1 << 16), (1024, 1024 * 8, 1024 * 9, 1024, 1024)])      # too many diagonals
def test_the_planner_refuses_with_the_condition_named(cols, R, C, Rb, Cb):
    import fhe_si_amd as F
    word = GM.refused(cols, R, C, Rb, Cb)
    assert word is not None
    with pytest.raises(F.FhesiError) as e:
        F.linear_grid_plan(cols, R, C, Rb, Cb)
    assert word in str(e.value), (word, str(e.value))
    if LM.admitted(cols, Rb, Cb) is not None:                   # the block's shape: the layer planner's own words
        with pytest.raises(F.FhesiError) as e2:
            F.linear_plan(cols, Rb, Cb)
        assert str(e2.value) == str(e.value)
    with pytest.raises(F.FhesiError, match="baby steps"):
        F.linear_grid_plan(16, 8, 8, 4, 4, -1)


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert hasattr(F, "linear_grid_plan") and hasattr(F, "LinearGrid") and F.binding.ABI_VERSION == 9
    for name in ("linear_grid", "linear_grid_diagonals", "replicate_blocks", "collect_blocks"):
        assert hasattr(F.SlotSpace, name)
    for name in ("apply", "close"):
        assert hasattr(F.LinearGrid, name)
