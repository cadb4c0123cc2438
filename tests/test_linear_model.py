"""CPU: the dense-layer identity in slot terms (tests/linear_model.py) against brute force M x + b for every admitted shape, the host-only planner
fhesi_linear_plan against the model's, its refusals, and the symbols the feature adds to the header and the binding.  Exact."""
import os
import re

import numpy as np
import pytest

import bsgs_model as BM
import linear_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fhesi_linear_plan", "fhesi_linear_create", "fhesi_linear_create_dev", "fhesi_linear_free", "fhesi_linear_info", "fhesi_linear_diagonals",
           "fhesi_ct_rot_fold_dev", "fhesi_ct_linear_dev")
BABIES = (0, 1, 3)


def shapes(cols):
    return [(R, C) for R in range(1, cols + 1) for C in range(1, cols + 1) if LM.admitted(cols, R, C) is None]


@pytest.mark.parametrize("rows,cols", [(2, 16), (1, 256)])
def test_the_layer_is_the_matrix_vector_product_for_every_admitted_shape(rows, cols):
    """diagonals, prepared diagonals, hybrid product, folds, bias = (M x_r + b)[i mod R] in every slot of every row; with and without bias, the
    planner's B, B = 1 (giants only) and B = 3 (a ragged last giant, a negative wrap of i - g B)"""
    p = 65537
    rng = np.random.default_rng(cols)
    todo = shapes(cols)
    assert (1, 1) in todo and (cols, cols) in todo and (1, cols) in todo and (cols, 1) in todo
    assert all(max(s) % min(s) == 0 and cols % max(s) == 0 for s in todo)
    assert len(todo) == {16: 25, 256: 81}[cols]
    for n, (R, C) in enumerate(todo):
        M = rng.integers(0, p, size=(R, C))
        x = rng.integers(0, p, size=(rows, C))
        bias = rng.integers(0, p, size=R) if n % 2 else None
        want = LM.expected_slots(M, bias, x, p, rows, cols)
        xs = LM.replicate(x, C, rows, cols)
        for baby in BABIES:
            assert list(LM.layer(M, bias, xs, p, rows, baby)) == want, (R, C, baby)


def test_the_prepared_diagonals_are_the_closed_form():
    """w_t[i] = M[i' mod R][(i' + t) mod C] with i' = ((i mod D) - g B) mod D, alike in both rows: what a thread of linear_diag_kernel computes"""
    rows, cols = 2, 16
    rng = np.random.default_rng(3)
    for R, C in shapes(cols):
        M = rng.integers(-99, 99, size=(R, C))
        D = max(R, C)
        for baby in BABIES:
            B = LM.plan(cols, R, C, baby)["B"]
            w = LM.prepared(M, rows, cols, B)
            for t in range(min(R, C)):
                for r in range(rows):
                    for i in range(cols):
                        ip = ((i % D) - (t // B) * B) % D
                        assert w[t][r * cols + i] == M[ip % R][(ip + t) % C], (R, C, baby, t, r, i)


def test_the_fold_sums_a_row():
    """y <- y + rot_a(y) over a = cols/2 .. 1 leaves the sum of a row in each of its slots; over C/2 .. R the sum of the C / R blocks"""
    rows, cols, p = 2, 16, 65537
    y = np.random.default_rng(5).integers(0, p, size=rows * cols)
    got = LM.fold(y, [8, 4, 2, 1], p, rows)
    for r in range(rows):
        assert list(got[r * cols:(r + 1) * cols]) == [int(y[r * cols:(r + 1) * cols].sum()) % p] * cols


def test_the_planner_equals_the_model():
    import fhe_si_amd as F
    for cols in (16, 256, 2048):
        for R, C in shapes(cols) if cols <= 256 else [(16, 2048), (2048, 16), (64, 1024), (512, 512), (1, 2048)]:
            for baby in (0, 1, 3, 7, 5000):
                assert F.linear_plan(cols, R, C, baby) == LM.plan(cols, R, C, baby), (cols, R, C, baby)
    pl = F.linear_plan(1024, 16, 1024)
    assert (pl["T"], pl["B"], pl["G"], pl["nfold"]) == (16, 4, 4, 6) and pl["amounts"] == [1, 2, 3, 4, 8, 12, 512, 256, 128, 64, 32, 16]
    assert len(pl["amounts"]) == 12 and sum(BM.plan(1024)) - 2 == 62                # the key switches of the layer and of the padded square
    assert F.linear_plan(16, 4, 16, 2)["amounts"] == [1, 2, 8, 4]                    # baby 1, giant 2, folds 8 and 4
    assert F.linear_plan(16, 2, 8, 1)["amounts"] == [1, 4, 2]


@pytest.mark.parametrize("cols,R,C,baby", [(16, 0, 4, 0), (16, 4, 0, 0), (16, -1, 4, 0),      # zero sizes
                                           (16, 32, 4, 0), (16, 4, 32, 0),                    # D > cols
                                           (24, 16, 4, 0), (16, 3, 12, 0),                    # D does not divide cols
                                           (24, 8, 12, 0), (24, 12, 8, 0),                    # T does not divide D
                                           (24, 4, 12, 0), (48, 2, 12, 0)])                   # C / R = 3 2^j
def test_the_planner_refuses_each_bad_shape_with_its_word(cols, R, C, baby):
    import fhe_si_amd as F
    word = LM.admitted(cols, R, C)
    assert word is not None
    with pytest.raises(F.FhesiError) as e:
        F.linear_plan(cols, R, C, baby)
    assert word in str(e.value) and "linear_plan" in str(e.value), (word, str(e.value))


def test_the_planner_refuses_a_negative_baby_step_and_a_row_out_of_range():
    import fhe_si_amd as F
    with pytest.raises(F.FhesiError, match="baby steps"):
        F.linear_plan(16, 4, 4, -1)
    for cols in (0, (1 << 20) + 1):
        with pytest.raises(F.FhesiError, match="outside"):
            F.linear_plan(cols, 1, 1)


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert hasattr(F.Context, "ct_rot_fold_dev") and hasattr(F, "linear_plan") and hasattr(F, "Linear")
    for name in ("linear", "linear_diagonals", "replicate", "fold"):
        assert hasattr(F.SlotSpace, name)
    for name in ("linear", "linear_apply"):
        assert hasattr(F.SlotBasis, name)
    for name in ("apply", "close"):
        assert hasattr(F.Linear, name)
