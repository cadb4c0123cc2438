"""Dense linear layers on packed slots in slot terms (numpy / Python ints): the model of fhesi_linear_* and fhesi_ct_rot_fold_dev.

The space has `rows` rows of `cols` slots; rot_t moves every row t slots to the left.  The layer is R x C, D = max(R, C), T = min(R, C); admitted:
T | D, D | cols, and for R < C the ratio C / R a power of two.

    input      slot (r, i) = x_r[i mod C]
    diagonals  e_t[i] = M[(i mod D) mod R][((i mod D) + t) mod C]          t < T, alike in every row
    prepared   w_t = rot_{-gB}(e_t),  t = g B + j, j < B
    product    y = sum_g rot_{gB}( sum_j w_{gB+j} o rot_j(x) )             (bsgs_model.slot_matvec_bsgs)
    folds      R < C only: for a = C/2, C/4, .., R:  y <- y + rot_a(y)
    bias       y <- y + (b[i mod R])
    result     slot (r, i) = (M x_r + b)[i mod R]

A plain module, imported like bsgs_model."""
import numpy as np

import bsgs_model as BM


def admitted(cols, R, C):
    """None, or the word of the condition the shape breaks (the order fhesi_linear_plan checks them in)"""
    if R < 1 or C < 1:
        return "at least 1"
    D, T = max(R, C), min(R, C)
    if D > cols:
        return "exceeds the row"
    if cols % D:
        return "does not divide the row"
    if D % T:
        return "does not divide max"
    if R < C and (C // R) & (C // R - 1):
        return "not a power of two"
    return None


def plan(cols, R, C, baby=0):
    """T, B, G, nfold and the amounts: babies 1 .. B-1, giants B .. (G-1)B, folds C/2 .. R -- an amount two lists share appears once per use"""
    assert admitted(cols, R, C) is None
    T = min(R, C)
    B = BM.plan(T)[0] if baby == 0 else min(baby, T)
    G = -(-T // B)
    folds = []
    a = C // 2
    while R < C and a >= R:
        folds.append(a)
        a //= 2
    return {"T": T, "B": B, "G": G, "nfold": len(folds), "amounts": list(range(1, B)) + [g * B for g in range(1, G)] + folds}


def replicate(x, C, rows, cols):
    """x [rows][C] -> [rows * cols] slot values, row r holding x_r with period C"""
    x = np.asarray(x).reshape(rows, C)
    return np.tile(x, cols // C).reshape(-1)


def diagonals(M, rows, cols):
    """e_t, t < T: [T][rows * cols], entries as they are in M (object arrays pass through)"""
    M = np.asarray(M)
    R, C = M.shape
    D, T = max(R, C), min(R, C)
    i = np.arange(cols) % D
    return np.stack([np.tile(M[i % R, (i + t) % C], rows) for t in range(T)])


def prepared(M, rows, cols, B):
    """w_t = rot_{-gB}(e_t): what fhesi_linear_diagonals returns before the reduction modulo p"""
    return BM.bsgs_diagonals(diagonals(M, rows, cols), B, rows)


def fold(y, amounts, p, rows):
    for a in amounts:
        y = (np.asarray(y, dtype=object) + np.asarray(BM.rotate_values(y, a, rows), dtype=object)) % p
    return y


def layer(M, bias, x_slots, p, rows, baby=0):
    """the hybrid product on slot values [rows * cols]: baby-step/giant-step product, folds, bias -- modulo p"""
    M = np.asarray(M)
    R, C = M.shape
    cols = len(x_slots) // rows
    pl = plan(cols, R, C, baby)
    w = np.asarray(prepared(M, rows, cols, pl["B"]), dtype=object) % p
    # slot_matvec_bsgs rotates the diagonals back itself: give it the diagonals, check that they are the prepared ones
    e = np.asarray(diagonals(M, rows, cols), dtype=object) % p
    assert np.array_equal(BM.bsgs_diagonals(e, pl["B"], rows), w)
    y = BM.slot_matvec_bsgs(e, x_slots, pl["B"], p, rows)
    y = fold(y, pl["amounts"][pl["B"] - 1 + pl["G"] - 1:], p, rows)
    if bias is not None:
        b = np.asarray(bias, dtype=object)
        y = (y + np.tile(b[np.arange(cols) % R], rows)) % p
    return y


def brute(M, bias, x, p):
    """(M x_r + b) mod p per row r: x [rows][C] -> [rows][R] Python ints"""
    M = np.asarray(M, dtype=object)
    out = []
    for xr in np.asarray(x, dtype=object):
        y = M.dot(xr)
        if bias is not None:
            y = y + np.asarray(bias, dtype=object)
        out.append([int(v) % p for v in y])
    return out


def expected_slots(M, bias, x, p, rows, cols):
    """slot (r, i) = (M x_r + b)[i mod R]"""
    R = np.asarray(M).shape[0]
    y = brute(M, bias, x, p)
    return [y[r][i % R] for r in range(rows) for i in range(cols)]
