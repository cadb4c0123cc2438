"""Dense layers larger than a row of slots in slot terms (numpy / Python ints): the model of fhesi_linear_grid_* and fhesi_ct_linear_grid_dev, built on
linear_model and bsgs_model.

The matrix is R x C = (nI Rb) x (nJ Cb), a grid of blocks of a shape linear_model admits; T = min(Rb, Cb), D = max(Rb, Cb).

    input      nJ plaintexts, plaintext J: slot (r, i) = x_r[J Cb + (i mod Cb)]
    diagonals  of block (I, J): linear_model.prepared(M[I Rb .., J Cb ..]) with the GRID's B
    output     y_I = fold( sum_g rot_{gB}( sum_J sum_j w^{IJ}_{gB+j} o rot_j(x_J) ) ) + b_I
    result     slot (r, i) of y_I = (M x_r + b)[I Rb + (i mod Rb)]

Rotations are ring maps and the plaintext sums are exact: the babies of input block J serve every output block, the giants and folds of output block I
run behind the sum over J -- nJ (B - 1) + nI (G - 1) + nI nfold key switches against nI nJ (B + G - 2 + nfold) for one layer per block.  A plain
module, imported like linear_model."""
import numpy as np

import bsgs_model as BM
import linear_model as LM


def refused(cols, R, C, Rb, Cb):
    """None, or the word of the condition the grid breaks (the order fhesi_linear_grid_plan checks them in)"""
    word = LM.admitted(cols, Rb, Cb)
    if word is not None:
        return word
    if R < 1 or C < 1:
        return "at least 1"
    if R % Rb or C % Cb:
        return "not a multiple"
    if (R // Rb) * (C // Cb) * min(Rb, Cb) > 65535:
        return "per handle"
    return None


def cost(nI, nJ, T, B):
    """key switches of the shared baby and giant steps"""
    return nJ * (B - 1) + nI * (-(-T // B) - 1)


def plan(cols, R, C, Rb, Cb, baby=0):
    """the block's plan with the B of the shared schedule: the B in 1 .. T of least cost, of equal costs the larger"""
    assert refused(cols, R, C, Rb, Cb) is None
    nI, nJ, T = R // Rb, C // Cb, min(Rb, Cb)
    B = min(baby, T) if baby else min(range(1, T + 1), key=lambda b: (cost(nI, nJ, T, b), -b))
    pl = LM.plan(cols, Rb, Cb, B)
    assert pl["B"] == B
    return {"nI": nI, "nJ": nJ, "T": T, "B": B, "G": pl["G"], "nfold": pl["nfold"], "amounts": pl["amounts"],
            "key_switches": cost(nI, nJ, T, B) + nI * pl["nfold"]}


def per_block_key_switches(cols, R, C, Rb, Cb, baby=0):
    """one linear_model.plan per block, each with its own babies, giants and folds"""
    return (R // Rb) * (C // Cb) * len(LM.plan(cols, Rb, Cb, baby)["amounts"])


def replicate_blocks(x, Cb, rows, cols):
    """x [rows][C] -> [nJ][rows * cols]: plaintext J holds x_r[J Cb .. (J + 1) Cb) with period Cb in row r"""
    x = np.asarray(x)
    x = x.reshape(rows, x.shape[-1])
    return np.stack([LM.replicate(x[:, J * Cb:(J + 1) * Cb], Cb, rows, cols) for J in range(x.shape[1] // Cb)])


def prepared(M, Rb, Cb, rows, cols, B):
    """[nI][nJ][T][rows * cols]: the prepared diagonals of every block, entries as they are in M"""
    M = np.asarray(M)
    nI, nJ = M.shape[0] // Rb, M.shape[1] // Cb
    return np.stack([np.stack([LM.prepared(M[I * Rb:(I + 1) * Rb, J * Cb:(J + 1) * Cb], rows, cols, B) for J in range(nJ)]) for I in range(nI)])


def grid(M, bias, xs, Rb, Cb, p, rows, baby=0):
    """the shared schedule on slot values xs [nJ][rows * cols] -> [nI][rows * cols], modulo p"""
    M = np.asarray(M)
    R, C = M.shape
    cols = len(xs[0]) // rows
    pl = plan(cols, R, C, Rb, Cb, baby)
    nI, nJ, T, B, G = pl["nI"], pl["nJ"], pl["T"], pl["B"], pl["G"]
    w = np.asarray(prepared(M, Rb, Cb, rows, cols, B), dtype=object) % p
    babies = [[np.asarray(BM.rotate_values(xs[J], j, rows), dtype=object) for j in range(min(B, T))] for J in range(nJ)]      # once per input block
    out = []
    for I in range(nI):
        acc = np.zeros(rows * cols, dtype=object)
        for g in range(G):
            inner = np.zeros(rows * cols, dtype=object)
            for J in range(nJ):
                for j in range(B):
                    if g * B + j < T:
                        inner = (inner + w[I][J][g * B + j] * babies[J][j]) % p
            acc = (acc + BM.rotate_values(inner, g * B, rows)) % p                  # once per output block
        y = LM.fold(acc, pl["amounts"][B - 1 + G - 1:], p, rows)
        if bias is not None:
            b = np.asarray(bias, dtype=object)[I * Rb:(I + 1) * Rb]
            y = (y + np.tile(b[np.arange(cols) % Rb], rows)) % p
        out.append(y)
    return out


def expected_slots(M, bias, x, Rb, p, rows, cols):
    """[nI][rows * cols]: slot (r, i) of block I = (M x_r + b)[I Rb + (i mod Rb)]"""
    y = LM.brute(M, bias, x, p)
    return [[y[r][I * Rb + i % Rb] for r in range(rows) for i in range(cols)] for I in range(np.asarray(M).shape[0] // Rb)]
