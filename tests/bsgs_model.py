"""Baby-step/giant-step matrix-vector products on the CPU model (tests/hoist_model.py over oracle/fhesi_pyref.py) and in slot terms (numpy).

With T = B G diagonals and t = g B + j

    sum_t d_t (*) rot_t(x)  =  sum_{g<G} rot_{gB}( sum_{j<B} rot_{-gB}(d_{gB+j}) (*) rot_j(x) )

because a rotation is a ring map: B - 1 baby rotations of x, G inner plaintext sums over diagonals rotated back in the clear, G - 1 giant rotations
of the inner sums.  `matvec_bsgs` is the right-hand side on ciphertexts, the definition of fhesi_ct_matvec_bsgs_dev.  A plain module, imported like
hoist_model."""
import numpy as np

import fhesi_pyref as R
import hoist_model as H


# ---- slot terms: a plaintext is `rows` rows of total / rows slots; a rotation by `amount` moves every row `amount` slots to the left
def rotate_values(vals, amount, rows=1):
    v = np.asarray(vals)
    shaped = v.reshape(v.shape[:-1] + (rows, v.shape[-1] // rows))
    return np.roll(shaped, -int(amount), axis=-1).reshape(v.shape)


def bsgs_diagonals(diags, B, rows=1):
    """row g B + j is diagonal g B + j rotated back by the giant step g B"""
    d = np.asarray(diags)
    return np.stack([rotate_values(d[t], -(t // B) * B, rows) for t in range(d.shape[0])])


def slot_matvec(diags, x, p, rows=1):
    """sum_t d_t o rotate(x, t) modulo p"""
    acc = np.zeros(len(x), dtype=object)
    for t, d in enumerate(diags):
        acc = (acc + np.asarray(d, dtype=object) * np.asarray(rotate_values(x, t, rows), dtype=object)) % p
    return acc


def slot_matvec_bsgs(diags, x, B, p, rows=1):
    """sum_g rotate( sum_j w_{gB+j} o rotate(x, j), g B ) modulo p with w = bsgs_diagonals(diags, B): the last group may be ragged"""
    T = len(diags)
    w = bsgs_diagonals(diags, B, rows)
    G = (T + B - 1) // B
    acc = np.zeros(len(x), dtype=object)
    for g in range(G):
        inner = np.zeros(len(x), dtype=object)
        for j in range(B):
            if g * B + j >= T:
                break
            inner = (inner + np.asarray(w[g * B + j], dtype=object) * np.asarray(rotate_values(x, j, rows), dtype=object)) % p
        acc = (acc + rotate_values(inner, g * B, rows)) % p
    return acc


# ---- the planner: the B that minimises (B - 1) + (G - 1), G = ceil(nk / B); of equal sums the larger B
def plan(nk):
    best = None
    for b in range(1, nk + 1):
        g = -(-nk // b)
        if best is None or (b + g, -b) < (best[0] + best[1], -best[0]):
            best = (b, g)
    return best


# ---- ciphertexts
def matvec_bsgs(ctx, baby, kb, giant, kg, nk, diagonals, parts):
    """Reduce( sum_g rot_kg[g]( sum_{j, gB+j<nk} rot_kb[j](c) (*) w[gB+j] ) ): hoist_model.rotation per baby and per giant, Ciphertext *= ZZX per
    term, Ciphertext += per sum.  baby[j] / giant[g]: the derived matrix of kb[j] / kg[g], or None with k = 1."""
    B, G = len(kb), len(kg)
    assert (G - 1) * B < nk <= G * B
    rots = [H.rotation(ctx, h, k, parts) for h, k in list(zip(baby, kb))[:min(B, nk)]]
    acc = None
    for g in range(G):
        inner = None
        for j in range(B):
            if g * B + j >= nk:
                break
            term = R.ct_mul_poly(ctx, rots[j], diagonals[g * B + j])
            inner = term if inner is None else R.ct_add(ctx, inner, term)
        rot = H.rotation(ctx, giant[g], kg[g], inner)
        acc = rot if acc is None else R.ct_add(ctx, acc, rot)
    return acc


def bsgs_polys(ctx, diagonals, kg, B):
    """the diagonals as message polynomials, rotated back in the clear: w[gB+j] = d_{gB+j}(X^(kg[g]^-1)) mod (Phi_m, p)"""
    return [H.automorph_message(ctx, d, pow(kg[t // B], -1, ctx.m)) for t, d in enumerate(diagonals)]
