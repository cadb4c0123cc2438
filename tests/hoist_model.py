"""The hoisted rotations on the CPU model (oracle/fhesi_pyref.py): many automorphism key switches of one ciphertext from ONE digit decomposition.

sigma_k is a ring map, so for the key-switch matrix W_k of the automorphism k (source key (1, s(X^k)), target s)

    sum_j sigma_k(D_j(c)) W_k[j]  =  sigma_k( sum_j D_j(c) W'_k[j] ),     W'_k = sigma_k^-1(W_k)   (every column, both rows)

modulo (Phi_m, 2^logQ).  `rotation` is the right-hand side, the definition of fhesi_ct_rotations_dev; `rotation_independent` is the left-hand side,
which never forms W'; `rotation_reference` is the reference's path (`>>= k`, then ApplyKeySwitch with W_k), which decomposes sigma_k(c) instead
and so gives other words for the same plaintext.  A plain module, imported like slots_model."""
import fhesi_pyref as R


def hoist_matrix(ctx, ksm, k):
    """W' = sigma_k^-1(W): DoubleCRT::automorph by k^-1 mod m on every column of both rows"""
    kinv = pow(k, -1, ctx.m)
    return [[R.dcrt_automorph(ctx, col, kinv) for col in row] for row in ksm]


def reduce_parts(ctx, parts):
    return [[R.reduce_logq(c, ctx.logQ) for c in part] for part in parts]


def rotation(ctx, hoisted, k, parts):
    """reduce_logq(ct_automorph(apply_key_switch_parts(W', c), k)); hoisted None (with k = 1) is the identity: the reduced copy"""
    sw = parts if hoisted is None else R.apply_key_switch_parts(ctx, hoisted, parts)
    return reduce_parts(ctx, R.ct_automorph(ctx, sw, k))


def rotations(ctx, hoisted, ks, cts):
    """out[t][i] = rotation(hoisted[t], ks[t], cts[i]), written as the device runs it: ByteDecomp and the forward transforms of a ciphertext
    once (what apply_key_switch_parts does first), then DotProduct, toPoly, Reduce and the automorphism per matrix"""
    out = [[None] * len(cts) for _ in ks]
    for i, parts in enumerate(cts):
        bd = [R.dcrt_from_poly(ctx, d) for d in R.byte_decomp(parts, ctx.logQ, ctx.ndigits, ctx.decomp_size)]
        for t, (h, k) in enumerate(zip(hoisted, ks)):
            sw = parts if h is None else [[R.reduce_logq(c, ctx.logQ) for c in R.dcrt_to_poly(ctx, R.dot_product(ctx, row, bd))] for row in h]
            out[t][i] = reduce_parts(ctx, R.ct_automorph(ctx, sw, k))
    return out


def rotation_independent(ctx, ksm, k, parts):
    """sum_j sigma_k(D_j(c)) W_k[j], reduced: the digits of the untouched ciphertext, moved by sigma_k in evaluation form, against W_k itself"""
    digits = R.byte_decomp(parts, ctx.logQ, ctx.ndigits, ctx.decomp_size)
    bd = [R.dcrt_automorph(ctx, R.dcrt_from_poly(ctx, d), k) for d in digits]
    return [[R.reduce_logq(c, ctx.logQ) for c in R.dcrt_to_poly(ctx, R.dot_product(ctx, row, bd))] for row in ksm]


def rotation_reference(ctx, ksm, k, parts):
    """Ciphertext >>= k, then ApplyKeySwitch with W_k (Regression::SumBatchedData's step)"""
    return R.apply_key_switch_parts(ctx, ksm, R.ct_automorph(ctx, parts, k))


def automorph_message(ctx, msg, k):
    """msg(X^k) mod (Phi_m, p): what a rotation by k decrypts to"""
    return [c % ctx.p for c in R.ct_automorph(ctx, [list(msg) + [0] * (ctx.phim - len(msg))], k)[0]]


def matvec(ctx, hoisted, ks, diagonals, parts):
    """sum_t rot_t(c) (*) w_t on the model: Ciphertext *= ZZX per term, Ciphertext += per sum (what fhesi_ct_plain_sum_dev computes)"""
    acc = None
    for h, k, w in zip(hoisted, ks, diagonals):
        term = R.ct_mul_poly(ctx, rotation(ctx, h, k, parts), w)
        acc = term if acc is None else R.ct_add(ctx, acc, term)
    return acc
