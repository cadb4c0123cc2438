"""What the GPU tests of the baby-step/giant-step products share (test_gpu_bsgs.py): rotation keys made on the device, planted inputs, the model's
view of a downloaded matrix.  A plain module, imported like slots_common."""
import numpy as np

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
from slots_common import I, device_keys

SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def rotation_keys(ctx, logQ, ks, seed=SEED):
    """(sk1, pk0, pk1), the matrices W_k of the automorphisms ks (source key (1, s(X^k)), target s) and their derived matrices"""
    n, nd = ctx.phim, R.ndigits(logQ)
    sk1, pk0, pk1 = device_keys(ctx, logQ, seed)
    one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
    autos = [F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(k)], sk1, logQ, seed, PUB, 2000 + 100 * i) for i, k in enumerate(ks)]
    return (sk1, pk0, pk1), autos, [w.hoist(k) for w, k in zip(autos, ks)]


def extremes(logQ, nl):
    """-2^(logQ-1) and 2^(logQ-1) - 1 as limbs"""
    return O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0], O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]


def inputs(rng, count, n, nl, logQ):
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    a[0, 0, 0], a[0, 0, 1] = extremes(logQ, nl)
    return a


def pyref_matrix(rows):
    """downloaded rows [2][ncol][L][n] -> the model's matrix of DoubleCRT dictionaries"""
    return [[{i: I(col[i]) for i in range(col.shape[0])} for col in row] for row in rows]


def as_ints(ct):
    return [O.limbs_to_ints(ct[r]) for r in range(2)]


def centred(v, logQ):
    half = 1 << (logQ - 1)
    return ((v + half) % (1 << logQ)) - half
