"""What the GPU slot tests share (test_gpu_slots.py, test_gpu_slots_pow2.py, test_gpu_slots_basis.py): contexts, random public keys, keys made
on the device, views into a device buffer.  A plain module, imported like slots_model."""
import numpy as np

import fhe_si_amd as F
import oracle_lib as O
import params as P


def I(v):
    return [int(x) for x in v]


def context(m, logQ=64, p=65537):
    primes, roots = P.chain_for(m, logQ, p)
    return F.Context(m, primes, roots), primes


def make(space, model, m, p, g, logQ=64):
    """context, the device space space(ctx, p, g) and its model"""
    ctx, _ = context(m, logQ, p)
    return ctx, space(ctx, p, g), model.slot_space(m, p, g)


def rand_pk(ctx, primes, rng):
    rows = P.rand_rows(rng, primes, ctx.phim, 2)
    out = []
    for r in range(2):
        d = F.DoubleCRT(ctx)
        for i in range(rows.shape[1]):
            d.set_row(i, np.ascontiguousarray(rows[r, i]))
        out.append(d)
    return out


class View:
    """part of a device buffer, for the calls that take one channel of a logical ciphertext"""

    def __init__(self, buf, off):
        self.ptr = F.binding._vp(buf.ptr.value + off)


def device_keys(ctx, logQ, seed):
    """t = sampleHWt(64), pk = (e + t c1, -c1), all on the device"""
    n, nl = ctx.phim, (logQ + 63) // 64
    sk1 = F.DoubleCRT(ctx).sample(0, 64, seed, 7)
    c1 = F.DoubleCRT.from_poly(ctx, P.rand_limbs(np.random.default_rng(seed), (n,), nl, logQ))
    pk0 = sk1.copy().op(c1, F.OP_MUL).op(F.DoubleCRT(ctx).sample(1, 0, seed, 9), F.OP_ADD)
    pk1 = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([0] * n, 1)).op(c1, F.OP_SUB)
    return sk1, pk0, pk1
