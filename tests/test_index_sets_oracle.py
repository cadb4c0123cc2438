"""CPU: the C oracle's calls over a proper index set against the Python big-integer model (oracle/fhesi_pyref.py), on the chain and the sets
test_gpu_index_sets.py checks the device with.  test_oracle_golden.py compares toPoly over {0, L - 1} and the modulus switching from the full
set (scaleDownToSet) or from [0], [0, 1], [1] (addPrimesAndScale) on chains of 60-bit primes; here the current set is a proper one without a
prefix, on a Bluestein ring (m = 45) and a power-of-two one (m = 16), with a 20-bit prime in the chain."""
import math

import numpy as np
import pytest

import fhesi_pyref as R
import index_sets_common as X
import oracle_lib as O

P_MOD = 23


def ints(row):
    return [int(v) for v in row]


@pytest.mark.parametrize("m", [45, 16])
def test_c_oracle_equals_python_model_over_proper_index_sets(m):
    primes, roots, _ = X.mixed_chain(m)
    ctx = R.Ctx(m, 100, P_MOD, primes, roots)
    orc = O.Oracle(m, primes, roots)
    n = orc.phim
    for S in list(X.SETS) + [X.FULL]:
        PS = X.product(primes, S)
        comp = [i for i in X.FULL if i not in S]
        W = len(S) + 2
        poly = X.centred_poly(n, PS, 1000 * m + sum(1 << i for i in S))
        limbs = X.to_limbs(poly, W)
        assert np.array_equal(limbs, O.ints_to_limbs(poly, W)) and X.to_ints(limbs) == O.limbs_to_ints(limbs) == poly
        rows = orc.dcrt_from_poly(limbs)
        model = R.dcrt_from_poly(ctx, poly)
        assert [ints(r) for r in rows] == [model[i] for i in X.FULL], S
        sub = {i: model[i] for i in S}
        # toPoly over the set: the polynomial itself, and its non-negative form
        assert X.to_ints(orc.dcrt_to_poly(rows, W, idx=S)) == R.dcrt_to_poly(ctx, model, idxset=S) == poly, S
        pos = X.to_ints(orc.dcrt_to_poly(rows, W, idx=S, positive=True))
        assert pos == R.dcrt_to_poly(ctx, model, idxset=S, positive=True) == [c % PS for c in poly], S
        if len(S) >= 2:
            for keep in (S[1:], S[-1:]):
                want = R.dcrt_scale_down_to_set(ctx, sub, keep)
                got = orc.dcrt_scale_down_to_set(rows, S, keep, P_MOD)
                for i in keep:
                    assert ints(got[i]) == want[i], (S, keep, i)
        if comp:
            want = R.dcrt_add_primes_and_scale(ctx, sub, comp)
            got, lf = orc.dcrt_add_primes_and_scale(rows, S, comp, P_MOD)
            for i in X.FULL:
                assert ints(got[i]) == want[i], (S, i)
            F = X.product(primes, comp)
            wlf = math.log(F * pow(F % P_MOD, -1, P_MOD))                # the logarithm of the factor (DoubleCRT.cpp:180-182)
            assert abs(lf - wlf) < 1e-9 * wlf, (S, lf, wlf)
