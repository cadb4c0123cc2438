"""GPU: prepared plaintext operands over a slot basis -- signed integer data and weights whose exact sum of products exceeds every single prime."""
import numpy as np
import pytest

import fhe_si_amd as F
import params as P
from slots_common import I, View, device_keys

pytestmark = pytest.mark.gpu


def test_integer_model_on_encrypted_data_over_three_primes():
    """y = sum_t a_t o w_t + c on m = 64 with three primes just below 2^31: |y| near 2^81, far above any prime and inside (-P/2, P/2), P > 2^91.
    logQ = 160: a product adds about n p^2 = 2^67 of noise per term against the rounding limit 2^(logQ - 32)."""
    m, g, logQ = 64, 5, 160
    primes = F.slots_basis_plan(m, 90, 31, g)["primes"]
    assert len(primes) == 3 and all((1 << 30) < q < (1 << 31) for q in primes)
    chain, roots = P.chain_for(m, logQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k, nl = B.total, B.k, (logQ + 63) // 64
    words = 2 * n * nl
    sk1, pk0, pk1 = device_keys(ctx, logQ, 31)
    rng = np.random.default_rng(64)
    G, T, NW = 2, 3, 4
    a = rng.integers(-(1 << 40), 1 << 40, size=(G * T, n)).astype(np.int64)
    w = rng.integers(-(1 << 39), 1 << 39, size=(NW, n)).astype(np.int64)
    c = rng.integers(-(1 << 62), 1 << 62, size=(G, n)).astype(np.int64)
    a_idx, seg = list(range(G * T)), [0, T, 2 * T]
    b_idx = [0, 1, 2, 3, 3, 1]
    exact = [[sum(int(a[t, j]) * int(w[b_idx[t], j]) for t in range(seg[gi], seg[gi + 1])) + int(c[gi, j]) for j in range(n)] for gi in range(G)]
    big = max(abs(v) for row in exact for v in row)
    assert big > max(primes) << 40 and big < B.modulus // 2

    enc = ctx.alloc(k * G * T * words * 8)
    B.encrypt_batch_seeded(pk0, pk1, logQ, 5150, 0, a, enc, nl)
    plains = B.plain(w)
    assert [pl.p for pl in plains] == primes and all(pl.nw == NW and pl.maxabs == q - 1 for pl, q in zip(plains, primes))
    out = ctx.alloc(k * G * words * 8)
    B.ct_plain_sum_dev(plains, logQ, enc, G * T, nl, a_idx, b_idx, seg, out)
    B.ct_add_slots_dev(logQ, out, nl, G, c)
    got = B.decrypt_batch(sk1, logQ, out, nl, G)
    for gi in range(G):
        assert I(got[gi]) == exact[gi], gi

    # every channel is the single-space call on that channel's part of the layout, bit for bit
    all_out = out.download((k, G, words))
    one = ctx.alloc(G * words * 8)
    for ch in range(k):
        space = B.channel(ch)
        pl = space.plain(np.mod(w, primes[ch]))
        ctx.ct_plain_sum_dev(pl, logQ, View(enc, ch * G * T * words * 8), G * T, nl, a_idx, b_idx, seg, one)
        space.ct_add_slots_dev(logQ, one, 2, nl, G, np.mod(c, primes[ch]))
        assert np.array_equal(one.download((G, words)), all_out[ch]), ch
        pl.close()
    # one constant for every group
    B.ct_add_slots_dev(logQ, out, nl, G, c[:1])
    got = B.decrypt_batch(sk1, logQ, out, nl, G)
    for gi in range(G):
        assert I(got[gi]) == [x + int(y) for x, y in zip(exact[gi], c[0])], gi
    for pl in plains:
        pl.close()
