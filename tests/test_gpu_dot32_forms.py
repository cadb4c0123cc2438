"""The digit-tile dot products (dot32_kernel2, dot32_kernel2p) at the smallest ring of the 30-bit path, m = 2^15, n = 2^14: one case per
way through the column sweep the two kernels share (dot32_sweep: 8-column pairs in rotated order, a 4-column chunk, a tail of up to 3
columns), through the tile loader taken in parts, and through the limb loop.  Every case multiplies a ragged batch of 9 ciphertexts -- one
full tile of 8 and a tile with a single ciphertext, so the loader's and the epilogue's ciphertext bounds both cut -- with option
dot32_k4 = 0, names the kernel that ran, and compares ciphertexts 0, 7 and 8 bit for bit with the oracle.  One more case runs the 5-pair
sweep on 57 ciphertexts = 8 tiles, because the rotation starts at tile & 7: only tiles 5 .. 7 start past the last pair and fold back."""
import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
from test_gpu_configs import ctx_kernel_name

pytestmark = pytest.mark.gpu

M, PT = 1 << 15, 65537

# ciphertexts (and those compared with the oracle), logQ, columns = 3 ceil(logQ / 24), generated matrix (centred limbs, at most 16) or uploaded uniform rows, kernel, limb-count condition
CASES = [
    pytest.param(9, (0, 7, 8), 256, 33, False, "dot32_kernel2<8, 8>", None, id="tail_only_33"),                      # 4 pairs + 1
    pytest.param(9, (0, 7, 8), 288, 36, False, "dot32_kernel2<8, 8>", "odd", id="chunk_no_tail_36"),                 # 4 pairs + 4; a half wave without a limb
    pytest.param(9, (0, 7, 8), 360, 45, False, "dot32_kernel2<8, 8>", "odd", id="chunk_and_tail_5_pairs_45"),        # 5 pairs + 4 + 1: the rotation wraps at a non-power-of-two
    pytest.param(9, (0, 7, 8), 384, 48, False, "dot32_kernel2<8, 8>", None, id="six_pairs_48"),                      # neither chunk nor tail
    pytest.param(9, (0, 7, 8), 768, 96, True, "dot32_kernel2p", "odd", id="two_parts_of_48"),                        # ncp = ((96 + 1) / 2 + 7) & ~7 = 48; 11 limbs
    pytest.param(9, (0, 7, 8), 840, 105, True, "dot32_kernel2p", None, id="parts_of_56_and_49"),                     # ncp = 56; the second part: 6 pairs + 1
    pytest.param(9, (0, 7, 8), 1024, 129, False, "dot32_kernel2<4, 8>", "over16", id="limb_loop_twice_129"),         # more than 16 limbs on 16 half waves
    # tiles 0 .. 7 of 5 pairs: starts 0 .. 4, then 5, 6, 7 -> 0, 1, 2; ciphertext 47 is in tile 5, 56 alone in tile 7
    pytest.param(57, (0, 8, 47, 56), 360, 45, False, "dot32_kernel2<8, 8>", "odd", id="rotation_start_folds_back_57"),
]


@pytest.mark.parametrize("count, checked, logQ, ncol, generated, kernel, limbs", CASES)
def test_digit_tile_form(count, checked, logQ, ncol, generated, kernel, limbs):
    primes, roots = P.chain_for(M, logQ, PT)
    ctx = F.Context(M, primes, roots)
    orc = O.Oracle(M, primes, roots)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    assert n == 1 << 14 and 3 * nd == ncol
    rng = np.random.default_rng(logQ)
    if generated:
        one = np.zeros((n, 1), dtype=np.uint64)
        one[0, 0] = 1
        t = F.DoubleCRT(ctx).sample(0, 64, 7 * logQ, 1)
        t2 = t.copy()
        t2.op(t, 2)
        ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([F.DoubleCRT.from_poly(ctx, one), t, t2], t, logQ, 7 * logQ, 11 * logQ, 5000, 3)
        ksm = ksk.download()
    else:
        ksm = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)])
        ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    assert ctx.get_option("dot32_k4") == 1 and ctx.get_option("batch_chunk") == 0
    ctx.set_option("dot32_k4", 0)
    ctx.set_option("batch_chunk", 64)                # the whole batch in one launch of the dot product: tiles 0 .. (count - 1) / 8
    try:
        got = ctx.ct_mul_relin(ksk, logQ, PT, a, b)
        form, rows, _ = ksk.form()
        name = ctx_kernel_name(ctx, ksk, logQ, PT, a, b, nl)
    finally:
        ctx.set_option("dot32_k4", 1)
        ctx.set_option("batch_chunk", 0)
    print(f"count={count} logQ={logQ} ncol={ncol} form={form} limbs={rows} kernel={name}")
    assert form == 1 and kernel in name, (form, rows, name)
    if generated:
        assert rows <= 16 and ksk.key_bits()[0], (rows, ksk.key_bits())
    if limbs == "odd":
        assert rows % 2 == 1, rows                   # the upper half of the last wave has no limb
    if limbs == "over16":
        assert rows > 16, rows                       # the waves go round the limb loop twice
    for c in checked:
        assert np.array_equal(got[c], orc.ct_mul_relin(ksm, a[c], b[c], logQ, PT)), c
