"""GPU: convolution layers on packed slots (fhesi_conv2d_*, fhesi_ct_conv2d_dev) through the C ABI -- the masked weight plaintexts conv_lattice_mask_kernel
writes with the unit geometry against the model of tests/conv_model.py without any key, the call word for word against the composition of existing entry points it is defined as,
through the scheme, inside a small network, over a slot basis, and the refusals.  Exact throughout."""
import ctypes
import functools

import numpy as np
import pytest

import conv_model as CM
import fhe_si_amd as F
import fhesi_pyref as R
import linear_grid_model as GM
import params as P
from bsgs_common import inputs, rotation_keys
from slots_common import I, View, context, device_keys
from test_gpu_linear import DevTensor, planted

pytestmark = pytest.mark.gpu
LOGQ, NL = 128, 2
RINGS = {4096: (65537, 3),                 # the two largest chain primes, limbs
         1 << 15: (65537, 3)}              # four 30-bit primes on rows of 2^14
# (kh, kw, anchor) on the 2 x 4 plane: every offset of these kernels is one of +-1, +-3, +-4, +-5
KERNELS = [(3, 3, (1, 1)), (1, 3, (0, 1)), (3, 1, (1, 0)), (2, 2, (0, 0))]
PLANE = (2, 4)


def shape_of(S):
    rows = max(S.rows, 1)
    return rows, S.total // rows


def kernel(rng, p, Cout, Cin, kh, kw):
    return planted(rng, p, Cout * Cin, kh * kw).reshape(Cout, Cin, kh, kw)


# ------------------------------------------------------------------------------------------------ the masks, no keys
def check_masks(S, cases, seed, channels=((1, 1), (2, 3))):
    rng = np.random.default_rng(seed)
    rows, cols = shape_of(S)
    ran = 0
    for (H, W), (kh, kw, anchor) in cases:
        for Cin, Cout in channels:
            if CM.refused(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1]) is not None:
                continue
            K = kernel(rng, S.p, Cout, Cin, kh, kw)
            if K.size >= 7:
                assert (K < 0).any() and (K == 0).any() and (K == S.p).any() and (abs(K) == 1 << 62).any()
            for form in (CM.FLAT, CM.SPLIT):
                want = CM.prepared(K, H, W, anchor, rows, cols, form) % S.p
                got = S.conv2d_masks(K, (H, W), anchor, form)
                assert got.shape == (Cout, Cin, kh * kw, S.total) and np.array_equal(got.astype(object), want), ((H, W), (kh, kw), anchor, Cin, Cout, form)
            ran += 1
    return ran


def composition(ctx, S, mats, K, bias, image, anchor, form, src, count, logQ=LOGQ, nl=NL):
    """flat: fhesi_ct_rotations_dev per input channel over the amounts into one pool, ONE fhesi_ct_plain_sum_dev with the groups (I, i) and the terms (J, t)
    over the plaintext SlotSpace.plain makes of the model's masked weights, fhesi_ct_add_slots_dev with b[I]; split: the rotations over the baby amounts,
    ONE plaintext sum with the groups (I, dy, i) and the terms (J, dx), per output channel fhesi_ct_rotations_dev (nk = 1) of each inner sum by its giant,
    the first into out, the others added with fhesi_ct_add_dev, then the bias -> [Cout][count][2][n][nl]"""
    Cout, Cin, kh, kw = K.shape
    rows, cols = shape_of(S)
    pl = CM.plan(cols, image[0], image[1], Cin, Cout, kh, kw, anchor[0], anchor[1], form)
    w = (CM.prepared(K, image[0], image[1], anchor, rows, cols, pl["form"]) % S.p).astype(np.int64).reshape(Cout * Cin * kh * kw, S.total)
    plain = S.plain(w, False)
    B, G = (kh * kw, 1) if pl["form"] == CM.FLAT else (kw, kh)
    kb, kg = pl["amounts"][:B], pl["amounts"][B:]
    ctb = 2 * ctx.phim * nl * 8
    pool = ctx.alloc(Cin * B * count * ctb)
    for J in range(Cin):
        ctx.ct_rotations_dev([mats[a] if a else None for a in kb], [S.rotation_k(a) for a in kb], logQ, View(src, J * count * ctb), nl, count,
                             View(pool, J * B * count * ctb), nl)
    a_idx, b_idx, seg = CM.sum_lists(Cout, Cin, kh * kw, B, G, count)
    inner = ctx.alloc(Cout * G * count * ctb)
    ctx.ct_plain_sum_dev(plain, logQ, pool, Cin * B * count, nl, a_idx, b_idx, seg, inner)
    out = inner
    if pl["form"] == CM.SPLIT:
        out, rot = ctx.alloc(Cout * count * ctb), ctx.alloc(count * ctb)
        for Ic in range(Cout):
            y = View(out, Ic * count * ctb)
            for g in range(G):
                ctx.ct_rotations_dev([mats[kg[g]] if kg[g] else None], [S.rotation_k(kg[g])], logQ, View(inner, (Ic * G + g) * count * ctb), nl, count, rot if g else y, nl)
                if g:
                    ctx.ct_add_dev(logQ, y, rot, 2, nl, count)
    if bias is not None:
        for Ic in range(Cout):
            S.ct_add_slots_dev(logQ, View(out, Ic * count * ctb), 2, nl, count, np.full((1, S.total), int(bias[Ic]) % S.p, dtype=np.int64), only_usable=False)
    plain.close()
    return out.download((Cout, count, 2, ctx.phim, nl))


def test_masks_equal_the_model_on_a_two_row_ring():
    """m = 64, p = 257, g = 3: two rows of 16.  4 x 4 fills the row (P = cols: the wrap of i - u W in the split form crosses the row's end), the others hold
    several images per row, 1 x 16 and 16 x 1 have one line, 1 x 1 one pixel; every anchor the kernel holds; 3 x 5 on 4 x 4 has the widest offsets.
    Then a stage of at least two chunks, and the host and the device constructor through layers that take no matrix."""
    big, _ = context(64, LOGQ, 257)
    SB = F.SlotSpace.pow2(big, 257, 3)
    assert (SB.rows, SB.cols, SB.total) == (2, 16, 32)
    kernels = [(1, 1, (0, 0)), (3, 3, (0, 0)), (3, 3, (1, 1)), (1, 3, (0, 0)), (1, 3, (0, 1)), (3, 1, (0, 0)), (3, 1, (1, 0)), (2, 2, (0, 0)), (2, 2, (1, 1))]
    cases = [(plane, k) for plane in [(4, 4), (2, 4), (4, 2), (1, 16), (16, 1), (2, 2), (1, 1)] for k in kernels] + [((4, 4), (3, 5, (1, 2)))]
    ran = check_masks(SB, cases, 64)
    assert ran >= 2 * 30
    # six channel pairs of nine plaintexts in chunks of two pairs: the same masks, chunk by chunk
    K = kernel(np.random.default_rng(9), 257, 3, 2, 3, 3)
    whole = [SB.conv2d_masks(K, (4, 4), (1, 1), form) for form in (1, 2)]
    big.set_option("stage_chunk_bytes", 2 * 9 * 32 * 8 + 100)
    try:
        assert all(np.array_equal(SB.conv2d_masks(K, (4, 4), (1, 1), form), whole[form - 1]) for form in (1, 2))
        assert np.array_equal(whole[0].astype(object), CM.prepared(K, 4, 4, (1, 1), 2, 16, 1) % 257)
        chunked = True
        run_without_a_matrix(big, SB, chunked)
    finally:
        big.set_option("stage_chunk_bytes", 0)
    run_without_a_matrix(big, SB, False)


def run_without_a_matrix(big, SB, chunked):
    """1 x 1 kernels take no matrix: out[I] = sum_J K[I][J] in[J] + b[I] -- Cin = Cout = 1, and 2 -> 3 channels (six pairs: three chunks of two where the
    stage is capped); the host and the device constructor give equal handles, equal to the composition"""
    n, count = big.phim, 2
    for Cin, Cout in ((1, 1), (2, 3)):
        if chunked:
            big.set_option("stage_chunk_bytes", 2 * 32 * 8 + 100)
        rng = np.random.default_rng(Cin)
        K, b = kernel(rng, 257, Cout, Cin, 1, 1), np.array([300, -1, 1 << 62][:Cout], dtype=np.int64)
        src = big.upload(np.concatenate([inputs(np.random.default_rng(J + 1), count, n, NL, LOGQ) for J in range(Cin)]))
        outs = []
        for cv in (SB.conv2d(K, b, (2, 4)), SB.conv2d(DevTensor(big, K), DevTensor(big, b), (2, 4), device=True)):
            assert (cv.shape, cv.image, cv.anchor, cv.form, cv.nh, cv.amounts, cv.key_switches, cv.terms, cv.has_bias) == \
                ((Cout, Cin, 1, 1), (2, 4), (0, 0), 1, 1, [0], 0, Cin, True)
            out = big.alloc(Cout * count * 2 * n * NL * 8)
            cv.apply([None], LOGQ, src, NL, count, out)
            outs.append(out.download((Cout, count, 2, n, NL)))
            cv.close()
        assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(outs[0], composition(big, SB, {}, K, b, (2, 4), (0, 0), 1, src, count))


def test_masks_equal_the_model_on_a_single_row_ring():
    """m = 257 (prime), p = 1543, g = 3 of order 256: one row of 256 slots through the chirp embedding's space -- 16 x 16 fills it, 8 x 8 holds four images"""
    ctx, _ = context(257, 64, 1543)
    S = F.SlotSpace(ctx, 1543, 3)
    assert shape_of(S) == (1, 256)
    assert check_masks(S, [((16, 16), (3, 3, (1, 1))), ((8, 8), (3, 3, (1, 1))), ((8, 8), (2, 2, (0, 0)))], 257) == 6


# ------------------------------------------------------------------------------------------------ the call against its definition
def amounts_of(cols, plane, kernels):
    out = set()
    for kh, kw, anchor in kernels:
        for form in (1, 2):
            out |= set(CM.plan(cols, plane[0], plane[1], 1, 1, kh, kw, anchor[0], anchor[1], form)["amounts"])
    return sorted(out - {0})


@functools.lru_cache(maxsize=None)
def ring(m):
    """one context, its two-row space, keys made on the device and the hoisted matrices by amount: the offsets of KERNELS on the 2 x 4 plane; m = 4096 also
    carries those of a 3 x 3 kernel on the 4 x 8 plane"""
    p, g = RINGS[m]
    primes, roots = P.chain_for(m, LOGQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    amounts = amounts_of(S.cols, PLANE, KERNELS)
    assert amounts == sorted([1, 3, 4, 5] + [S.cols - a for a in (1, 3, 4, 5)])
    if m == 4096:
        amounts = sorted(set(amounts) | set(amounts_of(S.cols, (4, 8), [(3, 3, (1, 1))])))
    keys, autos, hoisted = rotation_keys(ctx, LOGQ, [S.rotation_k(a) for a in amounts])
    return ctx, S, keys, dict(zip(amounts, hoisted))


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_conv_equals_the_composition_of_existing_calls(m):
    """plane 2 x 4 (128 / 2048 images per row): 3 x 3 centred, one line either way, 2 x 2 anchored at its corner; 2 -> 3 channels and one; both forms and
    the planner's; counts 1 and 3; with and without bias; the host and the device constructor; then the flat form of 2 -> 3 channels in chunks of one
    ciphertext, where a chunk's sums are not where the result goes"""
    ctx, S, _, mats = ring(m)
    n, top = ctx.phim, 3
    rng = np.random.default_rng(m + 2)
    for kh, kw, anchor in KERNELS:
        for Cin, Cout in ((2, 3), (1, 1)):
            a = np.stack([inputs(rng, top, n, NL, LOGQ) for _ in range(Cin)])                 # [Cin][top]
            src = ctx.upload(a)
            K = rng.integers(-S.p, 2 * S.p, size=(Cout, Cin, kh, kw)).astype(np.int64)
            for bias in (None, rng.integers(-S.p, 2 * S.p, size=Cout).astype(np.int64)):
                want = {form: composition(ctx, S, mats, K, bias, PLANE, anchor, form, src, top) for form in (1, 2)}
                for form in (0, 1, 2):
                    pl = CM.plan(S.cols, PLANE[0], PLANE[1], Cin, Cout, kh, kw, anchor[0], anchor[1], form)
                    made = [(S.conv2d(K, bias, PLANE, anchor, form), (1, top))]
                    if form == 0:
                        made.append((S.conv2d(DevTensor(ctx, K), None if bias is None else DevTensor(ctx, bias), PLANE, anchor, form, device=True), (top,)))
                    for cv, counts in made:
                        assert (cv.form, cv.nh, cv.amounts, cv.key_switches, cv.terms) == (pl["form"], pl["nh"], pl["amounts"], pl["key_switches"], pl["terms"])
                        assert cv.has_bias == (bias is not None)
                        for count in counts:
                            out = ctx.alloc(Cout * count * 2 * n * NL * 8)
                            cv.apply(mats, LOGQ, ctx.upload(a[:, :count]), NL, count, out)
                            assert np.array_equal(out.download((Cout, count, 2, n, NL)), want[pl["form"]][:, :count]), ((kh, kw), Cin, Cout, form, bias is not None, count)
                        cv.close()
            if (kh, kw, Cin) == (3, 3, 2):
                # 18 rotated ciphertexts per item: one item per chunk
                cv = S.conv2d(K, bias, PLANE, anchor, 1)
                out = ctx.alloc(Cout * top * 2 * n * NL * 8)
                ctx.set_option("wave_operands", 18)
                try:
                    cv.apply([mats[x] if x else None for x in cv.amounts], LOGQ, src, NL, top, out)
                finally:
                    ctx.set_option("wave_operands", 0)
                assert np.array_equal(out.download((Cout, top, 2, n, NL)), want[1]), "chunks below count"
                cv.close()


# ------------------------------------------------------------------------------------------------ through the scheme
def test_conv_through_the_scheme():
    """(4096, 65537, logQ 128), two rows of 1024: 32 images of 4 x 8 per row, every one different, 3 x 3, 2 -> 3 channels, both forms: EVERY decrypted slot is
    the direct convolution modulo p.  The budgets are printed beside a fresh ciphertext's and the same map through fhesi_linear_grid on its Toeplitz matrix."""
    ctx, S, (sk1, pk0, pk1), mats = ring(4096)
    p, n, count = S.p, S.total, 2
    H, W, Cin, Cout, anchor = 4, 8, 2, 3, (1, 1)
    rng = np.random.default_rng(19)
    ctb = 2 * n * NL * 8
    K, b = rng.integers(0, p, size=(Cout, Cin, 3, 3)), rng.integers(0, p, size=Cout)
    x = rng.integers(0, p, size=(Cin, count, S.rows, S.cols // (H * W), H, W))
    xs = S.pack_images(x)
    assert xs.shape == (Cin, count, n) and np.array_equal(S.unpack_images(xs, H, W), x) and xs[1][1][S.cols + 32 + 8 + 3] == x[1][1][1][1][1][3]
    cx, out = ctx.alloc(Cin * count * ctb), ctx.alloc(Cout * count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 7000, 0, xs.reshape(Cin * count, n), cx, NL, only_usable=False)
    print("noise budget of the fresh inputs:", I(S.noise_budget(sk1, LOGQ, cx, NL, Cin * count)))
    want = [CM.direct(K, b, xs[:, i], H, W, anchor, p, S.rows) for i in range(count)]
    for form in (1, 2):
        cv = S.conv2d(K, b, (H, W), anchor, form)
        cv.apply(mats, LOGQ, cx, NL, count, out)
        got = S.decrypt_batch(sk1, LOGQ, out, NL, Cout * count, only_usable=False).reshape(Cout, count, n)
        for i in range(count):
            for Ic in range(Cout):
                assert I(got[Ic][i]) == I(want[i][Ic]), (form, Ic, i)
        budget = np.asarray(S.noise_budget(sk1, LOGQ, out, NL, Cout * count))
        print("noise budget after the 3 x 3 convolution, 2 -> 3 channels on 4 x 8, form %d (%d key switches):" % (form, cv.key_switches), I(budget))
        assert (budget > 0).all()
        cv.close()
    # the same map on one image per row, replicated, through the grid on the Toeplitz matrix (blocks of 32 x 32)
    M = CM.toeplitz(K, H, W, anchor, p)
    lin = S.linear_grid(M, np.repeat(b, H * W), (H * W, H * W))
    _, _, hoisted = rotation_keys(ctx, LOGQ, [S.rotation_k(a) for a in lin.amounts])      # (the same seed: the same secret key)
    img = rng.integers(0, p, size=(count, S.rows, Cin * H * W))
    cg, og = ctx.alloc(Cin * count * ctb), ctx.alloc(Cout * count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 7100, 0, S.replicate_blocks(img, H * W).reshape(Cin * count, n), cg, NL, only_usable=False)
    lin.apply(dict(zip(lin.amounts, hoisted)), LOGQ, cg, NL, count, og)
    tg = S.decrypt_batch(sk1, LOGQ, og, NL, Cout * count, only_usable=False).reshape(Cout, count, n)
    for i in range(count):
        per = np.stack([np.tile(img[i][:, J * H * W:(J + 1) * H * W], S.cols // (H * W)).reshape(-1) for J in range(Cin)])
        d = CM.direct(K, b, per, H, W, anchor, p, S.rows)
        assert all(I(tg[Ic][i]) == I(d[Ic]) for Ic in range(Cout)), i
    print("noise budget of the same map through linear_grid on its Toeplitz matrix (%d key switches):" % lin.key_switches,
          I(S.noise_budget(sk1, LOGQ, og, NL, Cout * count)))
    lin.close()


def test_the_edges_of_the_places_the_matrices_go_to_in_chunks_of_one_ciphertext():
    """(4096, 65537, logQ 128), the 4 x 8 plane, two ciphertexts per channel, "wave_operands" set so that a chunk is ONE of them.  The layer's run call puts
    the caller's matrices at their places among babies and giants: a 1 x 1 kernel, 2 -> 2 channels with a bias, has the anchor as its ONLY entry and takes no
    matrix -- on every pixel, and at step (2, 2), stride (2, 2), where every slot off the output lattice (4, 4) decrypts to 0, the bias included; a split
    3 x 3 kernel anchored at (2, 2) has its null entries LAST among the babies and last among the giants; the flat 3 x 3 of 2 -> 3 channels leaves a chunk's
    sums where the result does not go.  Each: the words of the composition, and every decrypted slot the model's."""
    import lattice_model as LM
    from test_gpu_lattice import lattice_composition, ring as lattice_ring      # (that module imports this one; its ring holds the amounts c - 2 and c - 16)
    ctx, S, (sk1, pk0, pk1), mats = lattice_ring(4096)
    p, n, count, c = S.p, S.total, 2, S.cols
    H, W = 4, 8
    ctb = 2 * n * NL * 8
    rng = np.random.default_rng(41)
    xs = rng.integers(1, p, size=(2, count, n))                     # every slot live or garbage, never 0
    cx = ctx.alloc(2 * count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 7400, 0, xs.reshape(2 * count, n), cx, NL, only_usable=False)
    unit = ((1, 1), (1, 1), (1, 1))
    # (kernel, Cout, anchor, form, geometry, the rotated ciphertexts or key-switched sums of one item, the amounts)
    cases = [((1, 1), 2, (0, 0), 1, unit, 2, [0]),
             ((1, 1), 2, (0, 0), 1, ((2, 2), (2, 2), (1, 1)), 2, [0]),
             ((3, 3), 2, (2, 2), 2, unit, 6, [c - 2, c - 1, 0, c - 16, c - 8, 0]),
             ((3, 3), 3, (1, 1), 1, unit, 18, [c - 9, c - 8, c - 7, c - 1, 0, 1, 7, 8, 9])]
    for (kh, kw), Cout, anchor, form, geom, per_item, amounts in cases:
        K, b = rng.integers(0, p, size=(Cout, 2, kh, kw)), rng.integers(1, p, size=Cout)
        cv = S.conv2d(K, b, (H, W), anchor, form, step=geom[0], stride=geom[1], dilation=geom[2])
        assert (cv.form, cv.amounts, cv.nh, cv.has_bias) == (form, amounts, len(amounts), True)
        want = lattice_composition(ctx, S, mats, K, b, (H, W), anchor, geom, form, cx, count)
        out = ctx.alloc(Cout * count * ctb)
        ctx.set_option("wave_operands", per_item)
        try:
            cv.apply(mats, LOGQ, cx, NL, count, out)
        finally:
            ctx.set_option("wave_operands", 0)
        assert np.array_equal(out.download((Cout, count, 2, n, NL)), want), ((kh, kw), anchor, form, geom)
        got = S.decrypt_batch(sk1, LOGQ, out, NL, Cout * count, only_usable=False).reshape(Cout, count, n)
        for i in range(count):
            model = LM.direct(K, b, xs[:, i], H, W, anchor, *geom, p, S.rows)
            for Ic in range(Cout):
                assert I(got[Ic][i]) == I(model[Ic]), ((kh, kw), anchor, form, geom, Ic, i)
        off = LM.lattice(H, W, cv.out_step, S.rows, S.cols) == 0
        assert off.sum() == (0 if geom == unit else 15 * n // 16) and not got[:, :, off].any()
        cv.close()


# ------------------------------------------------------------------------------------------------ a network
def test_conv_activation_dense_network():
    """(4096, 65537, logQ 256): conv 1 -> 2 channels, 3 x 3 on 4 x 4 with the image replicated in every block, the activation x^2, a 4 x 32 dense layer as a
    grid of (4, 16) blocks whose input blocks ARE the convolution's output channels; every slot against the integer model, the budget after each step"""
    from test_gpu_poly import s2_matrix
    m, p, g, logQ, nl, count = 4096, 65537, 3, 256, 4, 2
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    n, H, W = S.total, 4, 4
    rng = np.random.default_rng(23)
    K, b = rng.integers(0, p, size=(2, 1, 3, 3)), rng.integers(0, p, size=2)
    M, b2 = rng.integers(0, p, size=(4, 32)), rng.integers(0, p, size=4)
    cv, lin = S.conv2d(K, b, (H, W)), S.linear_grid(M, b2, (4, 16))
    assert cv.anchor == (1, 1) and (lin.nI, lin.nJ) == (1, 2)
    amounts = sorted((set(cv.amounts) | set(lin.amounts)) - {0})
    (sk1, pk0, pk1), _, hoisted = rotation_keys(ctx, logQ, [S.rotation_k(a) for a in amounts])
    mats = dict(zip(amounts, hoisted))
    ksk = s2_matrix(ctx, logQ, sk1, 77)
    img = rng.integers(0, p, size=(count, S.rows, 1, H, W))
    xs = S.pack_images(np.broadcast_to(img, (count, S.rows, S.cols // (H * W), H, W)))
    ctb = 2 * n * nl * 8
    c0, c1, c2, c3 = ctx.alloc(count * ctb), ctx.alloc(2 * count * ctb), ctx.alloc(2 * count * ctb), ctx.alloc(count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, logQ, 15, 0, xs, c0, nl, only_usable=False)
    cv.apply(mats, logQ, c0, nl, count, c1)
    S.poly_eval(ksk, [0, 0, 1], logQ, c1, nl, 2 * count, c2)
    lin.apply(mats, logQ, c2, nl, count, c3)
    got = S.decrypt_batch(sk1, logQ, c3, nl, count, only_usable=False)
    for i in range(count):
        conv = CM.direct(K, b, xs[i][None, :], H, W, (1, 1), p, S.rows)                                   # [2][total]
        h = np.array([[int(v) ** 2 % p for J in range(2) for v in conv[J][r * S.cols:r * S.cols + H * W]] for r in range(S.rows)], dtype=object)      # [rows][32]
        assert I(got[i]) == GM.expected_slots(M, b2, h, 4, p, S.rows, S.cols)[0], i
    budgets = [I(S.noise_budget(sk1, logQ, c, nl, k * count)) for c, k in ((c0, 1), (c1, 2), (c2, 2), (c3, 1))]
    print("noise budget fresh, after the convolution (form %d), after x^2, after the dense grid:" % cv.form, budgets)
    assert min(budgets[3]) > 0
    cv.close()
    lin.close()


# ------------------------------------------------------------------------------------------------ a slot basis
def test_conv_over_a_slot_basis():
    """two primes below 2^20 on m = 4096: 3 x 3 on 2 x 4, 2 -> 2 channels of 12-bit weights and data -- the exact sums exceed either prime and stay inside
    (-P/2, P/2)"""
    m, g = 4096, 3
    primes = F.slots_basis_plan(m, 30, 20, g)["primes"]
    assert len(primes) == 2
    chain, roots = P.chain_for(m, LOGQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k, count, Cin, Cout = B.total, B.k, 2, 2, 2
    S0 = B.channel(0)
    rng = np.random.default_rng(31)
    K, b = rng.integers(0, 1 << 12, size=(Cout, Cin, 3, 3)), rng.integers(-(1 << 19), 1 << 19, size=Cout)
    layers = B.conv2d(K, b, PLANE, (1, 1), 2)
    amounts = [a for a in layers[0].amounts if a]
    assert all(l.amounts == layers[0].amounts and l.form == 2 for l in layers)
    (sk1, pk0, pk1), _, hoisted = rotation_keys(ctx, LOGQ, [S0.rotation_k(a) for a in amounts])
    x = rng.integers(0, 1 << 12, size=(Cin, count, n))
    big = B.modulus
    exact = [CM.direct(K, b, x[:, i], PLANE[0], PLANE[1], (1, 1), big, S0.rows) for i in range(count)]
    centred = lambda v: int(v) - big if int(v) > big // 2 else int(v)
    top = max(abs(centred(v)) for e in exact for row in e for v in row)
    assert top > max(primes) and top < big // 2
    words = 2 * n * NL * 8
    cx, out = ctx.alloc(k * Cin * count * words), ctx.alloc(k * Cout * count * words)
    B.encrypt_batch_seeded(pk0, pk1, LOGQ, 79, 0, x.reshape(Cin * count, n), cx, NL)
    B.conv2d_apply(layers, dict(zip(amounts, hoisted)), LOGQ, cx, NL, count, out)
    got = B.decrypt_batch(sk1, LOGQ, out, NL, Cout * count)
    for Ic in range(Cout):
        for i in range(count):
            assert I(got[Ic * count + i]) == [centred(v) for v in exact[i][Ic]], (Ic, i)
    for l in layers:
        l.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_condition_and_leave_the_context_working():
    ctx, S, _, mats = ring(4096)
    n, count = ctx.phim, 2
    ctb = 2 * n * NL * 8
    rng = np.random.default_rng(3)
    K, b = rng.integers(0, S.p, size=(3, 2, 3, 3)), rng.integers(0, S.p, size=3)
    cv = S.conv2d(K, b, PLANE, (1, 1), 2)
    c = S.cols
    assert cv.amounts == [c - 1, 0, 1, c - 4, 0, 4] and (cv.nh, cv.key_switches) == (6, 2 * 2 + 3 * 2)
    good_mats = [mats[a] if a else None for a in cv.amounts]
    src = ctx.upload(np.stack([inputs(rng, count, n, NL, LOGQ) for _ in range(2)]))
    out = ctx.alloc(3 * count * ctb)

    def call(hs=good_mats, s=src, o=out, l=cv, **kw):
        l.apply(hs, LOGQ, s, NL, count, o, **kw)
        return o.download((3, count, 2, n, NL))

    good = call()

    def refused(word, fn):
        with pytest.raises(F.FhesiError) as e:
            fn()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(call(), good), word               # a following good call returns the same words

    ones = lambda *shape: np.ones(shape, dtype=np.int64)
    # the shape: the plane, the sizes, the anchor, an empty mask with its offset, the rows of one handle, the form
    refused("the plane of 3 x 4 pixels does not divide the row", lambda: S.conv2d(ones(1, 1, 1, 1), image=(3, 4)))
    refused("does not divide", lambda: S.conv2d_masks(ones(1, 1, 1, 1), (2048, 1)))
    refused("at least 1", lambda: S.conv2d(ones(1, 1, 1, 1), image=(0, 4)))
    refused("at least 1", lambda: S.conv2d_masks(ones(1, 1, 3, 3), (2, 0)))
    refused("the anchor (3, 1) is outside the 3 x 3 kernel", lambda: S.conv2d(ones(1, 1, 3, 3), image=PLANE, anchor=(3, 1)))
    refused("the anchor (0, -1) is outside", lambda: S.conv2d_masks(ones(1, 1, 3, 3), PLANE, (0, -1)))
    refused("the offset (2, -1) has an empty mask on the 2 x 4 plane", lambda: S.conv2d(ones(1, 1, 3, 3), image=PLANE, anchor=(0, 1)))
    refused("the offset (0, 4) has an empty mask", lambda: S.conv2d_masks(ones(1, 1, 1, 5), PLANE, (0, 0)))
    refused("per handle", lambda: S.conv2d(ones(86, 86, 3, 3), image=PLANE))
    refused("form 3", lambda: S.conv2d(ones(1, 1, 3, 3), image=PLANE, form=3))
    refused("form -1", lambda: F.conv2d_plan(S.cols, 2, 4, 1, 1, 3, 3, 1, 1, -1))
    # a null kernel, through the C ABI itself
    lib, h = F.Backend.lib(), ctypes.c_void_p()

    def null_kernel(fn):
        if fn(S.h, None, 1, 1, 3, 3, 2, 4, 1, 1, None, 0, ctypes.byref(h)) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("null kernel", lambda: null_kernel(lib.fhesi_conv2d_create))
    refused("null kernel", lambda: null_kernel(lib.fhesi_conv2d_create_dev))
    # the matrices: their count, one missing, one at the anchor, their order, one not hoisted
    refused("matrices, the layer takes 6", lambda: call(hs=good_mats[:5]))
    refused("matrices, the layer takes 6", lambda: call(hs=good_mats + [None]))
    refused("has no matrix and its amount is 1", lambda: call(hs=good_mats[:2] + [None] + good_mats[3:]))
    refused("whose amount is 0", lambda: call(hs=[good_mats[0], mats[1]] + good_mats[2:]))
    refused("whose amount is 0", lambda: call(hs=good_mats[:4] + [mats[4], mats[4]]))
    refused("hoisted for k=", lambda: call(hs=[mats[1], None, mats[c - 1]] + good_mats[3:]))
    refused("hoisted for k=", lambda: call(hs=good_mats[:3] + [mats[4], None, mats[c - 4]]))
    _, autos, _ = rotation_keys(ctx, LOGQ, [S.rotation_k(1)])
    refused("was not made by fhesi_ksk_hoist", lambda: call(hs=good_mats[:2] + [autos[0]] + good_mats[3:]))
    # another context: a matrix, the layer itself
    primes, roots = P.chain_for(4096, LOGQ, S.p)
    other = F.Context(4096, primes, roots)
    SO = F.SlotSpace.pow2(other, S.p, S.generator)
    _, _, foreign = rotation_keys(other, LOGQ, [S.rotation_k(1)])
    foreign_cv = SO.conv2d(K, b, PLANE, (1, 1), 2)
    refused("another context", lambda: call(hs=good_mats[:2] + [foreign[0]] + good_mats[3:]))

    def foreign_layer():
        arr = (ctypes.c_void_p * 6)(*[x.h if x is not None else None for x in good_mats])
        if lib.fhesi_ct_conv2d_dev(ctx.h, foreign_cv.h, arr, 6, LOGQ, 3, src.ptr, NL, count, out.ptr) != 0:
            raise F.FhesiError(lib.fhesi_last_error().decode())
    refused("convolution layer belongs to another context", foreign_layer)
    foreign_cv.close()
    # the buffers -- out over the SECOND input channel --, the digits, the limbs
    refused("overlaps", lambda: call(o=src))
    refused("overlaps", lambda: call(o=View(src, count * ctb)))
    refused("digits", lambda: call(decomp_bytes=2))
    cv.close()


def test_a_sum_past_the_capacity_of_the_chain_is_refused():
    """two primes just below 2^60 on (64, 257), logQ 105: a sum of 2 products needs 119 bits, a sum of 4 needs 120 -- and the chain's 120 must EXCEED what a
    sum needs.  1 x 1 kernels take no matrix and their sums have Cin terms: 2 -> 1 channels run, 4 -> 1 are refused before anything is launched"""
    logQ = 105
    primes, roots = P.first_primes(64, 2)
    ctx = F.Context(64, primes, roots)
    S = F.SlotSpace.pow2(ctx, 257, 3)
    n, count = ctx.phim, 2
    rng = np.random.default_rng(4)
    src = ctx.upload(np.stack([inputs(rng, count, n, NL, logQ) for _ in range(4)]))
    out = ctx.alloc(count * 2 * n * NL * 8)
    two = S.conv2d(np.array([3, -4], dtype=np.int64).reshape(1, 2, 1, 1), None, (4, 4))
    four = S.conv2d(np.array([3, -4, 5, 6], dtype=np.int64).reshape(1, 4, 1, 1), None, (4, 4))
    assert (two.terms, four.terms) == (2, 4)

    def run(cv):
        cv.apply([None], logQ, src, NL, count, out)
        return out.download((count, 2, n, NL))

    good = run(two)
    with pytest.raises(F.FhesiError, match="a sum of 4 products needs 120 bits, the chain holds 120"):
        run(four)
    assert np.array_equal(run(two), good)
    two.close()
    four.close()
