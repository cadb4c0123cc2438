"""GPU: strided and dilated convolutions, sum pooling and the dense bridge on packed slots whose live pixels sit on a lattice of the plane
(fhesi_conv2d_lattice_*, fhesi_ct_pool2d_dev, fhesi_slots_lattice_columns) through the C ABI -- the masked weight plaintexts conv_lattice_mask_kernel writes
against the model of tests/lattice_model.py without any key, the calls word for word against the compositions of existing entry points they are defined as,
through the scheme, inside a small network, over a slot basis, and the refusals.  Exact throughout."""
import functools

import numpy as np
import pytest

import conv_model as CM
import fhe_si_amd as F
import lattice_model as LM
import linear_grid_model as GM
import params as P
from bsgs_common import inputs, rotation_keys
from slots_common import I, View, context
from test_gpu_conv import RINGS, kernel, shape_of
from test_gpu_linear import DevTensor, planted
from test_lattice_model import SPACES, sweep

pytestmark = pytest.mark.gpu
LOGQ, NL = 128, 2
PLANE = (4, 8)
# (step, stride, dilation) of the 3 x 3 convolution on the 4 x 8 plane: stride 2; the same on a step-(2, 2) input; on a step-(1, 1) input with dilation 2
GEOMETRIES = [((1, 1), (2, 2), (1, 1)), ((2, 2), (2, 2), (1, 1)), ((1, 1), (2, 2), (2, 2))]
# (window, step) of the poolings on the 4 x 8 plane: 2 x 2, 4 x 2, and the global pooling of the 4 x 4 logical plane of step (1, 2)
POOLS = [((2, 2), (1, 1)), ((4, 2), (1, 1)), ((4, 4), (1, 2))]


# ------------------------------------------------------------------------------------------------ the masks, no keys
@functools.lru_cache(maxsize=None)
def small(m):
    """m = 64 / 256, p = 257, g = 3: two rows of 16 / 64 slots"""
    ctx, _ = context(m, LOGQ, 257)
    plan = F.slots_plan_pow2(m, 257, 3)
    assert (plan["rows"], plan["cols"], plan["total"]) == (2, m // 4, m // 2)
    S = F.SlotSpace.pow2(ctx, 257, 3)
    assert (S.rows, S.cols, S.generator) == (2, m // 4, 3)
    return ctx, S


@pytest.mark.parametrize("cols,plane", SPACES)
def test_masks_equal_the_model_on_both_forms(cols, plane):
    """rows of 16 (m = 64) and of 64 (m = 256): at m = 256 the 8 x 8 plane fills a row -- the split form's move-back wraps the row's end -- and the 4 x 8 plane
    holds two images per row; every step, stride, dilation, kernel and anchor of the CPU sweep, bit for bit"""
    ctx, S = small(4 * cols)
    H, W = plane
    rng = np.random.default_rng(cols + 10 * H + W)
    ran = 0
    for step, stride, dilation, kh, kw, anchor, Cin, Cout in sweep(cols, H, W):
        if LM.refused(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], step, stride, dilation) is not None:
            continue
        K = kernel(rng, S.p, Cout, Cin, kh, kw)
        for form in (LM.FLAT, LM.SPLIT):
            want = LM.prepared(K, H, W, anchor, step, stride, dilation, 2, cols, form) % S.p
            got = S.conv2d_lattice_masks(K, (H, W), anchor, form, step, stride, dilation)
            assert got.shape == (Cout, Cin, kh * kw, S.total) and np.array_equal(got.astype(object), want), (step, stride, dilation, (kh, kw), anchor, Cin, Cout, form)
        ran += 1
    assert ran >= 20


def test_trivial_geometry_chunks_constructors_and_columns():
    """with step, stride and dilation (1, 1) the lattice kernel writes the words of conv2d_masks; a stage of three chunks writes the same masks; the host and
    the device constructor give equal handles, equal to the composition, through layers that take no matrix; lattice_columns against numpy"""
    ctx, S = small(256)
    rng = np.random.default_rng(12)
    for (H, W), (kh, kw, anchor) in [((8, 8), (3, 3, (1, 1))), ((4, 8), (3, 3, (0, 2))), ((4, 4), (2, 2, (0, 0))), ((1, 16), (1, 3, (0, 1))), ((2, 8), (3, 5, (1, 2)))]:
        K = kernel(rng, S.p, 3, 2, kh, kw)
        for form in (1, 2):
            assert np.array_equal(S.conv2d_lattice_masks(K, (H, W), anchor, form), S.conv2d_masks(K, (H, W), anchor, form)), ((H, W), (kh, kw), form)
    # six channel pairs of nine plaintexts in chunks of two pairs
    K = kernel(rng, S.p, 3, 2, 3, 3)
    geom = dict(step=(2, 1), stride=(1, 2), dilation=(1, 2))
    whole = [S.conv2d_masks(K, (8, 8), (1, 1), form, **geom) for form in (1, 2)]
    assert all(np.array_equal(whole[form - 1].astype(object), LM.prepared(K, 8, 8, (1, 1), (2, 1), (1, 2), (1, 2), 2, 64, form) % S.p) for form in (1, 2))
    ctx.set_option("stage_chunk_bytes", 2 * 9 * S.total * 8 + 100)
    try:
        assert all(np.array_equal(S.conv2d_masks(K, (8, 8), (1, 1), form, **geom), whole[form - 1]) for form in (1, 2))
        run_without_a_matrix(ctx, S, True)
    finally:
        ctx.set_option("stage_chunk_bytes", 0)
    run_without_a_matrix(ctx, S, False)
    # the bridge: host and device
    for nch, (H, W), step, R in [(2, (4, 8), (2, 2), 4), (1, (8, 8), (1, 1), 3), (3, (8, 8), (4, 2), 5), (2, (1, 16), (1, 4), 1), (1, (4, 4), (4, 4), 7)]:
        M = planted(rng, S.p, R, nch * (H // step[0]) * (W // step[1]))
        want = LM.lattice_columns(M, nch, H, W, step)
        assert np.array_equal(S.lattice_columns(M, nch, (H, W), step), want)
        out = DevTensor(ctx, np.full(want.shape, -7, dtype=np.int64))
        S.lattice_columns(DevTensor(ctx, M), nch, (H, W), step, device=True, out=out)
        assert np.array_equal(out.buf.download(want.shape, np.int64), want)
    # through the C ABI itself: the binding sizes the output, so it checks the step first
    lib, M, res = F.Backend.lib(), np.zeros(8, dtype=np.int64), np.zeros(32, dtype=np.int64)
    assert lib.fhesi_slots_lattice_columns(S.h, F.binding._p(M), 1, 1, 4, 8, 3, 1, F.binding._p(res)) != 0
    assert "the step (3, 1) does not divide the 4 x 8 plane" in lib.fhesi_last_error().decode()
    assert lib.fhesi_slots_lattice_columns(S.h, None, 1, 1, 4, 8, 2, 2, F.binding._p(res)) != 0 and "null argument" in lib.fhesi_last_error().decode()
    with pytest.raises(ValueError, match="lattice_columns"):
        S.lattice_columns(np.zeros((1, 9), dtype=np.int64), 1, (4, 8), (2, 2))
    # pack_images / unpack_images with a step: the logical planes onto the lattice and back
    logical = rng.integers(1, S.p, size=(3, S.rows, S.cols // 32, 2, 4))
    vals = S.pack_images(logical, step=(2, 2))
    assert vals.shape == (3, S.total) and np.count_nonzero(vals) == logical.size and np.array_equal(S.unpack_images(vals, 4, 8, step=(2, 2)), logical)
    assert np.array_equal(vals != 0, np.broadcast_to(LM.lattice(4, 8, (2, 2), S.rows, S.cols) == 1, vals.shape))


def lattice_composition(ctx, S, mats, K, bias, image, anchor, geom, form, src, count, logQ=LOGQ, nl=NL):
    """the composition test_gpu_conv.composition spells out, fed with the model's lattice plaintexts, amounts and bias rows -> [Cout][count][2][n][nl]"""
    Cout, Cin, kh, kw = K.shape
    rows, cols = shape_of(S)
    pl = LM.plan(cols, image[0], image[1], Cin, Cout, kh, kw, anchor[0], anchor[1], *geom, form)
    w = (LM.prepared(K, image[0], image[1], anchor, *geom, rows, cols, pl["form"]) % S.p).astype(np.int64).reshape(Cout * Cin * kh * kw, S.total)
    plain = S.plain(w, False)
    B, G = (kh * kw, 1) if pl["form"] == LM.FLAT else (kw, kh)
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
    if pl["form"] == LM.SPLIT:
        out, rot = ctx.alloc(Cout * count * ctb), ctx.alloc(count * ctb)
        for Ic in range(Cout):
            y = View(out, Ic * count * ctb)
            for g in range(G):
                ctx.ct_rotations_dev([mats[kg[g]] if kg[g] else None], [S.rotation_k(kg[g])], logQ, View(inner, (Ic * G + g) * count * ctb), nl, count, rot if g else y, nl)
                if g:
                    ctx.ct_add_dev(logQ, y, rot, 2, nl, count)
    if bias is not None:
        bv = LM.bias_values(bias, image[0], image[1], pl["out_step"], S.p, rows, cols).astype(np.int64)
        for Ic in range(Cout):
            S.ct_add_slots_dev(logQ, View(out, Ic * count * ctb), 2, nl, count, bv[Ic][None, :], only_usable=False)
    plain.close()
    return out.download((Cout, count, 2, ctx.phim, nl))


def run_without_a_matrix(ctx, S, chunked):
    """1 x 1 kernels take no matrix: out[I] = [on the output lattice] (sum_J K[I][J] in[J] + b[I]) -- the host and the device constructor give equal handles,
    equal to the composition; 2 -> 3 channels are six pairs: three chunks of two where the stage is capped"""
    n, count = ctx.phim, 2
    geom = ((2, 1), (2, 4), (1, 1))
    for Cin, Cout in ((1, 1), (2, 3)):
        if chunked:
            ctx.set_option("stage_chunk_bytes", 2 * S.total * 8 + 100)
        rng = np.random.default_rng(Cin)
        K, b = kernel(rng, 257, Cout, Cin, 1, 1), np.array([300, -1, 1 << 62][:Cout], dtype=np.int64)
        src = ctx.upload(np.concatenate([inputs(np.random.default_rng(J + 1), count, n, NL, LOGQ) for J in range(Cin)]))
        outs = []
        kw = dict(step=geom[0], stride=geom[1], dilation=geom[2])
        for cv in (S.conv2d(K, b, (8, 8), **kw), S.conv2d(DevTensor(ctx, K), DevTensor(ctx, b), (8, 8), device=True, **kw)):
            assert (cv.shape, cv.image, cv.anchor, cv.form, cv.nh, cv.amounts, cv.key_switches, cv.terms, cv.has_bias) == ((Cout, Cin, 1, 1), (8, 8), (0, 0), 1, 1, [0], 0, Cin, True)
            assert (cv.step, cv.stride, cv.dilation, cv.out_step) == (geom[0], geom[1], geom[2], (4, 4))
            out = ctx.alloc(Cout * count * 2 * n * NL * 8)
            cv.apply([None], LOGQ, src, NL, count, out)
            outs.append(out.download((Cout, count, 2, n, NL)))
            cv.close()
        assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(outs[0], lattice_composition(ctx, S, {}, K, b, (8, 8), (0, 0), geom, 1, src, count))
    plain = S.conv2d(np.ones((1, 1, 1, 1), dtype=np.int64), None, (8, 8))
    assert (plain.step, plain.stride, plain.dilation, plain.out_step) == ((1, 1),) * 4
    plain.close()


# ------------------------------------------------------------------------------------------------ the calls against their definitions
def lattice_amounts(cols):
    out = set()
    for geom in GEOMETRIES:
        for form in (1, 2):
            out |= set(LM.plan(cols, PLANE[0], PLANE[1], 1, 1, 3, 3, 1, 1, *geom, form)["amounts"])
    for (kh, kw), (sy, sx) in POOLS:
        for form in (1, 2):
            out |= set(LM.pool_plan(cols, PLANE[0], PLANE[1], kh, kw, sy, sx, form)["amounts"])
    return sorted(out - {0})


@functools.lru_cache(maxsize=None)
def ring(m):
    """one context, its two-row space, keys made on the device and the hoisted matrices by amount: every amount of GEOMETRIES and POOLS on the 4 x 8 plane"""
    p, g = RINGS[m]
    primes, roots = P.chain_for(m, LOGQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    amounts = lattice_amounts(S.cols)
    assert amounts == sorted([1, 2, 4, 6, 7, 8, 9, 14, 16, 18, 24] + [S.cols - a for a in (1, 2, 7, 8, 9, 14, 16, 18)])
    keys, autos, hoisted = rotation_keys(ctx, LOGQ, [S.rotation_k(a) for a in amounts])
    return ctx, S, keys, dict(zip(amounts, hoisted))


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_conv_equals_the_composition_of_existing_calls(m):
    """2 -> 3 channels, 3 x 3 on the 4 x 8 plane: stride 2, the same on a step-(2, 2) input, and with dilation 2 on a step-(1, 1) input; both forms and the
    planner's; counts 1 and 3; with bias; the host and the device constructor; then the flat form in chunks of one ciphertext"""
    ctx, S, _, mats = ring(m)
    n, top, Cin, Cout = ctx.phim, 3, 2, 3
    rng = np.random.default_rng(m + 5)
    a = np.stack([inputs(rng, top, n, NL, LOGQ) for _ in range(Cin)])                 # [Cin][top]
    src = ctx.upload(a)
    for geom in GEOMETRIES:
        kw = dict(step=geom[0], stride=geom[1], dilation=geom[2])
        K = rng.integers(-S.p, 2 * S.p, size=(Cout, Cin, 3, 3)).astype(np.int64)
        bias = rng.integers(1, S.p, size=Cout).astype(np.int64)
        want = {form: lattice_composition(ctx, S, mats, K, bias, PLANE, (1, 1), geom, form, src, top) for form in (1, 2)}
        for form in (0, 1, 2):
            pl = LM.plan(S.cols, PLANE[0], PLANE[1], Cin, Cout, 3, 3, 1, 1, *geom, form)
            made = [(S.conv2d(K, bias, PLANE, (1, 1), form, **kw), (1, top))]
            if form == 0:
                made.append((S.conv2d(DevTensor(ctx, K), DevTensor(ctx, bias), PLANE, (1, 1), form, device=True, **kw), (top,)))
            for cv, counts in made:
                assert (cv.form, cv.nh, cv.amounts, cv.key_switches, cv.terms, cv.out_step) == (pl["form"], pl["nh"], pl["amounts"], pl["key_switches"], pl["terms"], pl["out_step"])
                for count in counts:
                    out = ctx.alloc(Cout * count * 2 * n * NL * 8)
                    cv.apply(mats, LOGQ, ctx.upload(a[:, :count]), NL, count, out)
                    assert np.array_equal(out.download((Cout, count, 2, n, NL)), want[pl["form"]][:, :count]), (geom, form, count)
                cv.close()
        if geom == GEOMETRIES[0]:
            cv = S.conv2d(K, bias, PLANE, (1, 1), 1, **kw)      # 18 rotated ciphertexts per item: one item per chunk
            out = ctx.alloc(Cout * top * 2 * n * NL * 8)
            ctx.set_option("wave_operands", 18)
            try:
                cv.apply(mats, LOGQ, src, NL, top, out)
            finally:
                ctx.set_option("wave_operands", 0)
            assert np.array_equal(out.download((Cout, top, 2, n, NL)), want[1]), "chunks below count"
            cv.close()


def pool_composition(ctx, S, mats, window, step, form, src, count, logQ=LOGQ, nl=NL):
    """form 1: y = Reduce(in) (a fold over no amount); per direction fhesi_ct_rotations_dev of y over the direction's amounts, then fhesi_ct_add_dev of every term
    onto y -- horizontal, then vertical.  form 2: fhesi_ct_rot_fold_dev over the plan's amounts -> [count][2][n][nl]"""
    pl = LM.pool_plan(S.cols, PLANE[0], PLANE[1], window[0], window[1], step[0], step[1], form)
    ctb = 2 * ctx.phim * nl * 8
    y = ctx.alloc(count * ctb)
    if pl["form"] == 2:
        ctx.ct_rot_fold_dev([mats[a] for a in pl["amounts"]], [S.rotation_k(a) for a in pl["amounts"]], logQ, src, nl, count, y)
        return y.download((count, 2, ctx.phim, nl))
    ctx.ct_rot_fold_dev([], [], logQ, src, nl, count, y)
    for amounts in (pl["amounts"][:pl["nhor"]], pl["amounts"][pl["nhor"]:]):
        if not amounts:
            continue
        rot = ctx.alloc(len(amounts) * count * ctb)
        ctx.ct_rotations_dev([mats[a] for a in amounts], [S.rotation_k(a) for a in amounts], logQ, y, nl, count, rot, nl)
        for t in range(len(amounts)):
            ctx.ct_add_dev(logQ, y, View(rot, t * count * ctb), 2, nl, count)
    return y.download((count, 2, ctx.phim, nl))


@pytest.mark.parametrize("m", [4096, 1 << 15])
def test_pooling_equals_the_composition_of_existing_calls(m):
    """2 x 2, 4 x 2 and the global pooling of a 4 x 4 logical plane in forms 1 and 2 and the planner's; counts 1 and 3; in place; chunks of one ciphertext"""
    ctx, S, _, mats = ring(m)
    n, top = ctx.phim, 3
    rng = np.random.default_rng(m + 6)
    a = inputs(rng, top, n, NL, LOGQ)
    src = ctx.upload(a)
    ctb = 2 * n * NL * 8
    for window, step in POOLS:
        want = {form: pool_composition(ctx, S, mats, window, step, form, src, top) for form in (1, 2)}
        for form in (0, 1, 2):
            pl = LM.pool_plan(S.cols, PLANE[0], PLANE[1], window[0], window[1], step[0], step[1], form)
            for count in (1, top):
                out = ctx.alloc(count * ctb)
                got = S.pool2d(mats, PLANE, window, step, LOGQ, ctx.upload(a[:count]), NL, count, out, form)
                assert got == pl
                assert np.array_equal(out.download((count, 2, n, NL)), want[pl["form"]][:count]), (window, step, form, count)
            same = ctx.upload(a)                                  # in == out
            S.pool2d([mats[x] for x in pl["amounts"]], PLANE, window, step, LOGQ, same, NL, top, same, form)
            assert np.array_equal(same.download((top, 2, n, NL)), want[pl["form"]]), (window, step, form, "in place")
        # form 1 in chunks of one ciphertext: three terms per ciphertext and direction at the most
        out = ctx.alloc(top * ctb)
        ctx.set_option("wave_operands", 3)
        try:
            S.pool2d(mats, PLANE, window, step, LOGQ, src, NL, top, out, 1)
        finally:
            ctx.set_option("wave_operands", 0)
        assert np.array_equal(out.download((top, 2, n, NL)), want[1]), (window, step, "chunks below count")


# ------------------------------------------------------------------------------------------------ through the scheme
def test_lattice_layers_through_the_scheme():
    """(4096, 65537, logQ 128), two rows of 1024: 32 images of 4 x 8 per row, every one different, garbage off the input lattice.  EVERY decrypted slot of every
    item is the model: the zeros off the output lattice of the convolutions, the cyclic sums of the pools.  A pooled result keeps at least the budget of the
    same sums taken by fhesi_ct_conv2d_dev with an all-ones kernel, which pays a plaintext product"""
    ctx, S, (sk1, pk0, pk1), mats = ring(4096)
    p, n, count = S.p, S.total, 2
    H, W, Cin, Cout, anchor = 4, 8, 2, 3, (1, 1)
    rng = np.random.default_rng(29)
    ctb = 2 * n * NL * 8
    K, b = rng.integers(0, p, size=(Cout, Cin, 3, 3)), rng.integers(1, p, size=Cout)
    xs = rng.integers(1, p, size=(Cin, count, n))                     # every slot live or garbage, never 0
    cx, out = ctx.alloc(Cin * count * ctb), ctx.alloc(Cout * count * ctb)
    S.encrypt_batch_seeded(pk0, pk1, LOGQ, 7300, 0, xs.reshape(Cin * count, n), cx, NL, only_usable=False)
    print("noise budget of the fresh inputs:", I(S.noise_budget(sk1, LOGQ, cx, NL, Cin * count)))
    for geom in GEOMETRIES:
        want = [LM.direct(K, b, xs[:, i], H, W, anchor, *geom, p, S.rows) for i in range(count)]
        for form in (1, 2):
            cv = S.conv2d(K, b, (H, W), anchor, form, step=geom[0], stride=geom[1], dilation=geom[2])
            cv.apply(mats, LOGQ, cx, NL, count, out)
            got = S.decrypt_batch(sk1, LOGQ, out, NL, Cout * count, only_usable=False).reshape(Cout, count, n)
            for i in range(count):
                for Ic in range(Cout):
                    assert I(got[Ic][i]) == I(want[i][Ic]), (geom, form, Ic, i)
            off = LM.lattice(H, W, cv.out_step, S.rows, S.cols) == 0
            assert off.sum() >= 3 * n // 4 and not got[:, :, off].any()
            budget = np.asarray(S.noise_budget(sk1, LOGQ, out, NL, Cout * count))
            print("noise budget after the 3 x 3 convolution, step %s stride %s dilation %s, form %d (%d key switches):" % (geom + (form, cv.key_switches)), I(budget))
            assert (budget > 0).all()
            cv.close()
    # the pools on the first input channel's items, beside the all-ones convolution that takes the same sums
    pooled = ctx.alloc(count * ctb)
    for window, step in POOLS:
        kh, kw = window
        want = [LM.pool_formula(xs[0][i], H, W, kh, kw, step[0], step[1], p, S.rows) for i in range(count)]
        ones = S.conv2d(np.ones((1, 1, kh, kw), dtype=np.int64), None, (H, W), (0, 0), 0, step=step)
        ref = ctx.alloc(count * ctb)
        ones.apply(mats, LOGQ, cx, NL, count, ref)
        sums = S.decrypt_batch(sk1, LOGQ, ref, NL, count, only_usable=False)
        on = LM.lattice(H, W, (step[0] * kh, step[1] * kw), S.rows, S.cols) == 1
        conv_budget = np.asarray(S.noise_budget(sk1, LOGQ, ref, NL, count))
        ones.close()
        for form in (1, 2):
            pl = S.pool2d(mats, (H, W), window, step, LOGQ, cx, NL, count, pooled, form)
            got = S.decrypt_batch(sk1, LOGQ, pooled, NL, count, only_usable=False)
            for i in range(count):
                assert I(got[i]) == I(want[i]), (window, step, form, i)
                assert np.array_equal(got[i][on], sums[i][on])      # the same sums, where the windows start
            budget = np.asarray(S.noise_budget(sk1, LOGQ, pooled, NL, count))
            print("noise budget after the %d x %d sum pooling at step %s, form %d (%d key switches, %d levels):" % (kh, kw, step, form, pl["key_switches"], pl["levels"]), I(budget),
                  "-- the all-ones convolution:", I(conv_budget))
            assert (budget > 0).all() and (conv_budget > 0).all()
            assert budget.min() >= conv_budget.min()


# ------------------------------------------------------------------------------------------------ a network
def test_strided_conv_activation_pool_dense_network():
    """(4096, 65537, logQ 256): conv 3 x 3 stride 2, 1 -> 2 channels on 8 x 8 with the image replicated in every block -> x^2 -> 2 x 2 sum pool -> a 4 x (2 2 2)
    dense layer over the logical pixels through lattice_columns and a grid of (4, 64) blocks whose input blocks ARE the channels; every slot against the
    integer model, the budget after each step"""
    from test_gpu_poly import s2_matrix
    m, p, g, logQ, nl, count = 4096, 65537, 3, 256, 4, 2
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    n, H, W = S.total, 8, 8
    rng = np.random.default_rng(37)
    K, b = rng.integers(0, p, size=(2, 1, 3, 3)), rng.integers(0, p, size=2)
    M, b2 = rng.integers(0, p, size=(4, 8)), rng.integers(0, p, size=4)
    cv = S.conv2d(K, b, (H, W), stride=(2, 2))
    pool = F.pool2d_plan(S.cols, H, W, 2, 2, *cv.out_step)
    assert cv.out_step == (2, 2) and pool["out_step"] == (4, 4)
    Mp = S.lattice_columns(M, 2, (H, W), pool["out_step"])
    assert Mp.shape == (4, 128) and np.count_nonzero(Mp) <= 32
    lin = S.linear_grid(Mp, b2, (4, H * W))
    assert (lin.nI, lin.nJ) == (1, 2)
    amounts = sorted((set(cv.amounts) | set(pool["amounts"]) | set(lin.amounts)) - {0})
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
    S.pool2d(mats, (H, W), (2, 2), cv.out_step, logQ, c2, nl, 2 * count, c2)
    budget_pool = I(S.noise_budget(sk1, logQ, c2, nl, 2 * count))
    lin.apply(mats, logQ, c2, nl, count, c3)
    got = S.decrypt_batch(sk1, logQ, c3, nl, count, only_usable=False)
    for i in range(count):
        conv = LM.direct(K, b, xs[i][None, :], H, W, (1, 1), (1, 1), (2, 2), (1, 1), p, S.rows)                # [2][total]
        sq = [[int(v) ** 2 % p for v in conv[J]] for J in range(2)]
        pooled = [LM.pool_direct(sq[J], H, W, 2, 2, 2, 2, p, S.rows) for J in range(2)]                          # [2][rows][nimg][2][2]
        h = np.array([[int(v) for J in range(2) for v in pooled[J][r][0].reshape(-1)] for r in range(S.rows)], dtype=object)      # [rows][8]
        assert I(got[i]) == GM.expected_slots(M, b2, h, 4, p, S.rows, S.cols)[0], i
    budgets = [I(S.noise_budget(sk1, logQ, c, nl, k * count)) for c, k in ((c0, 1), (c1, 2))] + [budget_pool, I(S.noise_budget(sk1, logQ, c3, nl, count))]
    print("noise budget fresh, after the stride-2 convolution (form %d), after x^2 and the 2 x 2 pool, after the dense grid:" % cv.form, budgets)
    assert min(budgets[3]) > 0
    cv.close()
    lin.close()


# ------------------------------------------------------------------------------------------------ a slot basis
def test_lattice_layers_over_a_slot_basis():
    """two primes below 2^20 on m = 4096: 3 x 3 with stride 2 on 2 x 4, 2 -> 2 channels of 12-bit weights and data, then the 1 x 2 pooling of its output -- the
    exact sums exceed either prime and stay inside (-P/2, P/2)"""
    m, g, plane = 4096, 3, (2, 4)
    primes = F.slots_basis_plan(m, 30, 20, g)["primes"]
    assert len(primes) == 2
    chain, roots = P.chain_for(m, LOGQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, k, count, Cin, Cout = B.total, B.k, 2, 2, 2
    S0 = B.channel(0)
    rng = np.random.default_rng(41)
    K, b = rng.integers(0, 1 << 12, size=(Cout, Cin, 3, 3)), rng.integers(-(1 << 19), 1 << 19, size=Cout)
    layers = B.conv2d(K, b, plane, (1, 1), 2, stride=(2, 2))
    pool = F.pool2d_plan(S0.cols, plane[0], plane[1], 1, 2, 2, 2)
    assert all(l.amounts == layers[0].amounts and l.form == 2 and l.out_step == (2, 2) for l in layers) and pool["amounts"] == [2]
    amounts = sorted({a for a in layers[0].amounts if a} | set(pool["amounts"]))
    (sk1, pk0, pk1), _, hoisted = rotation_keys(ctx, LOGQ, [S0.rotation_k(a) for a in amounts])
    mats = dict(zip(amounts, hoisted))
    x = rng.integers(0, 1 << 12, size=(Cin, count, n))
    big = B.modulus
    geom = ((1, 1), (2, 2), (1, 1))
    conv = [LM.direct(K, b, x[:, i], plane[0], plane[1], (1, 1), *geom, big, S0.rows) for i in range(count)]
    exact = [[LM.pool_formula(conv[i][Ic], plane[0], plane[1], 1, 2, 2, 2, big, S0.rows) for Ic in range(Cout)] for i in range(count)]
    centred = lambda v: int(v) - big if int(v) > big // 2 else int(v)
    top = max(abs(centred(v)) for e in exact for row in e for v in row)
    assert top > max(primes) and top < big // 2
    words = 2 * n * NL * 8
    cx, out = ctx.alloc(k * Cin * count * words), ctx.alloc(k * Cout * count * words)
    B.encrypt_batch_seeded(pk0, pk1, LOGQ, 83, 0, x.reshape(Cin * count, n), cx, NL)
    B.conv2d_apply(layers, mats, LOGQ, cx, NL, count, out)
    assert B.pool2d(mats, plane, (1, 2), (2, 2), LOGQ, out, NL, Cout * count, out) == pool
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
    c = S.cols
    src = ctx.upload(np.stack([inputs(rng, count, n, NL, LOGQ) for _ in range(2)]))      # two ciphertexts' room on either side
    out = ctx.alloc(2 * count * ctb)
    plan = F.pool2d_plan(c, 4, 8, 4, 2, 1, 1, 1)
    assert plan["amounts"] == [1, 8, 16, 24] and plan["nhor"] == 1
    good_mats = [mats[a] for a in plan["amounts"]]

    def call(hs=good_mats, s=src, o=out, window=(4, 2), step=(1, 1), form=1, image=PLANE, **kw):
        S.pool2d(hs, image, window, step, LOGQ, s, NL, count, o, form, **kw)
        return o.download((count, 2, n, NL))

    good = call()

    def refused(word, fn):
        with pytest.raises(F.FhesiError) as e:
            fn()
        assert word in str(e.value), (word, str(e.value))
        assert np.array_equal(call(), good), word               # a following good call returns the same words

    # the shape
    refused("the plane of 3 x 8 pixels does not divide the row", lambda: call(image=(3, 8)))
    refused("the step (3, 1) does not divide the 4 x 8 plane", lambda: call(step=(3, 1)))
    refused("windows of 3 x 2 pixels do not tile the logical plane of 4 x 8 pixels", lambda: call(window=(3, 2)))
    refused("windows of 4 x 2 pixels do not tile the logical plane of 2 x 8 pixels", lambda: call(step=(2, 1)))
    refused("every size at least 1", lambda: call(window=(0, 2)))
    refused("form 3", lambda: call(form=3))
    refused("form 2 (doubling) takes windows of powers of two, not 1 x 3", lambda: F.pool2d_plan(192, 1, 12, 1, 3, 1, 1, 2))      # (no such window tiles 4 x 8)
    # the matrices: their count, one missing, the wrong one for an amount, one not hoisted, one of another context
    refused("matrices, the pooling takes 4 (1 horizontal, 3 vertical", lambda: call(hs=good_mats[:3]))
    refused("matrices, the pooling takes 4", lambda: call(hs=good_mats + [mats[1]]))
    refused("entry 2 has no matrix and its amount is 16", lambda: call(hs=good_mats[:2] + [None] + good_mats[3:]))
    refused("hoisted for k=", lambda: call(hs=[mats[8], mats[1]] + good_mats[2:]))
    refused("hoisted for k=", lambda: call(hs=good_mats[:3] + [mats[c - 8]]))
    _, autos, _ = rotation_keys(ctx, LOGQ, [S.rotation_k(1)])
    refused("was not made by fhesi_ksk_hoist", lambda: call(hs=[autos[0]] + good_mats[1:]))
    primes, roots = P.chain_for(4096, LOGQ, S.p)
    other = F.Context(4096, primes, roots)
    SO = F.SlotSpace.pow2(other, S.p, S.generator)
    _, _, foreign = rotation_keys(other, LOGQ, [S.rotation_k(1)])
    refused("another context", lambda: call(hs=[foreign[0]] + good_mats[1:]))
    refused("another context", lambda: SO.pool2d(good_mats, PLANE, (4, 2), (1, 1), LOGQ, src, NL, count, out, 1))
    # the buffers: out half over in; the digits
    refused("out overlaps in without being in", lambda: call(o=View(src, ctb)))
    refused("digits", lambda: call(decomp_bytes=2))
    # the convolution on a lattice: the run call is fhesi_ct_conv2d_dev, and a matrix hoisted for the stride-1 amount is not the step-2 layer's
    K, b = rng.integers(0, S.p, size=(3, 2, 3, 3)), rng.integers(0, S.p, size=3)
    cv = S.conv2d(K, b, PLANE, (1, 1), 2, step=(2, 2), stride=(2, 2))
    assert cv.amounts == [c - 2, 0, 2, c - 16, 0, 16] and (cv.nh, cv.key_switches, cv.out_step) == (6, 2 * 2 + 3 * 2, (4, 4))
    cout = ctx.alloc(3 * count * ctb)
    for hs, word in (([mats[c - 1], None, mats[1], mats[c - 8], None, mats[8]], "hoisted for k="), ([mats[c - 2], None, None, mats[c - 16], None, mats[16]], "has no matrix and its amount is 2"),
                     ([mats[c - 2], None, mats[2], mats[c - 16], None], "matrices, the layer takes 6")):
        with pytest.raises(F.FhesiError, match=word):
            cv.apply(hs, LOGQ, src, NL, count, cout)
    with pytest.raises(F.FhesiError, match="overlaps"):
        cv.apply(mats, LOGQ, src, NL, count, View(src, count * ctb))
    cv.apply(mats, LOGQ, src, NL, count, cout)
    cv.close()
    for word, fn in (("the stride (3, 1) does not divide the logical plane of 4 x 8 pixels", lambda: S.conv2d(K, b, PLANE, stride=(3, 1))),
                     ("the step (1, 3) does not divide the 4 x 8 plane", lambda: S.conv2d_masks(K, PLANE, step=(1, 3))),
                     ("the offset (-4, -1) has an empty mask on the 4 x 8 plane", lambda: S.conv2d(K, b, PLANE, dilation=(4, 1))),
                     ("every factor at least 1", lambda: S.conv2d(K, b, PLANE, stride=(0, 1)))):
        refused(word, fn)
