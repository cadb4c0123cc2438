"""CPU: strided and dilated convolutions and sum pooling on packed slots whose live pixels sit on a lattice of the plane.  Both forms of the convolution's
schedule and both pooling forms equal the direct definitions on EVERY slot -- the zeros off the output lattice and the cyclic sums of the pools included --
with garbage planted off the input lattice; the planner's counts are those the schedule itself runs; fhesi_conv2d_lattice_plan and fhesi_pool2d_plan equal the
model, refusals included; the header declares the entry points at ABI revision 9; one strided convolution and one pooling run end to end through the Python
model of the scheme (oracle/fhesi_pyref.py).  Exact."""
import os
import random
import re

import numpy as np
import pytest

import conv_model as CM
import fhesi_pyref as R
import hoist_model as HM
import lattice_model as LM
import noise_model as NM
import params as P
import slots_pow2_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fhesi_conv2d_lattice_plan", "fhesi_conv2d_lattice_create", "fhesi_conv2d_lattice_create_dev", "fhesi_conv2d_lattice_masks", "fhesi_conv2d_lattice_info",
           "fhesi_pool2d_plan", "fhesi_ct_pool2d_dev", "fhesi_slots_lattice_columns", "fhesi_slots_lattice_columns_dev"]
ROWS, PRIME = 2, 257
SPACES = [(16, (4, 4)), (16, (2, 8)), (16, (1, 16)), (64, (4, 4)), (64, (2, 8)), (64, (8, 8)), (64, (4, 8)), (64, (1, 16))]
STEPS = [(1, 1), (2, 1), (1, 2), (2, 2)]
STRIDES = [(1, 1), (2, 1), (2, 2)]
DILATIONS = [(1, 1), (2, 2), (1, 2)]


def every_anchor(kh, kw):
    return [(a, b) for a in range(kh) for b in range(kw)]


def sweep(cols, H, W):
    """(step, stride, dilation, kh, kw, anchor, Cin, Cout): kernels up to 3 x 3 with every anchor on one channel, the centred anchor on 2 -> 3 channels"""
    for step in STEPS:
        for stride in STRIDES:
            for dilation in DILATIONS:
                for kh in range(1, 4):
                    for kw in range(1, 4):
                        for anchor in every_anchor(kh, kw):
                            for Cin, Cout in ((1, 1), (2, 3)):
                                if (Cin, Cout) != (1, 1) and anchor != ((kh - 1) // 2, (kw - 1) // 2):
                                    continue
                                yield step, stride, dilation, kh, kw, anchor, Cin, Cout


def planted(rng, H, W, step, Cin, cols):
    """another image in every block and row, values in [0, p) on the lattice and garbage off it"""
    xs = rng.integers(0, PRIME, size=(Cin, ROWS * cols))
    off = LM.lattice(H, W, step, ROWS, cols) == 0
    xs[:, off] = rng.integers(1, PRIME, size=(Cin, int(off.sum())))
    return xs


@pytest.mark.parametrize("cols,plane", SPACES)
def test_both_forms_equal_the_direct_definition_on_every_slot(cols, plane):
    H, W = plane
    rng = np.random.default_rng(1000 * cols + 100 * H + W)
    ran = refused = 0
    for step, stride, dilation, kh, kw, anchor, Cin, Cout in sweep(cols, H, W):
        word = LM.refused(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], step, stride, dilation)
        if word is not None:
            assert "does not divide" in word or "empty mask" in word, word
            refused += 1
            continue
        K = rng.integers(-PRIME, 2 * PRIME, size=(Cout, Cin, kh, kw))
        b = rng.integers(1, PRIME, size=Cout)                      # never 0: a bias off the output lattice would show
        xs = planted(rng, H, W, step, Cin, cols)
        want = LM.direct(K, b, xs, H, W, anchor, step, stride, dilation, PRIME, ROWS)
        out_step = (step[0] * stride[0], step[1] * stride[1])
        off = LM.lattice(H, W, out_step, ROWS, cols) == 0
        assert not want[:, off].any() and (out_step == (1, 1) or off.any())
        for form in (LM.FLAT, LM.SPLIT):
            counts = {}
            got = LM.schedule(K, b, xs, H, W, anchor, step, stride, dilation, PRIME, ROWS, form, counts)
            assert np.array_equal(got, want), (step, stride, dilation, kh, kw, anchor, Cin, Cout, form)
            pl = LM.plan(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], step, stride, dilation, form)
            assert counts["key_switches"] == pl["key_switches"] == CM.key_switches(Cin, Cout, kh, kw, form) and pl["out_step"] == out_step
        ran += 1
    assert ran >= 20 and refused >= 1, (ran, refused)


def test_trivial_geometry_is_the_stride_one_convolution():
    import fhe_si_amd as F
    rng = np.random.default_rng(5)
    for cols, (H, W) in SPACES:
        for kh in range(1, 6):
            for kw in range(1, 6):
                for ah, aw in sorted({(0, 0), ((kh - 1) // 2, (kw - 1) // 2), (kh - 1, kw - 1)}):
                    for Cin, Cout in ((1, 1), (2, 3), (3, 2)):
                        word = CM.refused(cols, H, W, Cin, Cout, kh, kw, ah, aw)
                        assert LM.refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, *LM.TRIVIAL) == word or (word and word in LM.refused(cols, H, W, Cin, Cout, kh, kw, ah, aw, *LM.TRIVIAL))
                        if word is not None:
                            with pytest.raises(F.FhesiError) as e:
                                F.conv2d_lattice_plan(cols, H, W, Cin, Cout, kh, kw, ah, aw)
                            assert word in str(e.value)
                            continue
                        for form in (0, 1, 2):
                            want = F.conv2d_plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, form)
                            got = F.conv2d_lattice_plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, form=form)
                            assert got.pop("out_step") == (1, 1) and got == want
        K = rng.integers(-PRIME, 2 * PRIME, size=(3, 2, 3, 3))
        if CM.refused(cols, H, W, 2, 3, 3, 3, 1, 1) is None:
            for form in (1, 2):
                assert np.array_equal(LM.prepared(K, H, W, (1, 1), *LM.TRIVIAL, ROWS, cols, form), CM.prepared(K, H, W, (1, 1), ROWS, cols, form))


def test_the_library_plans_equal_the_model_on_every_shape_of_the_sweep():
    import fhe_si_amd as F
    ran = 0
    for cols, (H, W) in SPACES:
        for step, stride, dilation, kh, kw, anchor, Cin, Cout in sweep(cols, H, W):
            args = (cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], step, stride, dilation)
            word = LM.refused(*args)
            for form in (0, 1, 2):
                if word is not None:
                    with pytest.raises(F.FhesiError) as e:
                        F.conv2d_lattice_plan(*args, form)
                    assert word in str(e.value) and "conv2d_lattice_plan" in str(e.value), (word, str(e.value))
                    break
                got, want = F.conv2d_lattice_plan(*args, form), LM.plan(*args, form)
                assert got == want, (args, form)
                assert [i for i, a in enumerate(got["amounts"]) if a == 0] == ([anchor[0] * kw + anchor[1]] if got["form"] == 1 else [anchor[1], kw + anchor[0]])
                ran += 1
        for sy, sx in STEPS:
            for kh in (1, 2, 3, 4, 8):
                for kw in (1, 2, 3, 4, 8, 16):
                    for form in (0, 1, 2):
                        word = LM.pool_refused(cols, H, W, kh, kw, sy, sx, form)
                        if word is not None:
                            with pytest.raises(F.FhesiError) as e:
                                F.pool2d_plan(cols, H, W, kh, kw, sy, sx, form)
                            assert word in str(e.value) and "pool2d_plan" in str(e.value), (word, str(e.value))
                            continue
                        assert F.pool2d_plan(cols, H, W, kh, kw, sy, sx, form) == LM.pool_plan(cols, H, W, kh, kw, sy, sx, form)
                        ran += 1
    assert ran > 3000
    # stride 2 on 32 x 32: the amounts of a 3 x 3 kernel do not change with the stride, only the masks do; on a step-2 input they double
    assert F.conv2d_lattice_plan(1024, 32, 32, 1, 8, 3, 3, 1, 1, stride=(2, 2)) == \
        {"form": 1, "nh": 9, "key_switches": 8, "terms": 9, "amounts": [991, 992, 993, 1023, 0, 1, 31, 32, 33], "out_step": (2, 2)}
    assert F.conv2d_lattice_plan(1024, 32, 32, 1, 1, 3, 3, 1, 1, step=(2, 2), stride=(2, 2), form=2) == \
        {"form": 2, "nh": 6, "key_switches": 4, "terms": 3, "amounts": [1022, 0, 2, 960, 0, 64], "out_step": (4, 4)}
    assert F.pool2d_plan(1024, 32, 32, 2, 2) == {"form": 1, "nh": 2, "nhor": 1, "key_switches": 2, "levels": 2, "amounts": [1, 32], "out_step": (2, 2)}
    assert F.pool2d_plan(1024, 32, 32, 4, 4, 2, 2) == {"form": 2, "nh": 4, "nhor": 2, "key_switches": 4, "levels": 4, "amounts": [2, 4, 64, 128], "out_step": (8, 8)}
    assert F.pool2d_plan(1024, 32, 32, 4, 4, 2, 2, 1)["amounts"] == [2, 4, 6, 64, 128, 192]
    assert F.pool2d_plan(1024, 32, 32, 32, 32)["key_switches"] == 10 and F.pool2d_plan(1024, 32, 32, 32, 32, form=1)["key_switches"] == 62


@pytest.mark.parametrize("cols,plane", SPACES)
def test_both_pooling_forms_equal_the_formula_and_the_window_sums(cols, plane):
    H, W = plane
    rng = np.random.default_rng(7 * cols + H)
    ran = 0
    for sy, sx in STEPS:
        for kh in (1, 2, 3, 4, 8):
            for kw in (1, 2, 3, 4, 8, 16):
                if LM.pool_refused(cols, H, W, kh, kw, sy, sx) is not None:
                    continue
                x = planted(rng, H, W, (sy, sx), 1, cols)[0]
                want = LM.pool_formula(x, H, W, kh, kw, sy, sx, PRIME, ROWS)
                # on the output lattice the formula holds the window sums of the logical plane, whatever lies off the input lattice
                on = CM.images(want, H, W, ROWS)[..., ::sy * kh, ::sx * kw]
                assert np.array_equal(on, LM.pool_direct(x, H, W, kh, kw, sy, sx, PRIME, ROWS)), (sy, sx, kh, kw)
                for form in (1, 2):
                    if LM.pool_refused(cols, H, W, kh, kw, sy, sx, form) is not None:
                        assert form == 2 and not (LM.is_pow2(kh) and LM.is_pow2(kw))
                        continue
                    counts = {}
                    assert np.array_equal(LM.pool_schedule(x, H, W, kh, kw, sy, sx, PRIME, ROWS, form, counts), want), (sy, sx, kh, kw, form)
                    pl = LM.pool_plan(cols, H, W, kh, kw, sy, sx, form)
                    assert (counts["key_switches"], counts["levels"]) == (pl["key_switches"], pl["levels"]) and 0 not in pl["amounts"]
                    assert pl["key_switches"] == ((kw - 1) + (kh - 1) if form == 1 else round(np.log2(kw) + np.log2(kh)))
                auto = LM.pool_plan(cols, H, W, kh, kw, sy, sx)
                both = [LM.pool_plan(cols, H, W, kh, kw, sy, sx, f) for f in (1, 2) if LM.pool_refused(cols, H, W, kh, kw, sy, sx, f) is None]
                assert auto == min(both, key=lambda q: (q["key_switches"], q["levels"]))
                ran += 1
    assert ran >= 8
    # global pooling: every lattice pixel of an image into its first slot
    Hl, Wl = H // 2 if H % 2 == 0 else H, W // 2 if W % 2 == 0 else W
    step = (H // Hl, W // Wl)
    x = planted(rng, H, W, step, 1, cols)[0]
    got = CM.images(LM.pool_schedule(x, H, W, Hl, Wl, step[0], step[1], PRIME, ROWS, 0), H, W, ROWS)[..., 0, 0]
    assert np.array_equal(got, CM.images(x, H, W, ROWS)[..., ::step[0], ::step[1]].sum(axis=(-1, -2)) % PRIME)


@pytest.mark.parametrize("args,word", [
    ((16, 4, 4, 1, 1, 3, 3, 1, 1, (3, 1), (1, 1), (1, 1)), "the step (3, 1) does not divide the 4 x 4 plane"),
    ((16, 4, 4, 1, 1, 3, 3, 1, 1, (1, 8), (1, 1), (1, 1)), "the step (1, 8) does not divide the 4 x 4 plane"),
    ((16, 4, 4, 1, 1, 1, 1, 0, 0, (2, 2), (1, 4), (1, 1)), "the stride (1, 4) does not divide the logical plane of 2 x 2 pixels"),
    ((64, 4, 8, 1, 1, 1, 1, 0, 0, (1, 2), (3, 1), (1, 1)), "the stride (3, 1) does not divide the logical plane of 4 x 4 pixels"),
    ((16, 4, 4, 1, 1, 3, 3, 1, 1, (1, 1), (1, 1), (4, 1)), "the offset (-4, -1) has an empty mask on the 4 x 4 plane"),
    ((16, 4, 4, 1, 1, 3, 3, 1, 1, (2, 2), (1, 1), (1, 2)), "the offset (-2, -4) has an empty mask on the 4 x 4 plane"),
    ((16, 4, 4, 1, 1, 1, 1, 0, 0, (1, 1), (0, 1), (1, 1)), "every factor at least 1"),
    ((16, 4, 4, 1, 1, 1, 1, 0, 0, (1, 1), (1, 1), (1, -2)), "every factor at least 1"),
    ((16, 4, 4, 1, 1, 3, 3, 1, 3, (2, 2), (1, 1), (1, 1)), "the anchor (1, 3) is outside the 3 x 3 kernel"),
    ((16, 3, 4, 1, 1, 1, 1, 0, 0, (1, 2), (1, 1), (1, 1)), "does not divide the row"),
])
def test_the_convolution_planner_refuses_with_the_condition_named(args, word):
    import fhe_si_amd as F
    assert LM.refused(*args) is not None and LM.refused(*args) in word
    with pytest.raises(F.FhesiError) as e:
        F.conv2d_lattice_plan(*args)
    assert word in str(e.value) and "conv2d_lattice_plan" in str(e.value), (word, str(e.value))
    with pytest.raises(F.FhesiError, match="form 3"):
        F.conv2d_lattice_plan(16, 4, 4, 1, 1, 3, 3, 1, 1, (2, 2), (2, 2), (1, 1), 3)


@pytest.mark.parametrize("args,word", [
    ((16, 4, 4, 2, 2, 3, 1, 0), "the step (3, 1) does not divide the 4 x 4 plane"),
    ((16, 4, 4, 3, 2, 1, 1, 0), "windows of 3 x 2 pixels do not tile the logical plane of 4 x 4 pixels"),
    ((16, 4, 4, 2, 4, 1, 2, 0), "windows of 2 x 4 pixels do not tile the logical plane of 4 x 2 pixels"),
    ((64, 8, 8, 16, 1, 1, 1, 0), "windows of 16 x 1 pixels do not tile the logical plane of 8 x 8 pixels"),
    ((16, 4, 4, 2, 2, 1, 1, 3), "form 3"),
    ((16, 4, 4, 2, 2, 1, 1, -1), "form -1"),
    ((64, 1, 12, 1, 3, 1, 1, 2), "does not divide the row"),
    ((64, 4, 16, 1, 3, 1, 1, 2), "windows of 1 x 3 pixels do not tile the logical plane of 4 x 16 pixels"),
    ((64, 2, 8, 1, 1, 1, 1, 2), None),
    ((16, 4, 4, 0, 2, 1, 1, 0), "every size at least 1"),
    ((16, 4, 4, 2, 2, 0, 1, 0), "every size at least 1"),
])
def test_the_pooling_planner_refuses_with_the_condition_named(args, word):
    import fhe_si_amd as F
    if word is None:
        assert F.pool2d_plan(*args) == {"form": 2, "nh": 0, "nhor": 0, "key_switches": 0, "levels": 0, "amounts": [], "out_step": (1, 1)}
        return
    assert LM.pool_refused(*args) is not None and LM.pool_refused(*args) in word
    with pytest.raises(F.FhesiError) as e:
        F.pool2d_plan(*args)
    assert word in str(e.value) and "pool2d_plan" in str(e.value), (word, str(e.value))


def test_doubling_is_refused_on_a_window_that_is_no_power_of_two():
    import fhe_si_amd as F
    assert LM.pool_refused(64, 1, 12 + 4, 1, 4, 1, 1, 2) is None
    with pytest.raises(F.FhesiError, match=r"form 2 \(doubling\) takes windows of powers of two, not 1 x 3"):
        F.pool2d_plan(64 * 3, 1, 12, 1, 3, 1, 1, 2)
    assert LM.pool_refused(64 * 3, 1, 12, 1, 3, 1, 1, 2) == "form 2 (doubling) takes windows of powers of two"
    assert F.pool2d_plan(64 * 3, 1, 12, 1, 3, 1, 1, 0)["form"] == 1


def test_lattice_columns_of_the_model():
    M = np.arange(2 * 2 * 2 * 4).reshape(2, 16) + 1
    out = LM.lattice_columns(M, 2, 4, 8, (2, 2))
    assert out.shape == (2, 64) and out[1][32 + 2 * 8 + 6] == M[1][8 + 1 * 4 + 3] and np.count_nonzero(out) == M.size
    assert np.array_equal(LM.lattice_columns(M, 2, 2, 4, (1, 1)), M)


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert int(re.search(r"#define\s+FHESI_ABI_VERSION\s+(\d+)", src).group(1)) == 9 == F.binding.ABI_VERSION
    assert hasattr(F, "conv2d_lattice_plan") and hasattr(F, "pool2d_plan")
    for name in ("conv2d", "conv2d_masks", "pool2d", "lattice_columns", "pack_images", "unpack_images"):
        assert hasattr(F.SlotSpace, name)
    for name in ("conv2d", "pool2d"):
        assert hasattr(F.SlotBasis, name)
    import inspect
    for fn in (F.SlotSpace.conv2d, F.SlotSpace.conv2d_masks, F.SlotBasis.conv2d):
        sig = inspect.signature(fn).parameters
        assert all(sig[k].default == (1, 1) for k in ("step", "stride", "dilation"))
    assert inspect.signature(F.SlotSpace.pack_images).parameters["step"].default == (1, 1)
    assert inspect.signature(F.SlotSpace.unpack_images).parameters["step"].default == (1, 1)


# ------------------------------------------------------------------------------------------------ through the scheme's model
def scheme(seed):
    m, p, logQ, g = 64, 257, 256, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, list(primes), list(roots))
    rng = R.SplitMix64(seed)
    t, pk = R.keygen(ctx, rng)
    return ctx, SM.slot_space(m, p, g), rng, t, pk, logQ


def matrices(ctx, t, rng, g, amounts):
    mats = {1: None}
    for a in set(amounts) - {0}:
        k = pow(g, a, ctx.m)
        mats[k] = HM.hoist_matrix(ctx, R.key_switch_init_automorph(ctx, t, k, rng), k)
    return mats


def test_a_strided_convolution_through_the_scheme_model():
    """(64, 257, logQ 256): 3 x 3 with stride 2 on the 4 x 4 plane, 2 -> 2 channels, the split form: every slot, the zeros off the output lattice included"""
    ctx, S, rng, t, pk, logQ = scheme(0x1A7)
    p, rows, cols = ctx.p, 2, ctx.phim // 2
    rnd = random.Random(4)
    H, W, Cin, Cout, anchor, geom = 4, 4, 2, 2, (1, 1), ((1, 1), (2, 2), (1, 1))
    K = [[[[rnd.randrange(-p, 2 * p) for _ in range(3)] for _ in range(3)] for _ in range(Cin)] for _ in range(Cout)]
    bias = [rnd.randrange(1, p) for _ in range(Cout)]
    xs = [[rnd.randrange(p) for _ in range(ctx.phim)] for _ in range(Cin)]
    cts = [R.encrypt(ctx, pk, SM.embed_slots(S, x, only_usable=False), rng) for x in xs]
    pl = LM.plan(cols, H, W, Cin, Cout, 3, 3, 1, 1, *geom, LM.SPLIT)
    mats = matrices(ctx, t, rng, S.g, pl["amounts"])
    w = LM.prepared(K, H, W, anchor, *geom, rows, cols, LM.SPLIT) % p
    bvals = LM.bias_values(bias, H, W, pl["out_step"], p, rows, cols)
    k_of = lambda a: pow(S.g, a, ctx.m)
    kb, kg = pl["amounts"][:3], pl["amounts"][3:]
    babies = [[HM.rotation(ctx, mats[k_of(a)], k_of(a), cts[J]) for a in kb] for J in range(Cin)]
    want = LM.direct(K, bias, xs, H, W, anchor, *geom, p, rows)
    sk = R.dcrt_from_poly(ctx, t)
    for I in range(Cout):
        acc = None
        for g in range(3):
            inner = None
            for J in range(Cin):
                for j in range(3):
                    term = R.ct_mul_poly(ctx, babies[J][j], SM.embed_slots(S, [int(v) for v in w[I][J][g * 3 + j]], only_usable=False))
                    inner = term if inner is None else R.ct_add(ctx, inner, term)
            rot = HM.rotation(ctx, mats[k_of(kg[g])], k_of(kg[g]), inner)
            acc = rot if acc is None else R.ct_add(ctx, acc, rot)
        acc = R.ct_add_const(ctx, acc, SM.embed_slots(S, [int(v) for v in bvals[I]], only_usable=False))
        msg, _, budget = NM.noise(ctx, sk, acc)
        print(f"stride-2 convolution, output channel {I}: {pl['key_switches']} key switches, model budget {budget} of {logQ}")
        got = SM.decode_slots(S, msg, only_usable=False)
        assert got == [int(v) for v in want[I]] and any(got) and sum(1 for v in got if v) <= ctx.phim // 4
        assert budget > 0


@pytest.mark.parametrize("form", [1, 2])
def test_a_pooling_through_the_scheme_model(form):
    """(64, 257, logQ 256): 2 x 2 windows on the step-(1, 2) lattice of the 4 x 4 plane -- no plaintext product, so the budget stays near a fresh one's"""
    ctx, S, rng, t, pk, logQ = scheme(0x900 + form)
    p, rows, cols = ctx.p, 2, ctx.phim // 2
    rnd = random.Random(form)
    H, W, kh, kw, sy, sx = 4, 4, 2, 2, 1, 2
    x = [rnd.randrange(p) for _ in range(ctx.phim)]
    ct = R.encrypt(ctx, pk, SM.embed_slots(S, x, only_usable=False), rng)
    sk = R.dcrt_from_poly(ctx, t)
    fresh = NM.noise(ctx, sk, ct)[2]
    pl = LM.pool_plan(cols, H, W, kh, kw, sy, sx, form)
    mats = matrices(ctx, t, rng, S.g, pl["amounts"])
    k_of = lambda a: pow(S.g, a, ctx.m)
    y = ct
    groups = [pl["amounts"][:pl["nhor"]], pl["amounts"][pl["nhor"]:]] if pl["form"] == 1 else [[a] for a in pl["amounts"]]
    for amounts in groups:
        rots = [HM.rotation(ctx, mats[k_of(a)], k_of(a), y) for a in amounts]      # every rotation of ONE value
        for r in rots:
            y = R.ct_add(ctx, y, r)
    msg, _, budget = NM.noise(ctx, sk, y)
    print(f"2 x 2 sum pooling, form {pl['form']}: {pl['key_switches']} key switches over {pl['levels']} levels, model budget {budget} of {logQ} (fresh {fresh})")
    assert SM.decode_slots(S, msg, only_usable=False) == [int(v) for v in LM.pool_formula(x, H, W, kh, kw, sy, sx, p, rows)]
    assert budget > 0
