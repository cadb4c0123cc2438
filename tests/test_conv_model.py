"""CPU: convolution layers on packed slots.  Both forms of the schedule equal the direct definition on every plane, kernel and anchor the layout admits
(different images in every block and row); the planner equals a brute-force count; fhesi_conv2d_plan equals the model, refusals included; the header
declares the entry points at ABI revision 9; one flat and one split schedule run end to end through the Python model of the scheme
(oracle/fhesi_pyref.py).  Exact."""
import os
import random
import re

import numpy as np
import pytest

import bsgs_model as BM
import conv_model as CM
import fhesi_pyref as R
import hoist_model as HM
import noise_model as NM
import params as P
import slots_pow2_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fhesi_conv2d_plan", "fhesi_conv2d_create", "fhesi_conv2d_create_dev", "fhesi_conv2d_free", "fhesi_conv2d_info", "fhesi_conv2d_masks", "fhesi_ct_conv2d_dev"]
ROWS, COLS, PRIME = 2, 16, 257
PLANES = [(4, 4), (2, 4), (4, 2), (2, 8), (1, 16), (16, 1), (2, 2), (1, 1)]


def anchors(kh, kw):
    return sorted({(0, 0), ((kh - 1) // 2, (kw - 1) // 2), (kh - 1, kw - 1)})


@pytest.mark.parametrize("H,W", PLANES)
def test_both_forms_equal_the_direct_definition(H, W):
    """rows = 2, cols = 16, kernels up to 7 x 7, up to three anchors each, (Cin, Cout) in {(1,1), (2,3)}: every admitted case through both schedules, every
    refused one refused for an empty mask"""
    rng = np.random.default_rng(100 * H + W)
    ran = 0
    for kh in range(1, 8):
        for kw in range(1, 8):
            for anchor in anchors(kh, kw):
                for Cin, Cout in ((1, 1), (2, 3)):
                    word = CM.refused(COLS, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1])
                    if word is not None:
                        assert "empty mask" in word and (kh - 1 - anchor[0] >= H or anchor[0] >= H or kw - 1 - anchor[1] >= W or anchor[1] >= W)
                        continue
                    if (kh > 3 or kw > 3) and (Cin, Cout) != (1, 1) and anchor != anchors(kh, kw)[0]:
                        continue                                  # (the large kernels with channels: one anchor)
                    K = rng.integers(-PRIME, 2 * PRIME, size=(Cout, Cin, kh, kw))
                    b = rng.integers(-PRIME, 2 * PRIME, size=Cout)
                    xs = rng.integers(0, PRIME, size=(Cin, ROWS * COLS))      # every block and row another image
                    want = CM.direct(K, b, xs, H, W, anchor, PRIME, ROWS)
                    for form in (CM.FLAT, CM.SPLIT):
                        got = CM.schedule(K, b, xs, H, W, anchor, PRIME, ROWS, form)
                        assert np.array_equal(got, want), (kh, kw, anchor, Cin, Cout, form)
                    ran += 1
    assert ran >= (1 if (H, W) == (1, 1) else 3)


def test_the_rotation_never_leaves_the_block_where_the_mask_is_one():
    for H, W in PLANES:
        P_ = H * W
        for u in range(-H + 1, H):
            for v in range(-W + 1, W):
                mu = CM.mask(u, v, H, W, 1, COLS)
                for i in range(COLS):
                    if mu[i]:
                        assert (i + u * W + v) // P_ == i // P_ and abs(u * W + v) < P_


def test_equal_amounts_are_listed_once_per_use():
    pl = CM.plan(16, 4, 4, 1, 1, 5, 1, 2, 0, CM.FLAT)
    assert pl["amounts"] == [8, 12, 0, 4, 8]
    pl = CM.plan(16, 4, 4, 1, 1, 5, 1, 2, 0, CM.SPLIT)
    assert pl["amounts"] == [0] + [8, 12, 0, 4, 8] and pl["nh"] == 6


def test_the_planner_equals_a_brute_force_count_and_the_library_equals_the_model():
    import fhe_si_amd as F
    for cols, H, W in ((16, 4, 4), (16, 2, 4), (1024, 32, 32), (1024, 2, 4), (256, 16, 16)):
        for kh in range(1, 6):
            for kw in range(1, 6):
                for ah, aw in anchors(kh, kw):
                    for Cin, Cout in ((1, 1), (2, 3), (3, 2), (4, 4), (1, 8), (8, 1)):
                        if CM.refused(cols, H, W, Cin, Cout, kh, kw, ah, aw) is not None:
                            continue
                        # brute force: the rotations each form runs on ciphertexts, the identity not counted
                        flat = Cin * sum(1 for u, v in CM.offsets(kh, kw, ah, aw) if (u, v) != (0, 0))
                        split = Cin * sum(1 for dx in range(kw) if dx != aw) + Cout * sum(1 for dy in range(kh) if dy != ah)
                        pl = CM.plan(cols, H, W, Cin, Cout, kh, kw, ah, aw)
                        assert pl["key_switches"] == min(flat, split) and pl["form"] == (CM.SPLIT if split < flat else CM.FLAT)
                        for form in (0, 1, 2):
                            got, want = F.conv2d_plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, form), CM.plan(cols, H, W, Cin, Cout, kh, kw, ah, aw, form)
                            assert got == want, (cols, H, W, Cin, Cout, kh, kw, ah, aw, form)
                            assert [i for i, a in enumerate(got["amounts"]) if a == 0] == ([ah * kw + aw] if got["form"] == 1 else [aw, kw + ah])
                            assert len(set(got["amounts"]) - {0}) <= (kh * kw - 1 if got["form"] == 1 else kh + kw - 2)
    assert F.conv2d_plan(1024, 32, 32, 1, 1, 3, 3, 1, 1)["form"] == 2 and F.conv2d_plan(1024, 32, 32, 1, 1, 1, 3, 0, 1)["form"] == 1      # a tie goes to flat
    assert F.conv2d_plan(1024, 32, 32, 1, 8, 3, 3, 1, 1) == {"form": 1, "nh": 9, "key_switches": 8, "terms": 9, "amounts": [991, 992, 993, 1023, 0, 1, 31, 32, 33]}


@pytest.mark.parametrize("args", [(16, 3, 4, 1, 1, 1, 1, 0, 0, 0), (16, 8, 4, 1, 1, 1, 1, 0, 0, 0),                    # P does not divide cols
                                  (16, 0, 4, 1, 1, 1, 1, 0, 0, 0), (16, 4, 4, 0, 1, 1, 1, 0, 0, 0), (16, 4, 4, 1, 1, 0, 3, 0, 1, 0),      # sizes below 1
                                  (16, 4, 4, 1, 1, 3, 3, 3, 1, 0), (16, 4, 4, 1, 1, 3, 3, 1, -1, 0),                  # the anchor
                                  (16, 2, 4, 1, 1, 3, 3, 0, 1, 0), (16, 4, 4, 1, 1, 1, 7, 0, 2, 0), (16, 1, 16, 1, 1, 3, 3, 1, 1, 0),      # empty masks
                                  (1024, 32, 32, 86, 86, 3, 3, 1, 1, 0), (1024, 32, 32, 65536, 1, 1, 1, 0, 0, 0),      # rows of one handle
                                  (16, 4, 4, 1, 1, 3, 3, 1, 1, 3), (16, 4, 4, 1, 1, 3, 3, 1, 1, -1),                   # the form
                                  (0, 1, 1, 1, 1, 1, 1, 0, 0, 0)])
def test_the_planner_refuses_with_the_condition_named(args):
    import fhe_si_amd as F
    word = CM.refused(*args)
    assert word is not None
    with pytest.raises(F.FhesiError) as e:
        F.conv2d_plan(*args)
    assert word in str(e.value) and "conv2d_plan" in str(e.value), (word, str(e.value))
    assert F.conv2d_plan(16, 4, 4, 1, 1, 3, 3, 1, 1)["nh"] in (6, 9)       # host only: nothing to recover from


def test_an_empty_mask_names_its_offset():
    import fhe_si_amd as F
    with pytest.raises(F.FhesiError, match=r"the offset \(2, -1\) has an empty mask on the 2 x 4 plane"):
        F.conv2d_plan(16, 2, 4, 1, 1, 3, 3, 0, 1)


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    text = open(os.path.join(ROOT, "include", "fhesi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert int(re.search(r"#define\s+FHESI_ABI_VERSION\s+(\d+)", src).group(1)) == 9 == F.binding.ABI_VERSION
    assert hasattr(F, "conv2d_plan") and hasattr(F, "Conv2d")
    for name in ("conv2d", "conv2d_masks", "pack_images", "unpack_images"):
        assert hasattr(F.SlotSpace, name)
    for name in ("conv2d", "conv2d_apply"):
        assert hasattr(F.SlotBasis, name)
    for name in ("apply", "close"):
        assert hasattr(F.Conv2d, name)


# ------------------------------------------------------------------------------------------------ through the scheme's model
def conv_ct(ctx, S, mats, K, bias, H, W, anchor, form, cts):
    """the schedule on ciphertexts of the model: hoist_model.rotation per baby and giant, Ciphertext *= ZZX per term, += per sum, += the embedded bias"""
    K = np.asarray(K, dtype=object)
    Cout, Cin, kh, kw = K.shape
    rows, cols = 2, ctx.phim // 2
    pl = CM.plan(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1], form)
    w = CM.prepared(K, H, W, anchor, rows, cols, pl["form"]) % ctx.p
    B, G = (kh * kw, 1) if pl["form"] == CM.FLAT else (kw, kh)
    kb, kg = pl["amounts"][:B], ([0] if pl["form"] == CM.FLAT else pl["amounts"][B:])
    k_of = lambda a: pow(S.g, a, ctx.m)
    babies = [[HM.rotation(ctx, mats[k_of(a)], k_of(a), cts[J]) for a in kb] for J in range(Cin)]
    out = []
    for I in range(Cout):
        acc = None
        for g in range(G):
            inner = None
            for J in range(Cin):
                for j in range(B):
                    term = R.ct_mul_poly(ctx, babies[J][j], SM.embed_slots(S, [int(v) for v in w[I][J][g * B + j]], only_usable=False))
                    inner = term if inner is None else R.ct_add(ctx, inner, term)
            rot = HM.rotation(ctx, mats[k_of(kg[g])], k_of(kg[g]), inner)
            acc = rot if acc is None else R.ct_add(ctx, acc, rot)
        if bias is not None:
            acc = R.ct_add_const(ctx, acc, SM.embed_slots(S, [int(bias[I]) % ctx.p] * ctx.phim, only_usable=False))
        out.append(acc)
    return out, pl


@pytest.mark.parametrize("form", [CM.FLAT, CM.SPLIT])
def test_schedule_through_the_scheme_model(form):
    m, p, logQ, g = 64, 257, 256, 3
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, list(primes), list(roots))
    rng = R.SplitMix64(0xC0 + form)
    t, pk = R.keygen(ctx, rng)
    S = SM.slot_space(m, p, g)
    rnd = random.Random(form)
    H, W, Cin, Cout, anchor = 2, 4, 2, 2, (1, 1)
    K = [[[[rnd.randrange(-p, 2 * p) for _ in range(3)] for _ in range(3)] for _ in range(Cin)] for _ in range(Cout)]
    bias = [rnd.randrange(-p, 2 * p) for _ in range(Cout)]
    xs = [[rnd.randrange(p) for _ in range(ctx.phim)] for _ in range(Cin)]
    cts = [R.encrypt(ctx, pk, SM.embed_slots(S, x, only_usable=False), rng) for x in xs]
    pl = CM.plan(16, H, W, Cin, Cout, 3, 3, 1, 1, form)
    mats = {1: None}
    for a in set(pl["amounts"]) - {0}:
        k = pow(g, a, m)
        mats[k] = HM.hoist_matrix(ctx, R.key_switch_init_automorph(ctx, t, k, rng), k)
    ys, pl = conv_ct(ctx, S, mats, K, bias, H, W, anchor, form, cts)
    want = CM.direct(K, bias, xs, H, W, anchor, p, 2)
    sk = R.dcrt_from_poly(ctx, t)
    for I, y in enumerate(ys):
        msg, _, budget = NM.noise(ctx, sk, y)
        print(f"form {pl['form']}, output channel {I}: {pl['key_switches']} key switches, model budget {budget} of {logQ}")
        assert SM.decode_slots(S, msg, only_usable=False) == [int(v) for v in want[I]]
        assert budget > 0
