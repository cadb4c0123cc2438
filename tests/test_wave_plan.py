"""CPU (no GPU): the pass planner of the sum waves (fhe-si_amd/csrc/wave_plan.h, the one both fhesi_ct_plain_sum_dev and
fhesi_ct_mul_sum_relin_dev call) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_wave_plan.cpp),
word for word against the two planners it replaced (wave_plan_model.py), and against properties that need no model: every term in exactly one
pass, local slots inside the pass's own distinct list, segment bounds non-decreasing and ending at the pass's term count.

Plaintext mode: both caps are `cap`, distinct operands are the a's, a group over the cap goes in pieces of `cap` terms.  Product mode: the
group cap and the operand cap are separate, a's and b's count apart (the same index on both sides counts twice), pieces of cap / 2 terms."""
import os
import random
import subprocess

import pytest

import wave_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def case(b_op, max_groups, max_operands, groups):
    """groups: list of lists of (a, b) terms"""
    seg, a, b = [0], [], []
    for g in groups:
        a += [t[0] for t in g]
        b += [t[1] for t in g]
        seg.append(len(a))
    return dict(b_op=b_op, max_groups=max_groups, max_operands=max_operands, seg=seg, a=a, b=b, ng=len(groups))


def fixed_cases():
    out = {}
    for b_op in (0, 1):
        out[f"one_term_{b_op}"] = case(b_op, 4, 4, [[(3, 1)]])
        shared = [[(0, 1), (2, 3)], [(2, 3), (0, 1)]]
        out[f"shared_operands_{b_op}"] = case(b_op, 8, 8, shared)
    out["one_group_a_pass_1"] = case(1, 1, 8, shared + [[(1, 1)]])
    out["one_group_a_pass_0"] = case(0, 1, 1, [[(0, 0)], [(0, 1), (0, 2)], [(1, 1)]])
    # two groups of two distinct operands each (four a's; two a's and two b's apart): one below what both need splits between them
    out["operand_cap_splits_0"] = case(0, 3, 3, [[(0, 0), (1, 0)], [(2, 0), (3, 0)]])
    out["operand_cap_splits_1"] = case(1, 4, 7, [[(0, 0), (1, 1)], [(2, 2), (3, 3)]])
    big = [(i % 5, (i + 1) % 5) for i in range(7)]
    out["over_cap_product_step1"] = case(1, 4, 2, [big])
    out["over_cap_plain_step1"] = case(0, 1, 1, [big])
    out["over_cap_between_others_0"] = case(0, 2, 2, [[(0, 0)], big, [(1, 1)]])
    out["over_cap_between_others_1"] = case(1, 4, 4, [[(0, 0)], big, [(1, 1)]])
    out["empty_first"] = case(0, 4, 4, [[], [(0, 0), (1, 1)]])
    out["empty_last"] = case(0, 4, 4, [[(0, 0), (1, 1)], []])
    out["empty_alone"] = case(0, 4, 4, [[]])
    out["empty_each_a_pass"] = case(0, 1, 1, [[], [], [(2, 2)]])
    out["same_index_both_sides"] = case(1, 4, 2, [[(3, 3)], [(3, 3)]])             # {3} + {3} = 2 operands: both groups fit one pass
    out["same_index_both_sides_over"] = case(1, 4, 3, [[(3, 3), (4, 4)]])          # {3, 4} + {3, 4} = 4 > 3: piecewise, step 1
    return out


def random_cases(n=400, seed=20261019):
    rng = random.Random(seed)
    out = {}
    for i in range(n):
        b_op = i % 2
        ng = rng.randint(1, 6)
        lo = 1 if b_op else 0                      # the product wave refuses empty groups before it plans
        groups = [[(rng.randrange(5), rng.randrange(5)) for _ in range(rng.randint(lo, 8))] for _ in range(ng)]
        cap = rng.randint(2 if b_op else 1, 10)
        out[f"random_{i}"] = case(b_op, rng.randint(1, 6) if b_op else cap, cap, groups)
    return out


def model(c):
    if c["b_op"]:
        return M.mul_sum_plan(c["a"], c["b"], c["seg"], c["ng"], c["max_groups"], c["max_operands"])
    assert c["max_groups"] == c["max_operands"]      # the plaintext sum has ONE cap: its planner is compared where the two agree
    return M.plain_sum_plan(c["a"], c["b"], c["seg"], c["ng"], c["max_operands"])


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """every case through the program once: name -> (case, passes, ix)"""
    subprocess.check_call(["make", "-C", HOST, "test_wave_plan"], stdout=subprocess.DEVNULL)
    cs = {**fixed_cases(), **random_cases()}
    path = tmp_path_factory.mktemp("wave_plan") / "cases.txt"
    path.write_text("".join(" ".join(map(str, [c["b_op"], c["max_groups"], c["max_operands"], c["ng"]] + c["seg"] + c["a"] + c["b"])) + "\n" for c in cs.values()))
    r = subprocess.run([os.path.join(HOST, "test_wave_plan"), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    lines = iter(r.stdout.split("\n"))
    got = {}
    for name, c in cs.items():
        head = next(lines).split()
        assert head[0] == "passes"
        passes = []
        for _ in range(int(head[1])):
            v = [int(x) for x in next(lines).split()]
            passes.append(tuple(v[:6]) + (bool(v[6]), bool(v[7])))
        ix = next(lines).split()
        assert ix[0] == "ix"
        got[name] = (c, passes, [int(x) for x in ix[1:]])
    return got


def test_same_passes_and_words_as_the_planners_it_replaced(planned):
    assert len(planned) >= 300
    wrong = [(name, model(c), (passes, ix)) for name, (c, passes, ix) in planned.items() if model(c) != (passes, ix)]
    assert not wrong, wrong[:3]
    assert {c["b_op"] for c, _, _ in planned.values()} == {0, 1}
    # the random cases reach every branch: several groups in a pass, a split between groups, a piecewise group
    for b_op in (0, 1):
        mine = [(p, c) for c, p, _ in planned.values() if c["b_op"] == b_op]
        assert any(q[1] > 1 for p, _ in mine for q in p) and any(q[6] for p, _ in mine for q in p) and any(len(p) > 1 and not any(q[6] for q in p) for p, _ in mine)


def test_every_term_in_one_pass_slots_and_bounds_in_range(planned):
    for name, (c, passes, ix) in planned.items():
        seg, a, b, b_op = c["seg"], c["a"], c["b"], c["b_op"]
        covered, at, next_g = [], 0, 0
        for (g, ng, nua, nub, nt, off, accumulate, close) in passes:
            assert off == at and ng >= 1 and ng <= c["max_groups"], name
            assert nub == 0 or b_op, name
            ua, ub = ix[off:off + nua], ix[off + nua:off + nua + nub]
            sa = ix[off + nua + nub:off + nua + nub + nt]
            sb = ix[off + nua + nub + nt:off + nua + nub + 2 * nt]
            bounds = ix[off + nua + nub + 2 * nt:off + nua + nub + 2 * nt + ng + 1]
            at = off + nua + nub + 2 * nt + ng + 1
            assert len(set(ua)) == nua and len(set(ub)) == nub, name
            assert all(0 <= s < nua for s in sa), name
            assert all(0 <= s < nub for s in sb) if b_op else True, name
            assert len(bounds) == ng + 1 and bounds[0] == 0 and bounds[-1] == nt and all(x <= y for x, y in zip(bounds, bounds[1:])), name
            # which terms: a whole run of groups, or the next piece of one group
            if accumulate:
                assert g == next_g - 1 and ng == 1, name
                t0 = covered[-1] + 1
            else:
                assert g == next_g, name
                t0 = seg[g]
                next_g = g + ng
            terms = list(range(t0, t0 + nt))
            assert close == (t0 + nt == seg[g + ng]), name
            if ng > 1:
                assert bounds == [seg[g + i] - seg[g] for i in range(ng + 1)], name
            assert [ua[s] for s in sa] == [a[t] for t in terms], name
            assert ([ub[s] for s in sb] if b_op else sb) == [b[t] for t in terms], name
            # the operand cap holds for every pass: a group that alone exceeds it went in pieces
            assert nua + nub <= c["max_operands"], name
            covered += terms
        assert at == len(ix) and next_g == c["ng"], name
        assert covered == list(range(seg[-1])), name


def test_flags_of_a_piecewise_group(planned):
    for name, step in (("over_cap_product_step1", 1), ("over_cap_plain_step1", 1)):
        c, passes, ix = planned[name]
        assert len(passes) == 7 and all(p[0] == 0 and p[1] == 1 and p[4] == step for p in passes)
        assert [p[6] for p in passes] == [False] + [True] * 6           # accumulate: every piece but the first
        assert [p[7] for p in passes] == [False] * 6 + [True]           # close: the last piece only
    c, passes, ix = planned["over_cap_between_others_1"]                # cap 4: pieces of 2 terms, 7 terms = 4 pieces, between two whole groups
    assert [(p[0], p[4], p[6], p[7]) for p in passes] == [(0, 1, False, True), (1, 2, False, False), (1, 2, True, False), (1, 2, True, False), (1, 1, True, True), (2, 1, False, True)]


def test_fixed_cases_split_where_stated(planned):
    assert [p[:2] for p in planned["one_group_a_pass_1"][1]] == [(0, 1), (1, 1), (2, 1)]
    assert [p[:2] for p in planned["one_group_a_pass_0"][1]] == [(0, 1), (1, 1), (2, 1)]
    assert [p[:2] for p in planned["empty_each_a_pass"][1]] == [(0, 1), (1, 1), (2, 1)]
    assert [p[:2] for p in planned["operand_cap_splits_0"][1]] == [(0, 1), (1, 1)]
    assert [p[:2] for p in planned["operand_cap_splits_1"][1]] == [(0, 1), (1, 1)]
    assert [p[:5] for p in planned["shared_operands_1"][1]] == [(0, 2, 2, 2, 4)]
    assert [p[:5] for p in planned["shared_operands_0"][1]] == [(0, 2, 2, 0, 4)]
    assert [p[:5] for p in planned["same_index_both_sides"][1]] == [(0, 2, 1, 1, 2)]
    assert [p[:5] for p in planned["same_index_both_sides_over"][1]] == [(0, 1, 1, 1, 1), (0, 1, 1, 1, 1)]
    assert [p[:5] for p in planned["empty_alone"][1]] == [(0, 1, 0, 0, 0)] and planned["empty_alone"][2] == [0, 0]
    assert [p[:5] for p in planned["empty_first"][1]] == [(0, 2, 2, 0, 2)] and planned["empty_first"][2][-3:] == [0, 0, 2]
    assert [p[:5] for p in planned["empty_last"][1]] == [(0, 2, 2, 0, 2)] and planned["empty_last"][2][-3:] == [0, 2, 2]
