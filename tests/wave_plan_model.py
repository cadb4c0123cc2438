"""The two pass planners that csrc/wave_plan.h replaced, restated in Python from the code as it stood before the header existed: the plan
block of fhesi_ct_plain_sum_dev (capi_ct.hip) and the group loop around the `pass` lambda of fhesi_ct_mul_sum_relin_dev (capi_pipeline.hip).
Each is transcribed statement by statement from its own C++ -- two functions that share nothing, as the originals did -- so that
tests/test_wave_plan.py compares the header with what the library used to do, not with a second spelling of itself.

Both return (passes, ix): passes as tuples (g, ng, nua, nub, nt, off, accumulate, close), ix the index words of all passes in order.  The
product planner uploaded one array per pass; here the arrays are laid end to end and `off` is where each begins.  It had no close flag either:
the key switch followed the last pass of every run of groups, which is where close is set."""


def plain_sum_plan(a_idx, b_idx, seg, ngroups, cap):
    passes, ix = [], []

    def add_pass(g, ng, t0, t1, accumulate, close):
        off = len(ix)
        slot_of = {}
        for t in range(t0, t1):
            if a_idx[t] not in slot_of:
                slot_of[a_idx[t]] = len(slot_of)
                ix.append(a_idx[t])
        nu = len(ix) - off
        for t in range(t0, t1):
            ix.append(slot_of[a_idx[t]])
        ix.extend(b_idx[t0:t1])
        if ng == 1:
            ix.extend([0, t1 - t0])
        else:
            for i in range(ng + 1):
                ix.append(seg[g + i] - seg[g])
        passes.append((g, ng, nu, 0, t1 - t0, off, accumulate, close))

    g = 0
    while g < ngroups:
        seen = set()
        g2 = g
        while g2 < ngroups and g2 - g < cap:
            grp = set()
            for t in range(seg[g2], seg[g2 + 1]):
                if a_idx[t] not in seen:
                    grp.add(a_idx[t])
            if g2 > g and len(seen) + len(grp) > cap:
                break
            seen |= grp
            g2 += 1
        if g2 - g == 1 and len(seen) > cap:
            for t0 in range(seg[g], seg[g + 1], cap):
                t1 = min(t0 + cap, seg[g + 1])
                add_pass(g, 1, t0, t1, t0 != seg[g], t1 == seg[g + 1])
        else:
            add_pass(g, g2 - g, seg[g], seg[g2], False, True)
        g = g2
    return passes, ix


def mul_sum_plan(a_idx, b_idx, seg, ngroups, chunk, ucap):
    passes, ix = [], []

    def run_pass(g, t0, t1, gseg, accumulate):
        ua, ub, ma, mb, sa, sb = [], [], {}, {}, [], []
        for t in range(t0, t1):
            if a_idx[t] not in ma:
                ma[a_idx[t]] = len(ua)
                ua.append(a_idx[t])
            if b_idx[t] not in mb:
                mb[b_idx[t]] = len(ub)
                ub.append(b_idx[t])
            sa.append(ma[a_idx[t]])
            sb.append(mb[b_idx[t]])
        passes.append([g, len(gseg) - 1, len(ua), len(ub), t1 - t0, len(ix), accumulate, False])
        ix.extend(ua + ub + sa + sb + gseg)

    g = 0
    while g < ngroups:
        seen_a, seen_b = set(), set()
        g2 = g
        while g2 < ngroups and g2 - g < chunk:
            na, nb = set(seen_a), set(seen_b)
            for t in range(seg[g2], seg[g2 + 1]):
                na.add(a_idx[t])
                nb.add(b_idx[t])
            if g2 > g and len(na) + len(nb) > ucap:
                break
            seen_a, seen_b = na, nb
            g2 += 1
        ng = g2 - g
        if ng == 1 and len(seen_a) + len(seen_b) > ucap:
            step = ucap // 2
            for t0 in range(seg[g], seg[g + 1], step):
                t1 = min(t0 + step, seg[g + 1])
                run_pass(g, t0, t1, [0, t1 - t0], t0 != seg[g])
        else:
            run_pass(g, seg[g], seg[g2], [seg[g + i] - seg[g] for i in range(ng + 1)], False)
        passes[-1][7] = True      # the key switch of groups [g, g2) came here
        g = g2
    return [tuple(p) for p in passes], ix
