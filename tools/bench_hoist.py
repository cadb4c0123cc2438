#!/usr/bin/env python3
"""T rotations of the same ciphertexts, measured: fhesi_ct_rotations_dev on derived matrices against T calls of
fhesi_ct_automorph_key_switch_dev, the only form the parent commit has.

    python3 tools/bench_hoist.py --hoisted --out hoisted.json
    python3 tools/bench_hoist.py --compose --tree <checkout of the parent commit, built> --out compose.json
    python3 tools/bench_hoist.py --merge hoisted.json compose.json --out profiles/hoist_bench.json

Workload: count in {1, 8, 64} ciphertexts (real encryptions of random slots) x T in {1, 4, 16, 32} rotations k = g^1 .. g^T on the two-row rings
(4096, 65537, logQ 128) and (2^15, 65537, logQ 512), the shapes of tools/bench_plain.py; T matrices generated on the device from seeds, the
same seeds in both modes.  --hoisted: one call per measurement, with option hoist_dot = 1 (one dot launch per matrix), 2 (the multi-matrix
kernel, where the form admits it) and 0 (automatic).  --compose: the module is imported from --tree, so the parent's own binding and library run.
Times are host clocks around work that ends in a stream synchronise, in --blocks blocks of --reps calls after --warmup calls: the median of
each block is kept, and the spread of a measurement is the distance between its slowest and its fastest block.  Both modes record the least
decrypted noise budget over all outputs.  --merge adds, per point, hoisted over compose (median of block medians), whether the margin exceeds
the parent's own spread, which of the options 1 and 2 the automatic choice took (by the dot kernel it ran) and whether that one is the faster
of the two (not behind the other by more than their spread)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 15, 65537, 3, 512)]
COUNTS, TS = (1, 8, 64), (1, 4, 16, 32)
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def blocks_of(fn, sync, warmup, reps, blocks):
    for _ in range(warmup):
        fn()
    sync()
    meds = []
    for _ in range(blocks):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        meds.append(round(statistics.median(ts) * 1e3, 4))
    return {"block_ms": meds, "ms": round(statistics.median(meds), 4), "spread_ms": round(max(meds) - min(meds), 4)}


def run(a):
    root = a.tree if a.compose else HERE
    for d in (root, os.path.join(root, "tests"), os.path.join(root, "oracle")):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import fhesi_pyref as R
    import oracle_lib as O
    import params as P
    from slots_common import device_keys

    lines = []
    for m, p, g, logQ in RINGS:
        if a.m and m not in a.m:
            continue
        primes, roots = P.chain_for(m, logQ, p)
        ctx = F.Context(m, primes, roots)
        S = F.SlotSpace.pow2(ctx, p, g)
        n, nl, nd = ctx.phim, (logQ + 63) // 64, R.ndigits(logQ)
        words = 2 * n * nl
        sk1, pk0, pk1 = device_keys(ctx, logQ, SEED)
        one = F.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
        counts, ts = tuple(a.count or COUNTS), tuple(a.t or TS)
        tmax = max(ts)
        ks = [pow(g, t + 1, m) for t in range(tmax)]
        mats, extra = [], {}
        for i, k in enumerate(ks):
            w = F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(k)], sk1, logQ, SEED, PUB, 2000 + 100 * i)
            mats.append(w if a.compose else w.hoist(k))          # (the source matrix of a derived one is released here)
        rng = np.random.default_rng(m)
        cmax = max(counts)
        src = ctx.alloc(cmax * words * 8)
        S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, rng.integers(0, p, size=(cmax, n)).astype(np.int64), src, nl)
        for count in counts:
            for T in ts:
                out = ctx.alloc(T * count * words * 8)
                rec = {"workload": "rotations", "mode": "compose" if a.compose else "hoisted", "m": m, "p": p, "logQ": logQ, "chain_primes": len(primes), "digits": nd,
                       "count": count, "T": T, "warmup": a.warmup, "reps": a.reps, "blocks": a.blocks}
                if a.compose:
                    def call():
                        for t in range(T):
                            ctx.ct_automorph_key_switch_dev(mats[t], logQ, ks[t], src, nl, count, F.binding._View(out, t * count * words * 8), nl)
                    rec["time"] = blocks_of(call, ctx.sync, a.warmup, a.reps, a.blocks)
                else:
                    def call():
                        ctx.ct_rotations_dev(mats[:T], ks[:T], logQ, src, nl, count, out, nl)
                    call()
                    form, rows, limb_bits = mats[0].form()
                    rec["form"] = [form, rows, limb_bits]
                    row_len = (1 << 14 if n <= (1 << 14) else n) if form == 1 else n
                    table = 2 * rows * 2 * 2 * nd * row_len * 8 if form else 0
                    rec["matrix_bytes"], rec["table_bytes"] = mats[0].nbytes, table
                    for how in (1, 2, 0):
                        if how == 2 and form != 1:
                            continue
                        ctx.set_option("hoist_dot", how)
                        rec["time_hoist_dot_%d" % how] = blocks_of(call, ctx.sync, a.warmup, a.reps, a.blocks)
                        ctx.prof_enable(True)                       # which dot kernel this option ran (the last launch of the call)
                        call()
                        ctx.sync()
                        rec["dot_kernel_%d" % how] = ctx.prof_kernel_name("dot")
                        ctx.prof_enable(False)
                    ctx.set_option("hoist_dot", 0)
                    call()
                rec["min_noise_budget"] = int(S.noise_budget(sk1, logQ, out, nl, T * count).min())
                rec["loadavg"] = [round(x, 2) for x in os.getloadavg()]
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                out.free()
        S.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


def merge(a):
    hoisted, comp = (json.load(open(f)) for f in a.merge)
    key = lambda r: (r["m"], r["count"], r["T"])
    by = {key(r): r for r in comp}
    rows = []
    for r in hoisted:
        c = by[key(r)]["time"]
        auto, one = r["time_hoist_dot_0"], r["time_hoist_dot_1"]
        two = r.get("time_hoist_dot_2")
        # the option the automatic choice took, by the kernel it ran; it is the faster one when the other is not ahead of it by more than their spread
        took = 2 if two and r["dot_kernel_0"] == r["dot_kernel_2"] and r["dot_kernel_0"] != r["dot_kernel_1"] else 1
        mine, other = (two, one) if took == 2 else (one, two)
        rows.append({"m": r["m"], "logQ": r["logQ"], "count": r["count"], "T": r["T"], "compose_ms": c["ms"], "compose_spread_ms": c["spread_ms"],
                     "hoist_dot_1_ms": one["ms"], "hoist_dot_2_ms": two["ms"] if two else None, "auto_ms": auto["ms"], "auto_spread_ms": auto["spread_ms"],
                     "compose_over_auto": round(c["ms"] / auto["ms"], 3), "margin_ms": round(c["ms"] - auto["ms"], 4),
                     "faster_beyond_parent_spread": c["ms"] - auto["ms"] > c["spread_ms"],
                     "auto_took": took, "auto_is_the_faster_choice": other is None or mine["ms"] <= other["ms"] + max(mine["spread_ms"], other["spread_ms"]),
                     "noise_budget_hoisted": r["min_noise_budget"], "noise_budget_compose": by[key(r)]["min_noise_budget"],
                     "derived_matrix_bytes": r["matrix_bytes"] + r["table_bytes"]})
    with open(a.out, "w") as f:
        json.dump({"summary": rows, "hoisted": hoisted, "compose": comp}, f, indent=1)
    for row in rows:
        print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hoisted", action="store_true")
    ap.add_argument("--compose", action="store_true")
    ap.add_argument("--tree", help="--compose: root of a built checkout of the parent commit (its binding and library are the ones that run)")
    ap.add_argument("--merge", nargs=2, metavar=("HOISTED", "COMPOSE"))
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--t", type=int, nargs="*")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge:
        merge(a)
    elif a.hoisted != a.compose and (a.tree or not a.compose):
        run(a)
    else:
        ap.error("one of --hoisted, --compose --tree PATH, --merge A B")
