#!/usr/bin/env python3
"""Matrix-vector products by T diagonals, measured: the baby-step/giant-step schedule (fhesi_ct_matvec_bsgs_dev) against the flat product
(fhesi_ct_matvec_dev, one hoisted rotation per diagonal), the only form the parent commit has.

    python3 tools/bench_bsgs.py --bsgs --out bsgs.json
    python3 tools/bench_bsgs.py --flat --tree <checkout of the parent commit, built> --out flat.json
    python3 tools/bench_bsgs.py --merge bsgs.json flat.json --out profiles/bsgs_bench.json

Workload: count in {1, 8} ciphertexts (real encryptions of random slots) x T in {16, 64, 256} random diagonals on the two-row rings
(4096, 65537, logQ 128) and (2^15, 65537, logQ 512); rotation t is k = g^t, its matrix generated on the device from a seed that depends on t
alone, so both modes hold the same keys.  --bsgs runs the planner's B at every T and every B in {2, 4, 8, 16, 32} at T = 64; it also times the
sum of G rotated ciphertexts alone (fhesi_ct_rot_sum_dev), as the kernel and as the composition the library runs under option automorph_rows,
and gives both as shares of the whole call.  --flat imports the module from --tree, so the parent's own binding and library run; at T = 256 on
the large ring the flat form's 255 derived matrices (about 106 GB with their tables) are not allocated and the record says so.  Times are host clocks around a call that
ends in a stream synchronise: one warm-up call, then the median / min / max of 5.  Both modes record the least decrypted noise budget of the
result and the bytes of the matrices the call keeps resident (rows plus derived table).  --merge puts flat over bsgs beside the ratio of the
key-switch counts, (T - 1) / (B + G - 2), and says whether the planner's B is the measured best at T = 64."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 15, 65537, 3, 512)]
COUNTS, TS, SWEEP_T, SWEEP_B = (1, 8), (16, 64, 256), 64, (2, 4, 8, 16, 32)
FLAT_KEY_LIMIT = 64 << 30          # the flat form is not set up when its matrices would take more than this
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def timed(fn, sync, warmup=1, reps=5):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def run(a):
    root = a.tree if (a.flat and a.tree) else HERE
    for d in (root, os.path.join(root, "tests"), os.path.join(root, "oracle")):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import fhesi_pyref as R
    import oracle_lib as O
    import params as P
    from slots_common import device_keys

    lines = []

    def keep(rec):
        """print the record and rewrite --out, so that a run cut short leaves what it measured"""
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)

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
        mats = {0: None}

        def matrix(e):
            """the derived matrix of g^e, made at its first use and kept"""
            if e not in mats:
                k = pow(g, e, m)
                w = F.KeySwitchMatrix(ctx, 2, nd).init_batch_seeded([one, sk1.copy().automorph(k)], sk1, logQ, SEED, PUB, 2000 + 100 * e)
                mats[e] = w.hoist(k)                              # (the source matrix is released here)
            return mats[e]

        def resident(es):
            """bytes of the distinct matrices a call reads: rows plus the derived table of the running form"""
            tot = 0
            for e in set(es) - {0}:
                form, rows, _ = mats[e].form()
                row_len = (1 << 14 if n <= (1 << 14) else n) if form == 1 else n
                tot += mats[e].nbytes + (2 * rows * 2 * 2 * nd * row_len * 8 if form > 0 else 0)
            return tot

        one_matrix = 2 * 2 * nd * len(primes) * n * 8
        rng = np.random.default_rng(m)
        cmax = max(a.count or COUNTS)
        src = ctx.alloc(cmax * words * 8)
        S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, rng.integers(0, p, size=(cmax, n)).astype(np.int64), src, nl)
        for T in (a.t or TS):
            d = rng.integers(0, p, size=(T, n)).astype(np.int64)
            for count in (a.count or COUNTS):
                out = ctx.alloc(count * words * 8)
                base = {"workload": "matvec", "m": m, "p": p, "logQ": logQ, "chain_primes": len(primes), "digits": nd, "count": count, "T": T}
                if a.flat:
                    rec = dict(base, mode="flat", key_switches=T - 1)
                    if 2 * (T - 1) * one_matrix > FLAT_KEY_LIMIT:    # (rows, and a table of about their size)
                        rec["skipped"] = "the flat form's %d derived matrices (about %.0f GB with their tables) were not allocated" % (T - 1, 2 * (T - 1) * one_matrix / 1e9)
                    else:
                        hs = [matrix(t) for t in range(T)]
                        plain = S.plain(d, False)
                        call = lambda: S.matvec(hs, range(T), plain, logQ, src, nl, count, out)
                        rec["time"] = timed(call, ctx.sync)
                        rec["matrix_bytes_resident"] = resident(range(T))
                        rec["min_noise_budget"] = int(S.noise_budget(sk1, logQ, out, nl, count).min())
                        plain.close()
                    keep(rec)
                else:
                    planned = F.matvec_bsgs_plan(T)[0]
                    for B in sorted({planned} | (set(SWEEP_B) if T == SWEEP_T else set())):
                        G = -(-T // B)
                        baby, giant = [matrix(j) for j in range(B)], [matrix(i * B) for i in range(G)]
                        plain = S.plain(S.bsgs_diagonals(d, B), False)
                        call = lambda: S.matvec_bsgs(baby, giant, B, plain, logQ, src, nl, count, out)
                        rec = dict(base, mode="bsgs", B=B, G=G, planned_B=planned, key_switches=B + G - 2)
                        rec["time"] = timed(call, ctx.sync)
                        rec["matrix_bytes_resident"] = resident(list(range(B)) + [i * B for i in range(G)])
                        rec["min_noise_budget"] = int(S.noise_budget(sk1, logQ, out, nl, count).min())
                        # the sum of G rotated ciphertexts alone: the kernel, and the composition the library runs in its place
                        pre, res = ctx.alloc(G * count * words * 8), ctx.alloc(count * words * 8)
                        for i in range(G):                        # (every term a copy of the inputs: the time does not depend on the values)
                            ctx.ct_automorph_dev(1, src, 2, nl, count, F.binding._View(pre, i * count * words * 8), nl)
                        kg = [S.rotation_k(i * B) for i in range(G)]
                        rot = lambda: ctx.ct_rot_sum_dev(kg, logQ, None, pre, count, nl, res)
                        rec["rot_sum_kernel"] = timed(rot, ctx.sync)
                        ctx.set_option("automorph_rows", 1)
                        rec["rot_sum_composed"] = timed(rot, ctx.sync)
                        ctx.set_option("automorph_rows", 0)
                        rec["rot_sum_kernel_share"] = round(rec["rot_sum_kernel"]["ms"] / rec["time"]["ms"], 4)
                        rec["rot_sum_composed_share"] = round(rec["rot_sum_composed"]["ms"] / (rec["time"]["ms"] - rec["rot_sum_kernel"]["ms"] + rec["rot_sum_composed"]["ms"]), 4)
                        rec["loadavg"] = [round(x, 2) for x in os.getloadavg()]
                        keep(rec)
                        pre.free()
                        res.free()
                        plain.close()
                out.free()
        S.close()


def merge(a):
    bsgs, flat = (json.load(open(f)) for f in a.merge)
    key = lambda r: (r["m"], r["count"], r["T"])
    by = {key(r): r for r in flat}
    rows, best = [], {}
    for r in bsgs:
        f = by.get(key(r), {})
        row = {"m": r["m"], "logQ": r["logQ"], "count": r["count"], "T": r["T"], "B": r["B"], "G": r["G"], "planned_B": r["planned_B"], "bsgs_ms": r["time"]["ms"],
               "flat_ms": f["time"]["ms"] if "time" in f else None, "flat_skipped": f.get("skipped"),
               "flat_over_bsgs": round(f["time"]["ms"] / r["time"]["ms"], 3) if "time" in f else None,
               "key_switch_ratio": round((r["T"] - 1) / max(1, r["key_switches"]), 3),
               "bsgs_matrix_bytes": r["matrix_bytes_resident"], "flat_matrix_bytes": f.get("matrix_bytes_resident"),
               "rot_sum_kernel_ms": r["rot_sum_kernel"]["ms"], "rot_sum_composed_ms": r["rot_sum_composed"]["ms"],
               "rot_sum_kernel_share": r["rot_sum_kernel_share"], "rot_sum_composed_share": r["rot_sum_composed_share"],
               "noise_budget_bsgs": r["min_noise_budget"], "noise_budget_flat": f.get("min_noise_budget")}
        rows.append(row)
        if r["T"] == SWEEP_T:
            k = (r["m"], r["count"])
            if k not in best or r["time"]["ms"] < best[k]["time"]["ms"]:
                best[k] = r
    planner = [{"m": k[0], "count": k[1], "T": SWEEP_T, "planned_B": r["planned_B"], "measured_best_B": r["B"], "planner_is_best": r["B"] == r["planned_B"]}
               for k, r in sorted(best.items())]
    with open(a.out, "w") as f:
        json.dump({"summary": rows, "planner_at_T64": planner, "bsgs": bsgs, "flat": flat}, f, indent=1)
    for row in rows + planner:
        print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsgs", action="store_true")
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--tree", help="--flat: root of a built checkout of the parent commit (its binding and library are the ones that run; default: this tree)")
    ap.add_argument("--merge", nargs=2, metavar=("BSGS", "FLAT"))
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--t", type=int, nargs="*")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge:
        merge(a)
    elif a.bsgs != a.flat:
        run(a)
    else:
        ap.error("one of --bsgs, --flat [--tree PATH], --merge A B")
