#!/usr/bin/env python3
"""Weighted sums of ciphertext x plaintext-slot products, measured: fhesi_ct_plain_sum_dev on a prepared handle against the sequence of calls a
caller had to write before it existed.

    python3 tools/bench_plain.py --fused   --out fused.json
    python3 tools/bench_plain.py --compose --tree <checkout of the parent commit, built> --out compose.json
    python3 tools/bench_plain.py --merge fused.json compose.json --out profiles/plain_bench.json

Workload: out[g] = sum_{t < T} x[g T + t] (*) w[(g + t) mod 16] for 256 groups, T in {1, 4, 16}, 16 shared weights given as slot values, on the
two-row rings (4096, 65537, logQ 128) and (2^15, 65537, logQ 512); 256 T distinct ciphertexts resident in HBM (eight random ones, repeated).
--fused: one fhesi_ct_plain_sum_dev call per sum; creating the handle (embed, reduce, forward rows of the 16 weights) is timed on its own.
--compose: only entry points the parent commit has, and the module is imported from --tree, so the parent's own binding and library run: the
weights are embedded on the device and downloaded once (timed on its own, the counterpart of the handle), then per term position t one gather of
the 256 operands into a scratch batch (the copy: fhesi_ct_mul_poly_dev works in place; the first position lands in the sums directly), one fhesi_ct_mul_poly_dev over the batch with the 256
polynomials of that position, one fhesi_ct_add_dev into the sums.  That is the batched form of the composition -- 3 T calls per sum instead of
3 T per group -- and the faster one.
Times are host clocks around work that ends in a stream synchronise: median / min / max of --reps calls after --warmup calls.  Both modes
record a SHA-256 of the sums; --merge refuses files whose sums differ, and adds the ratio of the rates and the new kernel's share: of the
wall time of one profiled call (the first profiled call of a process also pays for the creation of its events) and of the time of all timed
kernel classes of that call."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 15, 65537, 3, 512)]
GROUPS, NW, TERMS, BASE = 256, 16, (1, 4, 16), 8


def median_time(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return [round(x * 1e3, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def run(a):
    root = a.tree if a.compose else HERE
    for d in (root, os.path.join(root, "tests"), os.path.join(root, "oracle")):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import params as P

    lines = []
    for m, p, g, logQ in RINGS:
        if a.m and m not in a.m:
            continue
        primes, roots = P.chain_for(m, logQ, p)
        ctx = F.Context(m, primes, roots)
        S = F.SlotSpace.pow2(ctx, p, g)
        n, nl = ctx.phim, (logQ + 63) // 64
        words = 2 * n * nl
        rng = np.random.default_rng(m)
        base = ctx.upload(P.rand_limbs(rng, (BASE, 2, n), nl, logQ))
        wvals = rng.integers(0, p, size=(NW, n)).astype(np.int64)
        for T in TERMS:
            npool = GROUPS * T
            pool = ctx.alloc(npool * words * 8)
            ctx.ct_gather_dev(base, [i % BASE for i in range(npool)], words, pool)
            a_idx = np.arange(npool, dtype=np.int32)
            b_idx = np.array([(gi + t) % NW for gi in range(GROUPS) for t in range(T)], dtype=np.int32)
            seg = np.arange(GROUPS + 1, dtype=np.int32) * T
            out = ctx.alloc(GROUPS * words * 8)
            rec = {"workload": "plain_sum", "mode": "compose" if a.compose else "fused", "m": m, "p": p, "logQ": logQ, "slots": n, "chain_primes": len(primes),
                   "groups": GROUPS, "terms": T, "weights": NW, "warmup": a.warmup, "reps": a.reps}
            if a.compose:
                polys = {}

                def prepare():
                    polys["w"] = S.embed(wvals)

                rec["prepare_ms"] = median_time(prepare, ctx.sync, 1, 3)
                tmp = ctx.alloc(GROUPS * words * 8)
                per_t = [np.ascontiguousarray(polys["w"][[b_idx[gi * T + t] for gi in range(GROUPS)]]) for t in range(T)]
                gat = [[gi * T + t for gi in range(GROUPS)] for t in range(T)]

                def call():
                    for t in range(T):
                        dst = tmp if t else out                 # the first product lands in the sums directly
                        ctx.ct_gather_dev(pool, gat[t], words, dst)
                        ctx.ct_mul_poly_dev(logQ, dst, 2, nl, GROUPS, per_t[t])
                        if t:
                            ctx.ct_add_dev(logQ, out, tmp, 2, nl, GROUPS)
            else:
                held = {}

                def prepare():
                    if "w" in held:
                        held["w"].close()
                    held["w"] = S.plain(wvals)

                rec["prepare_ms"] = median_time(prepare, ctx.sync, 1, 3)

                def call():
                    ctx.ct_plain_sum_dev(held["w"], logQ, pool, npool, nl, a_idx, b_idx, seg, out)
            rec["call_ms"] = median_time(call, ctx.sync, a.warmup, a.reps)
            rec["sums_per_s"] = round(GROUPS / (rec["call_ms"][0] * 1e-3), 1)
            rec["products_per_s"] = round(GROUPS * T / (rec["call_ms"][0] * 1e-3), 1)
            rec["sha256"] = hashlib.sha256(out.download((GROUPS, words)).tobytes()).hexdigest()
            if not a.compose:
                ctx.prof_enable(True)
                t0 = time.perf_counter()
                call()
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                prof = {k: ctx.prof_read(k) for k in F.binding.PROF_CLASSES}
                name = ctx.prof_kernel_name("plain_sum")
                ctx.prof_enable(False)
                ms = prof["plain_sum"][2]
                # 3 T rows read and 2 written per (group, prime), 8 bytes a word
                nbytes = GROUPS * len(primes) * (3 * T + 2) * n * 8
                rec["profiled"] = {"call_ms": round(wall, 3), "kernel": name, "kernel_launches": prof["plain_sum"][0], "kernel_ms": round(ms, 3),
                                   "kernel_share_of_call": round(ms / wall, 4), "class_ms": {k: round(v[2], 3) for k, v in prof.items() if v[0]},
                                   "algorithmic_bytes": nbytes, "algorithmic_GBps": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms else None, "bound": "unknown"}
                held["w"].close()
            rec["loadavg"] = [round(x, 2) for x in os.getloadavg()]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            pool.free()
            out.free()
        S.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


def merge(a):
    fused, comp = (json.load(open(f)) for f in a.merge)
    key = lambda r: (r["m"], r["terms"])
    by = {key(r): r for r in comp}
    rows = []
    for r in fused:
        c = by[key(r)]
        if c["sha256"] != r["sha256"]:
            raise SystemExit(f"sums differ at m={r['m']} T={r['terms']}")
        rows.append({"m": r["m"], "logQ": r["logQ"], "terms": r["terms"], "groups": r["groups"], "fused_sums_per_s": r["sums_per_s"], "compose_sums_per_s": c["sums_per_s"],
                     "fused_over_compose": round(r["sums_per_s"] / c["sums_per_s"], 3), "fused_prepare_ms": r["prepare_ms"][0], "compose_prepare_ms": c["prepare_ms"][0],
                     "kernel_share_of_fused_call": r["profiled"]["kernel_share_of_call"],
                     "kernel_share_of_kernel_time": round(r["profiled"]["class_ms"]["plain_sum"] / sum(r["profiled"]["class_ms"].values()), 4), "sums_equal": True})
    with open(a.out, "w") as f:
        json.dump({"summary": rows, "fused": fused, "compose": comp}, f, indent=1)
    for row in rows:
        print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--compose", action="store_true")
    ap.add_argument("--tree", help="--compose: root of a built checkout of the parent commit (its binding and library are the ones that run)")
    ap.add_argument("--merge", nargs=2, metavar=("FUSED", "COMPOSE"))
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge:
        merge(a)
    elif a.fused != a.compose and (a.tree or not a.compose):
        run(a)
    else:
        ap.error("one of --fused, --compose --tree PATH, --merge A B")
