#!/usr/bin/env python3
"""The noise budget next to a plain decryption, measured.

    python3 tools/bench_noise.py --parent-tree <checkout of the parent commit, built> --out profiles/noise_bench.json

256 two-part ciphertexts resident in HBM (eight random ones, repeated) on the two-row rings (4096, 65537, logQ 128) and (2^15, 65537, logQ 512):
fhesi_decrypt_batch with the parent commit's own binding and library and with this tree's, fhesi_decrypt_noise_batch (message and residual from
one pass over z) and fhesi_ct_noise_batch (the residual only) on this tree.  Every figure is the median / min / max of --reps calls after
--warmup calls, host clocks around calls that end in a stream synchronise.  The trees run in fresh processes, parent / this tree / parent /
this tree, so that a drift of the box shows as a difference between the two runs of one tree; the ratios are taken against the mean of the
parent's two medians of fhesi_decrypt_batch.  The messages of the three calls are compared by SHA-256 across processes.
No kernel trace or counter pass is taken here: the roofline entry stays `bound: "unknown"`."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 128), (1 << 15, 65537, 512)]
COUNT, BASE = 256, 8


def median_time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                   # (every entry point measured here ends in a stream synchronise)
        ts.append(time.perf_counter() - t0)
    return [round(x * 1e3, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def worker(a):
    for d in (a.tree, os.path.join(a.tree, "tests"), os.path.join(a.tree, "oracle")):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import params as P

    out = []
    for m, p, logQ in RINGS:
        primes, roots = P.chain_for(m, logQ, p)
        ctx = F.Context(m, primes, roots)
        n, nl = ctx.phim, (logQ + 63) // 64
        words = 2 * n * nl
        rng = np.random.default_rng(m)
        base = ctx.upload(P.rand_limbs(rng, (BASE, 2, n), nl, logQ))
        cts = ctx.alloc(COUNT * words * 8)
        ctx.ct_gather_dev(base, [i % BASE for i in range(COUNT)], words, cts)
        sk1 = F.DoubleCRT(ctx).sample(0, 64, 11, 7)
        sha = lambda msg: hashlib.sha256(np.ascontiguousarray(msg).tobytes()).hexdigest()
        rec = {"m": m, "p": p, "logQ": logQ, "phim": n, "chain_primes": len(primes), "ciphertexts": COUNT, "warmup": a.warmup, "reps": a.reps,
               "loadavg": round(os.getloadavg()[0], 1)}
        rec["decrypt_batch_ms"] = median_time(lambda: ctx.decrypt_batch(sk1, logQ, p, cts, nl, COUNT), a.warmup, a.reps)
        rec["msg_sha256"] = sha(ctx.decrypt_batch(sk1, logQ, p, cts, nl, COUNT))
        if hasattr(ctx, "noise_budget"):
            rec["decrypt_noise_batch_ms"] = median_time(lambda: ctx.decrypt_noise_batch(sk1, logQ, p, cts, nl, COUNT), a.warmup, a.reps)
            rec["ct_noise_batch_ms"] = median_time(lambda: ctx.noise_budget(sk1, logQ, p, cts, nl, COUNT), a.warmup, a.reps)
            msg, budget = ctx.decrypt_noise_batch(sk1, logQ, p, cts, nl, COUNT)
            rec["noise_msg_sha256"] = sha(msg)
            rec["budgets_of_the_eight"] = [int(b) for b in budget[:BASE]]
        out.append(rec)
    print("BENCH_NOISE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    runs = []
    for label, tree in [("parent", a.parent_tree), ("this", HERE)] * 2:
        if tree is None:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--warmup", str(a.warmup), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"{label} worker failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_NOISE ")][-1]
        runs.append({"tree": label, "rings": json.loads(line[len("BENCH_NOISE "):])})
    rings = []
    for i, (m, p, logQ) in enumerate(RINGS):
        par = [r["rings"][i] for r in runs if r["tree"] == "parent"]
        own = [r["rings"][i] for r in runs if r["tree"] == "this"]
        if len({r["msg_sha256"] for r in par + own} | {r["noise_msg_sha256"] for r in own}) != 1:
            sys.exit(f"m={m}: the messages differ between the calls or the trees")
        rec = {"workload": "noise", "m": m, "p": p, "logQ": logQ, "ciphertexts": COUNT, "bound": "unknown",
               "this_decrypt_batch_ms": [r["decrypt_batch_ms"] for r in own], "decrypt_noise_batch_ms": [r["decrypt_noise_batch_ms"] for r in own],
               "ct_noise_batch_ms": [r["ct_noise_batch_ms"] for r in own], "budgets_of_the_eight": own[0]["budgets_of_the_eight"], "messages_equal": True,
               "loadavg": [r["loadavg"] for r in par + own]}
        if par:
            ref = statistics.mean(r["decrypt_batch_ms"][0] for r in par)
            med = lambda key: statistics.mean(r[key][0] for r in own)
            rec["parent_decrypt_batch_ms"] = [r["decrypt_batch_ms"] for r in par]
            rec["ratio_to_parent_decrypt_batch"] = {"decrypt_batch": round(med("decrypt_batch_ms") / ref, 4), "decrypt_noise_batch": round(med("decrypt_noise_batch_ms") / ref, 4),
                                                    "ct_noise_batch": round(med("ct_noise_batch_ms") / ref, 4)}
        rings.append(rec)
    text = json.dumps(rings, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
