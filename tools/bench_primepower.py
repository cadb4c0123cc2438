#!/usr/bin/env python3
"""The metric's multiplication (ciphertext mult + relinearize, logQ = 512, generated key-switch matrix) on a prime-power ring: m = p - 1 = 2 3^9
for p = 39367, phi(m) = 13122 -- padded rows of 2^15, the same row length as `bench.py --workload refring` at p = 32603 -- on the fused 30-bit
paths (strided fold) and on per-prime rows (ks_direct = 1, tensor32 = 0: the only path these rings had before), in the same process.

    python3 tools/bench_primepower.py [--p 39367] [--batch 1024] [--small-batch 8] [--steps 5] [--warmup 2] [--out profiles/primepower_bench.json]

Operands are `--uniq` distinct random ciphertext pairs repeated to fill the batch, as bench.py fills its batches.  Times are host clocks around
calls that end in a stream synchronise; each figure is the median of --steps calls after --warmup calls.  The first --small-batch outputs of
the two paths are compared word for word.  One JSON line on stdout; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, d)

import numpy as np  # noqa: E402

import fhe_si_amd as F  # noqa: E402
import fhesi_pyref as R  # noqa: E402
import params as P  # noqa: E402


def timed(fn, sync, warmup, steps):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=39367)
    ap.add_argument("--logQ", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--small-batch", type=int, default=8)
    ap.add_argument("--uniq", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, p, logQ = a.p - 1, a.p, a.logQ
    off, st, lg = F.lin_class(m)
    if st < 2:
        raise SystemExit(f"--p {p}: m = {m} is not q^k or 2 q^k with k >= 2")
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    one = np.zeros((n, 1), dtype=np.uint64)
    one[0, 0] = 1
    t = F.DoubleCRT(ctx).sample(0, 64, 77, 1)
    t2 = t.copy()
    t2.op(t, 2)
    ksk = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([F.DoubleCRT.from_poly(ctx, one), t, t2], t, logQ, 77, 78, 100, 3)
    rng = np.random.default_rng(m)
    ua, ub = P.rand_limbs(rng, (a.uniq, 2, n), nl, logQ), P.rand_limbs(rng, (a.uniq, 2, n), nl, logQ)
    B, Bs = a.batch, min(a.small_batch, a.batch)
    rep = lambda u, c: np.concatenate([u] * (-(-c // a.uniq)))[:c]
    da, db, dout = ctx.upload(rep(ua, B)), ctx.upload(rep(ub, B)), ctx.alloc(B * 2 * n * nl * 8)
    fused = timed(lambda: ctx.ct_mul_relin_dev(ksk, logQ, p, da, db, dout, nl, B, 3), ctx.sync, a.warmup, a.steps)
    form, rows, bits = ksk.form()
    fused_small = timed(lambda: ctx.ct_mul_relin_dev(ksk, logQ, p, da, db, dout, nl, Bs, 3), ctx.sync, a.warmup, a.steps)
    first = dout.download((Bs, 2, n, nl))
    ctx.set_option("ks_direct", 1)
    ctx.set_option("tensor32", 0)
    ksk_d = F.KeySwitchMatrix(ctx, 3, nd).upload(ksk.download())
    dref = ctx.alloc(Bs * 2 * n * nl * 8)
    direct = timed(lambda: ctx.ct_mul_relin_dev(ksk_d, logQ, p, da, db, dref, nl, Bs, 3), ctx.sync, 1, max(1, min(a.steps, 3)))
    same = bool(np.array_equal(dref.download((Bs, 2, n, nl)), first))
    line = json.dumps({
        "workload": "primepower", "p": p, "m": m, "phim": n, "fold_offset": off, "fold_stride": st, "row_log2": lg, "logQ": logQ, "chain_primes": len(primes),
        "ndigits": nd, "keys": "generated", "key_switch_form": {"form": form, "rows": rows, "limb_bits": bits, "centred_limbs": ksk.key_bits()[0]},
        "batch": B, "small_batch": Bs, "steps": a.steps, "warmup": a.warmup,
        "fused_mults_per_s": round(B / fused[0], 2), "fused_ms_per_step": [round(x * 1e3, 3) for x in fused],
        "fused_small_batch_mults_per_s": round(Bs / fused_small[0], 2),
        "per_prime_mults_per_s": round(Bs / direct[0], 2), "per_prime_ms_per_step": [round(x * 1e3, 3) for x in direct], "per_prime_form": ksk_d.form()[0],
        "fused_over_per_prime": round((B / fused[0]) / (Bs / direct[0]), 1), "paths_agree": same,
        "loadavg": [round(x, 2) for x in os.getloadavg()],
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same or form != 1:
        raise SystemExit("the fused path did not run, or the two paths disagree")


if __name__ == "__main__":
    main()
