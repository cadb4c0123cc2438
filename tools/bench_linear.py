#!/usr/bin/env python3
"""Dense linear layers on packed slots, measured: fhesi_ct_linear_dev (R diagonals of length max(R, C), folds, bias) against the best form the parent
commit has -- the matrix padded to a D x D square, D = max(R, C) diagonals through fhesi_ct_matvec_bsgs_dev.

    python3 tools/bench_linear.py --layer --out layer.json
    python3 tools/bench_linear.py --padded --tree <checkout of the parent commit, built> --out padded.json
    python3 tools/bench_linear.py --merge layer.json padded.json --out profiles/linear_bench.json

Workload: count in {1, 8} ciphertexts (real encryptions of replicated random vectors) on the two-row rings (4096, 65537, logQ 128) and
(2^16, 65537, logQ 512), shapes 16 x cols, 64 x cols, cols x 16 and 64 x 64, M and b uniform in [0, p); rotation amount t is k = g^t, its matrix
generated on the device from a seed that depends on t alone, so both modes hold the same keys.  --layer records (a) the time of Linear.apply,
(b) the time to make the handle from a matrix in HBM (SlotSpace.linear(device=True)) against SlotSpace.plain(SlotSpace.bsgs_diagonals(d)) with d
the same T diagonals built in numpy on the host, and the time of linear_diag_kernel's stage alone (fhesi_linear_diagonals, download included),
(c) the least decrypted noise budget, and checks the decrypted slots against M x + b.  --padded imports the module from --tree, so the parent's own
binding and library run; where the padded form's derived matrices would take more than 64 GB they are not allocated and the record says so.
Times are host clocks around a call that ends in a stream synchronise: one warm-up call, then the median / min / max of 5.  --merge puts padded
over layer beside the ratio of the key-switch counts."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 16, 65537, 3, 512)]
COUNTS = (1, 8)
KEY_LIMIT = 64 << 30               # the padded form is not set up when its matrices would take more than this
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def shapes(cols):
    return [(16, cols), (64, cols), (cols, 16), (64, 64)]


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


class DevTensor:
    """an int64 array in HBM as SlotSpace.linear(device=True) takes it"""

    def __init__(self, ctx, a):
        self.buf, self.shape, self.dtype = ctx.upload(a), a.shape, "int64"

    def data_ptr(self):
        return self.buf.ptr.value

    def is_contiguous(self):
        return True


def run(a):
    root = a.tree if (a.padded and a.tree) else HERE
    for d in (os.path.join(HERE, "tests"), os.path.join(root, "oracle"), os.path.join(root, "tests"), root):      # (root first on the path)
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import fhesi_pyref as R
    import oracle_lib as O
    import params as P
    import linear_model as LM          # (this tree's tests/: the parent has no such model)
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
        n, nl, nd, cols = ctx.phim, (logQ + 63) // 64, R.ndigits(logQ), S.cols
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

        one_matrix = 2 * 2 * nd * len(primes) * n * 8
        cmax = max(a.count or COUNTS)
        for Rr, Cc in shapes(cols):
            rng = np.random.default_rng(m + Rr + 7 * Cc)
            M, b = rng.integers(0, p, size=(Rr, Cc)).astype(np.int64), rng.integers(0, p, size=Rr).astype(np.int64)
            x = rng.integers(0, p, size=(cmax, 2, Cc)).astype(np.int64)
            xs = np.stack([LM.replicate(x[i], Cc, 2, cols) for i in range(cmax)])
            src = ctx.alloc(cmax * words * 8)
            S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, xs, src, nl, only_usable=False)
            D, T = max(Rr, Cc), min(Rr, Cc)
            base = {"workload": "linear", "m": m, "p": p, "logQ": logQ, "chain_primes": len(primes), "digits": nd, "cols": cols, "R": Rr, "C": Cc}
            if a.padded:
                B, G = F.matvec_bsgs_plan(D)
                rec = dict(base, mode="padded", diagonals=D, B=B, G=G, key_switches=B + G - 2)
                if 2 * (B + G - 2) * one_matrix > KEY_LIMIT or D * len(primes) * n * 8 > KEY_LIMIT:
                    rec["skipped"] = "the padded form's %d derived matrices (about %.0f GB with their tables) and %d prepared diagonals (%.0f GB) were not allocated" % (
                        B + G - 2, 2 * (B + G - 2) * one_matrix / 1e9, D, D * len(primes) * n * 8 / 1e9)
                    keep(rec)
                    continue
                sq = np.zeros((D, D), dtype=np.int64)
                sq[:Rr, :Cc] = M
                t0 = time.perf_counter()
                plain = S.plain(S.bsgs_diagonals(LM.diagonals(sq, 2, cols), B), False)
                ctx.sync()
                rec["create_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                baby, giant = [matrix(j) for j in range(B)], [matrix(i * B) for i in range(G)]
                for count in (a.count or COUNTS):
                    out = ctx.alloc(count * words * 8)
                    call = lambda: S.matvec_bsgs(baby, giant, B, plain, logQ, src, nl, count, out)
                    r = dict(rec, count=count, time=timed(call, ctx.sync))
                    r["min_noise_budget"] = int(np.asarray(S.noise_budget(sk1, logQ, out, nl, count)).min())
                    got = S.decrypt_batch(sk1, logQ, out, nl, count, only_usable=False)
                    want = LM.brute(M, None, x[0], p)          # the padded product leaves (M x_r)[i] in slot (r, i), i < R
                    r["correct"] = all([int(v) for v in got[0][r0 * cols:r0 * cols + min(Rr, cols)]] == want[r0][:cols] for r0 in range(2))
                    r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
                    keep(r)
                    out.free()
                plain.close()
            else:
                pl = F.linear_plan(cols, Rr, Cc)
                rec = dict(base, mode="layer", diagonals=T, B=pl["B"], G=pl["G"], nfold=pl["nfold"], key_switches=len(pl["amounts"]))
                dM, db = DevTensor(ctx, M), DevTensor(ctx, b)
                made = []

                def create_dev():
                    made.append(S.linear(dM, db, device=True))
                    while len(made) > 1:
                        made.pop(0).close()

                def create_host_numpy():
                    S.plain(S.bsgs_diagonals(np.mod(LM.diagonals(M, 2, cols), p), pl["B"]), False).close()
                rec["create_dev"] = timed(create_dev, ctx.sync)
                rec["create_numpy_plain"] = timed(create_host_numpy, ctx.sync)
                rec["diagonals_stage_and_download"] = timed(lambda: S.linear_diagonals(M), ctx.sync)
                rec["diagonal_bytes"] = T * n * 8
                lin = made[-1]
                hs = [matrix(t) for t in lin.amounts]
                for count in (a.count or COUNTS):
                    out = ctx.alloc(count * words * 8)
                    call = lambda: lin.apply(hs, logQ, src, nl, count, out)
                    r = dict(rec, count=count, time=timed(call, ctx.sync))
                    r["min_noise_budget"] = int(np.asarray(S.noise_budget(sk1, logQ, out, nl, count)).min())
                    got = S.decrypt_batch(sk1, logQ, out, nl, count, only_usable=False)
                    r["correct"] = all([int(v) for v in got[i]] == LM.expected_slots(M, b, x[i], p, 2, cols) for i in range(count))
                    r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
                    keep(r)
                    out.free()
                lin.close()
            src.free()
        S.close()


def merge(a):
    layer, padded = (json.load(open(f)) for f in a.merge)
    key = lambda r: (r["m"], r["R"], r["C"], r.get("count"))
    by = {key(r): r for r in padded}
    rows = []
    for r in layer:
        f = by.get(key(r)) or by.get((r["m"], r["R"], r["C"], None), {})
        rows.append({"m": r["m"], "logQ": r["logQ"], "R": r["R"], "C": r["C"], "count": r["count"], "layer_ms": r["time"]["ms"],
                     "padded_ms": f["time"]["ms"] if "time" in f else None, "padded_skipped": f.get("skipped"),
                     "padded_over_layer": round(f["time"]["ms"] / r["time"]["ms"], 3) if "time" in f else None,
                     "layer_key_switches": r["key_switches"], "padded_key_switches": f.get("key_switches"),
                     "key_switch_ratio": round(f["key_switches"] / max(1, r["key_switches"]), 3) if "key_switches" in f else None,
                     "layer_diagonals": r["diagonals"], "padded_diagonals": f.get("diagonals"),
                     "create_dev_ms": r["create_dev"]["ms"], "create_numpy_plain_ms": r["create_numpy_plain"]["ms"], "padded_create_ms": f.get("create_ms"),
                     "diagonals_stage_and_download_ms": r["diagonals_stage_and_download"]["ms"],
                     "noise_budget_layer": r["min_noise_budget"], "noise_budget_padded": f.get("min_noise_budget"),
                     "correct_layer": r["correct"], "correct_padded": f.get("correct")})
    with open(a.out, "w") as f:
        json.dump({"summary": rows, "layer": layer, "padded": padded}, f, indent=1)
    for row in rows:
        print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", action="store_true")
    ap.add_argument("--padded", action="store_true")
    ap.add_argument("--tree", help="--padded: root of a built checkout of the parent commit (its binding and library are the ones that run; default: this tree)")
    ap.add_argument("--merge", nargs=2, metavar=("LAYER", "PADDED"))
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge:
        merge(a)
    elif a.layer != a.padded:
        run(a)
    else:
        ap.error("one of --layer, --padded [--tree PATH], --merge A B")
