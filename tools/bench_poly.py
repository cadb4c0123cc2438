#!/usr/bin/env python3
"""Polynomial activations on packed slots, measured: fhesi_ct_poly_eval_dev against the two forms a caller of the parent commit has.

    python3 tools/bench_poly.py --tree <checkout of the parent commit, built> --out profiles/poly_bench.json

Workload: count in {1, 8, 64} ciphertexts (real encryptions of random slot values) on (4096, 65537, logQ 128) and (2^15, 65537, logQ 512), dense
polynomials of degree 3, 7, 15, 31 with coefficients uniform in [1, p), the planner's B.  Three forms, timed alternately in one process (one warm-up of
each, then 5 rounds of new, Horner, composed; median / min / max of the 5):
  new       Context.ct_poly_eval_dev of this tree;
  horner    y = c_d x + c_(d-1), then y = y x + c_k: d - 1 dependent fhesi_ct_mul_relin_batch_dev, with copy + fhesi_ct_mul_long_dev and
            fhesi_ct_add_const_dev for the scalars -- through the package imported from --tree under another name: the parent's own binding and library,
            on a context of its own with the same keys (without --tree: this tree's, and the record says so);
  composed  the same Paterson-Stockmeyer schedule (tests/poly_model.py) from the parent's public calls: fhesi_ct_mul_relin_batch_dev per product, one
            per outer term included, with fhesi_ct_add_dev between; copy + fhesi_ct_mul_long_dev + fhesi_ct_add_dev per scalar term.
Each ratio stands beside the key-switch counts it should follow, and counts only where it exceeds the baseline's spread (max - min of its timed calls
over its median).  Also: ct_lin_comb_kernel's call alone against its three-pass composition at 1 / 4 / 16 terms, and the least decrypted noise budget of
the new call and of Horner.  Times are host clocks around a call that ends in a stream synchronise."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 15, 65537, 3, 512)]
DEGREES = (3, 7, 15, 31)
COUNTS = (1, 8, 64)
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def load_parent(tree):
    """the package of another checkout under another name: its binding loads its own library"""
    d = os.path.join(tree, "fhe-si_amd")
    spec = importlib.util.spec_from_file_location("fhe_si_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fhe_si_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def alternately(forms, warmup=1, reps=5):
    """forms {name: (call, sync)} -> {name: {ms, min_ms, max_ms, spread}}"""
    ts = {k: [] for k in forms}
    for r in range(warmup + reps):
        for k, (fn, sync) in forms.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for k, v in ts.items()}


def main(a):
    for d in (os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), HERE):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import fhesi_pyref as R
    import oracle_lib as O
    import params as P
    import poly_model as PM

    FP = load_parent(a.tree) if a.tree else F
    lines = []

    def keep(rec):
        """print the record and rewrite --out, so that a run cut short leaves what it measured"""
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)

    def keys(FX, ctx, logQ):
        """t = sampleHWt(64), pk = (e + t c1, -c1), the s^2 -> s matrix: all on the device, from seeds -- the same keys on either library"""
        n, nl = ctx.phim, (logQ + 63) // 64
        sk1 = FX.DoubleCRT(ctx).sample(0, 64, SEED, 7)
        c1 = FX.DoubleCRT.from_poly(ctx, P.rand_limbs(np.random.default_rng(SEED), (n,), nl, logQ))
        pk0 = sk1.copy().op(c1, FX.OP_MUL).op(FX.DoubleCRT(ctx).sample(1, 0, SEED, 9), FX.OP_ADD)
        pk1 = FX.DoubleCRT.from_poly(ctx, O.ints_to_limbs([0] * n, 1)).op(c1, FX.OP_SUB)
        one = FX.DoubleCRT.from_poly(ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
        ksk = FX.KeySwitchMatrix(ctx, 3, R.ndigits(logQ)).init_batch_seeded([one, sk1, sk1.copy().op(sk1, FX.OP_MUL)], sk1, logQ, SEED, PUB, 1000)
        return sk1, pk0, pk1, ksk

    for m, p, g, logQ in RINGS:
        if a.m and m not in a.m:
            continue
        primes, roots = P.chain_for(m, logQ, p)
        n, nl = R.zms_idx(m)[1], (logQ + 63) // 64
        ctb = 2 * n * nl * 8
        ctx, ctxP = F.Context(m, primes, roots), FP.Context(m, primes, roots)
        S, SP = F.SlotSpace.pow2(ctx, p, g), FP.SlotSpace.pow2(ctxP, p, g)
        sk1, pk0, pk1, ksk = keys(F, ctx, logQ)
        sk1P, pk0P, pk1P, kskP = keys(FP, ctxP, logQ)
        cmax = max(a.count or COUNTS)
        vals = np.random.default_rng(m).integers(0, p, size=(cmax, n))
        x, xP = ctx.alloc(cmax * ctb), ctxP.alloc(cmax * ctb)
        S.encrypt_batch_seeded(pk0, pk1, logQ, 99, 0, vals, x, nl, only_usable=False)
        SP.encrypt_batch_seeded(pk0P, pk1P, logQ, 99, 0, vals, xP, nl, only_usable=False)
        base = {"m": m, "p": p, "logQ": logQ, "chain_primes": len(primes), "baseline_library": "parent checkout" if a.tree else "this tree"}

        def scaled(dst, src_ptr, c, count):
            """dst = c * src: a copy and Ciphertext *= long"""
            ctxP.dev_copy(dst.ptr.value, src_ptr, count * ctb)
            ctxP.ct_mul_long_dev(logQ, dst, int(c), 2, nl, count)

        def add_const(buf, c, count):
            poly = np.zeros((1, n), dtype=np.int64)
            poly[0, 0] = c
            ctxP.ct_add_const_dev(logQ, p, buf, 2, nl, count, poly)

        def lin_comb3(dst, tmp, terms, konst, count):
            """copy + *= long + += per term (terms [(c, buffer)]), += ZZX"""
            if not terms:
                ctxP.dev_copy(dst.ptr.value, zero.ptr.value, count * ctb)
            for i, (c, buf) in enumerate(terms):
                scaled(dst if i == 0 else tmp, buf.ptr.value, c, count)
                if i:
                    ctxP.ct_add_dev(logQ, dst, tmp, 2, nl, count)
            add_const(dst, konst, count)

        zero = ctxP.upload(np.zeros(cmax * ctb // 8, dtype=np.uint64))
        # ---- the scalar linear combination alone
        for T in (1, 4, 16):
            count = 64 if m == 4096 else 8
            pool = ctx.upload(P.rand_limbs(np.random.default_rng(T), (T * count, 2, n), nl, logQ))
            poolP = ctxP.upload(pool.download((T * count, 2, n, nl)))
            out, accP, tmpP = ctx.alloc(count * ctb), ctxP.alloc(count * ctb), ctxP.alloc(count * ctb)
            cf = [int(c) for c in np.random.default_rng(T + 1).integers(-p // 2, p // 2, size=T)]
            ia = [t * count + i for i in range(count) for t in range(T)]
            new = lambda: ctx.ct_lin_comb_dev(logQ, p, pool, T * count, nl, ia, cf * count, [T * i for i in range(count + 1)], [7] * count, out)

            class Part:
                def __init__(self, t):
                    self.ptr = FP.binding._vp(poolP.ptr.value + t * count * ctb)
            three = lambda: lin_comb3(accP, tmpP, [(cf[t], Part(t)) for t in range(T)], 7, count)
            tm = alternately({"new": (new, ctx.sync), "three_pass": (three, ctxP.sync)})
            same = bool(np.array_equal(out.download((count, 2, n, nl)), accP.download((count, 2, n, nl))))
            keep(dict(base, workload="lin_comb", terms=T, count=count, time=tm, three_pass_over_new=round(tm["three_pass"]["ms"] / tm["new"]["ms"], 3),
                      baseline_spread=tm["three_pass"]["spread"], same_words=same))
        # ---- the evaluation
        for d in (a.degree or DEGREES):
            coef = [int(c) for c in np.random.default_rng(m + d).integers(1, p, size=d + 1)]
            s = PM.schedule(coef, p)
            plan = F.poly_eval_plan(d)
            want0 = [sum(c * pow(int(v), k, p) for k, c in enumerate(coef)) % p for v in vals[0]]
            for count in (a.count or COUNTS):
                out = ctx.alloc(count * ctb)
                hy, hn = ctxP.alloc(count * ctb), ctxP.alloc(count * ctb)
                pw = {k: ctxP.alloc(count * ctb) for level in s["levels"] for k, _, _ in level}
                pw[1] = xP
                us = {gg: ctxP.alloc(count * ctb) for gg, _, _ in s["inner"]}
                W, tmp, tmp2, cy = (ctxP.alloc(count * ctb) for _ in range(4))
                state = {}

                def new():
                    S.poly_eval(ksk, coef, logQ, x, nl, count, out)

                def horner():
                    y, nx = hy, hn
                    scaled(y, xP.ptr.value, coef[d], count)
                    add_const(y, coef[d - 1], count)
                    for k in range(d - 2, -1, -1):
                        ctxP.ct_mul_relin_dev(kskP, logQ, p, y, xP, nx, nl, count)
                        y, nx = nx, y
                        add_const(y, coef[k], count)
                    state["horner"] = y

                def composed():
                    for level in s["levels"]:
                        for k, ka, kb in level:
                            ctxP.ct_mul_relin_dev(kskP, logQ, p, pw[ka], pw[kb], pw[k], nl, count)
                    for gg, terms, konst in s["inner"]:
                        lin_comb3(us[gg], tmp, [(c, pw[j]) for c, j in terms], konst, count)
                    for i, (gg, k) in enumerate(s["pairs"]):
                        ctxP.ct_mul_relin_dev(kskP, logQ, p, us[gg], pw[k], W if i == 0 else tmp2, nl, count)
                        if i:
                            ctxP.ct_add_dev(logQ, W, tmp2, 2, nl, count)
                    terms, konst = s["final"]
                    lin_comb3(cy, tmp, [(c, W if ref[0] == "W" else pw[ref[1]]) for c, ref in terms], konst, count)

                tm = alternately({"new": (new, ctx.sync), "horner": (horner, ctxP.sync), "composed": (composed, ctxP.sync)})
                got = S.decrypt_batch(sk1, logQ, out, nl, count, only_usable=False)
                gotc = SP.decrypt_batch(sk1P, logQ, cy, nl, count, only_usable=False)
                goth = SP.decrypt_batch(sk1P, logQ, state["horner"], nl, count, only_usable=False)
                rec = dict(base, workload="poly_eval", degree=d, count=count, B=plan["B"], G=plan["G"], depth_new=plan["depth"], depth_horner=d - 1,
                           key_switches={"new": plan["nks"], "composed": plan["nprod"], "horner": d - 1}, time=tm,
                           horner_over_new=round(tm["horner"]["ms"] / tm["new"]["ms"], 3), horner_key_switch_ratio=round((d - 1) / plan["nks"], 3),
                           horner_spread=tm["horner"]["spread"],
                           composed_over_new=round(tm["composed"]["ms"] / tm["new"]["ms"], 3), composed_key_switch_ratio=round(plan["nprod"] / plan["nks"], 3),
                           composed_spread=tm["composed"]["spread"],
                           min_noise_budget={"new": int(np.asarray(S.noise_budget(sk1, logQ, out, nl, count)).min()),
                                             "composed": int(np.asarray(SP.noise_budget(sk1P, logQ, cy, nl, count)).min()),
                                             "horner": int(np.asarray(SP.noise_budget(sk1P, logQ, state["horner"], nl, count)).min())},
                           correct={"new": [int(v) for v in got[0]] == want0, "composed": [int(v) for v in gotc[0]] == want0, "horner": [int(v) for v in goth[0]] == want0},
                           loadavg=[round(v, 2) for v in os.getloadavg()])
                keep(rec)
                for b in [out, hy, hn, W, tmp, tmp2, cy] + [b for k, b in pw.items() if k != 1] + list(us.values()):
                    b.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="root of a built checkout of the parent commit: its binding and library run Horner and the composed schedule (default: this tree's)")
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--degree", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--out")
    main(ap.parse_args())
