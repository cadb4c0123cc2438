#!/usr/bin/env python3
"""Strided convolutions and sum pooling on packed slots, measured against what a caller of the parent commit has.

    python3 tools/bench_lattice.py --tree <checkout of the parent commit, built> --out profiles/lattice_bench.json

The baselines go through the package imported from --tree under another name -- the parent's own binding and library, on a context and a key set of its own
made from the same seeds (without --tree: this tree's, which has the same entry points).  Rings (4096, 65537, logQ 128) and (2^15, 65537, logQ 512), two
rows, plane 32 x 32 (a whole row / eight images per row, one random image per row replicated in every block), count in {1, 8} real encryptions.
  pool     fhesi_ct_pool2d_dev over 2 x 2, 4 x 4 and the global 32 x 32 window in form 1 (hoisted sums) and form 2 (doubling) against the parent's
           fhesi_ct_conv2d_dev with an all-ones kernel of the window's size anchored at (0, 0), in the planner's form: the same sums where the windows start,
           through a plaintext product
  conv     a 3 x 3 convolution of stride 2, Cin = Cout = 1, in both forms against the parent's only route: the strided map as a Toeplitz matrix (zero rows off
           the output lattice) through fhesi_linear_grid in blocks of 1024 x 1024
  create   the stride-2 handle from a tensor in HBM against SlotSpace.plain of the masks built in numpy
Per workload and count every form is warmed up once, then timed alternately `--reps` times each; times are host clocks around a call that ends in a stream
synchronise: median / min / max.  Recorded beside them: key switches, matrices, resident bytes of prepared plaintexts and matrices, the least decrypted noise
budget of each result, the check of every decrypted slot, the baseline's spread (max - min) and per form "margin_ok": its median is below the baseline's by
more than that spread."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(4096, 65537, 3, 128), (1 << 15, 65537, 3, 512)]
PLANE = (32, 32)
WINDOWS = [(2, 2), (4, 4), (32, 32)]
COUNTS = (1, 8)
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def load_parent(tree):
    """the package of another checkout under another name: its binding loads its own library"""
    d = os.path.join(tree, "fhe-si_amd")
    spec = importlib.util.spec_from_file_location("fhe_si_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fhe_si_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(ts):
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def once(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternately(calls, reps):
    """calls {name: (fn, sync)} -> {name: [ms]}: one warm-up of each, then the forms in turn"""
    for fn, sync in calls.values():
        once(fn, sync)
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, (fn, sync) in calls.items():
            ts[k].append(once(fn, sync))
    return ts


class DevTensor:
    """an int64 array in HBM as SlotSpace.conv2d(device=True) takes it"""

    def __init__(self, ctx, a):
        self.buf, self.shape, self.dtype = ctx.upload(a), a.shape, "int64"

    def data_ptr(self):
        return self.buf.ptr.value

    def is_contiguous(self):
        return True


class Side:
    """one library: its context, two-row space, keys from the seeds, derived matrices by amount"""

    def __init__(self, FX, m, p, g, logQ, mods):
        np, R, O, P = mods
        self.F, self.g, self.m, self.logQ = FX, g, m, logQ
        primes, roots = P.chain_for(m, logQ, p)
        self.L = len(primes)
        self.ctx = FX.Context(m, primes, roots)
        self.S = FX.SlotSpace.pow2(self.ctx, p, g)
        self.nd = R.ndigits(logQ)
        n, nl = self.ctx.phim, (logQ + 63) // 64
        self.sk1 = FX.DoubleCRT(self.ctx).sample(0, 64, SEED, 7)
        c1 = FX.DoubleCRT.from_poly(self.ctx, P.rand_limbs(np.random.default_rng(SEED), (n,), nl, logQ))
        self.pk0 = self.sk1.copy().op(c1, FX.OP_MUL).op(FX.DoubleCRT(self.ctx).sample(1, 0, SEED, 9), FX.OP_ADD)
        self.pk1 = FX.DoubleCRT.from_poly(self.ctx, O.ints_to_limbs([0] * n, 1)).op(c1, FX.OP_SUB)
        self.one = FX.DoubleCRT.from_poly(self.ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
        self.mats = {0: None}

    def matrix(self, e):
        if e not in self.mats:
            k = pow(self.g, e, self.m)
            w = self.F.KeySwitchMatrix(self.ctx, 2, self.nd).init_batch_seeded([self.one, self.sk1.copy().automorph(k)], self.sk1, self.logQ, SEED, PUB, 2000 + 100 * e)
            self.mats[e] = w.hoist(k)
        return self.mats[e]

    def matrix_bytes(self, amounts):
        return sum(int(self.matrix(e).nbytes) for e in set(amounts) if e)

    def encrypt(self, vals, count, nl):
        buf = self.ctx.alloc(count * 2 * self.ctx.phim * nl * 8)
        self.S.encrypt_batch_seeded(self.pk0, self.pk1, self.logQ, 99, 0, vals, buf, nl, only_usable=False)
        return buf

    def budget(self, np, buf, nl, count):
        return int(np.asarray(self.S.noise_budget(self.sk1, self.logQ, buf, nl, count)).min())

    def decrypt(self, buf, nl, count):
        return self.S.decrypt_batch(self.sk1, self.logQ, buf, nl, count, only_usable=False)


def pool_formula(np, x, W, kh, kw, rows, p):
    """lattice_model.pool_formula at step (1, 1) in int64: x [count][rows * cols]"""
    v = x.reshape(x.shape[0], rows, -1)
    inner = sum(np.roll(v, -dx, axis=-1) for dx in range(kw))
    return (sum(np.roll(inner, -dy * W, axis=-1) for dy in range(kh)) % p).reshape(x.shape)


def strided_direct(np, K, b, x, H, W, stride, rows, p):
    """lattice_model.direct for one channel, a 3 x 3 kernel anchored at its centre, step and dilation (1, 1), in int64: x [count][rows * cols]"""
    img = x.reshape(x.shape[0], rows, -1, H, W)
    pad = np.zeros(img.shape[:3] + (H + 2, W + 2), dtype=np.int64)
    pad[..., 1:1 + H, 1:1 + W] = img
    out = np.zeros(img.shape, dtype=np.int64) + int(b)
    for dy in range(3):
        for dx in range(3):
            out += (int(K[dy][dx]) % p) * pad[..., dy:dy + H, dx:dx + W]
    on = np.zeros((H, W), dtype=np.int64)
    on[::stride[0], ::stride[1]] = 1
    return ((out % p) * on).reshape(x.shape)


def strided_toeplitz(np, K, H, W, stride, p):
    """[P][P]: row y W + x on the output lattice, column yy W + xx; zero rows off the lattice"""
    P_ = H * W
    M = np.zeros((P_, P_), dtype=np.int64)
    y, x = np.divmod(np.arange(P_), W)
    for dy in range(3):
        for dx in range(3):
            yy, xx = y + dy - 1, x + dx - 1
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & (y % stride[0] == 0) & (x % stride[1] == 0)
            M[np.arange(P_)[ok], (yy * W + xx)[ok]] = int(K[dy][dx]) % p
    return M


def run(a):
    for d in (os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), HERE):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    import fhesi_pyref as R
    import lattice_model as LM
    import oracle_lib as O
    import params as P
    FP = load_parent(a.tree) if a.tree else F
    lines = []

    def keep(rec):
        """print the record and rewrite --out, so that a run cut short leaves what it measured"""
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)

    H, W = PLANE
    P_ = H * W
    for m, p, g, logQ in RINGS:
        if a.m and m not in a.m:
            continue
        new, old = Side(F, m, p, g, logQ, (np, R, O, P)), Side(FP, m, p, g, logQ, (np, R, O, P))
        ctx, S, n, cols, nl = new.ctx, new.S, new.ctx.phim, new.S.cols, (logQ + 63) // 64
        ctb = 2 * n * nl * 8
        base = {"m": m, "p": p, "logQ": logQ, "chain_primes": new.L, "digits": new.nd, "cols": cols, "H": H, "W": W,
                "baseline_library": "parent checkout" if a.tree else "this tree"}
        rng = np.random.default_rng(m)
        cmax = max(a.count or COUNTS)
        img = rng.integers(0, p, size=(cmax, 2, 1, H, W)).astype(np.int64)
        xs = S.pack_images(np.broadcast_to(img, (cmax, 2, cols // P_, H, W)))      # [cmax][n]
        src, srcP = new.encrypt(xs, cmax, nl), old.encrypt(xs, cmax, nl)
        fresh = new.budget(np, src, nl, cmax)
        # ---- (a) sum pooling against the parent's all-ones convolution
        for kh, kw in WINDOWS:
            plans = {form: F.pool2d_plan(cols, H, W, kh, kw, 1, 1, form) for form in (1, 2)}
            ones = old.S.conv2d(np.ones((1, 1, kh, kw), dtype=np.int64), None, (H, W), (0, 0), 0)
            hs = {form: [new.matrix(t) for t in plans[form]["amounts"]] for form in (1, 2)}
            hP = [old.matrix(t) for t in ones.amounts]
            on = np.tile(LM.lattice(H, W, (kh, kw), 2, cols) == 1, (cmax, 1))
            for count in (a.count or COUNTS):
                outs = {1: ctx.alloc(count * ctb), 2: ctx.alloc(count * ctb)}
                outP = old.ctx.alloc(count * ctb)
                calls = {"form1": (lambda: S.pool2d(hs[1], (H, W), (kh, kw), (1, 1), logQ, src, nl, count, outs[1], 1), ctx.sync),
                         "form2": (lambda: S.pool2d(hs[2], (H, W), (kh, kw), (1, 1), logQ, src, nl, count, outs[2], 2), ctx.sync),
                         "ones_conv": (lambda: ones.apply(hP, logQ, srcP, nl, count, outP), old.ctx.sync)}
                ts = alternately(calls, a.reps)
                want = pool_formula(np, xs[:count], W, kh, kw, 2, p)
                sums = old.decrypt(outP, nl, count)
                bt = spread(ts["ones_conv"])
                r = dict(base, workload="pool", kh=kh, kw=kw, count=count, planner_form=F.pool2d_plan(cols, H, W, kh, kw)["form"], fresh_noise_budget=fresh,
                         ones_conv={"form": ones.form, "key_switches": ones.key_switches, "matrices": len(set(ones.amounts) - {0}), "plaintexts": kh * kw,
                                    "plaintext_bytes": kh * kw * old.L * n * 8, "matrix_bytes": old.matrix_bytes(ones.amounts), "time": bt,
                                    "min_noise_budget": old.budget(np, outP, nl, count), "correct_where_windows_start": bool(np.array_equal(sums[on[:count]], want[on[:count]]))},
                         baseline_spread_ms=round(bt["max_ms"] - bt["min_ms"], 4))
                for form in (1, 2):
                    t = spread(ts["form%d" % form])
                    r["form%d" % form] = {"key_switches": plans[form]["key_switches"], "levels": plans[form]["levels"], "matrices": len(set(plans[form]["amounts"])),
                                          "plaintext_bytes": 0, "matrix_bytes": new.matrix_bytes(plans[form]["amounts"]), "time": t,
                                          "min_noise_budget": new.budget(np, outs[form], nl, count), "correct": bool(np.array_equal(new.decrypt(outs[form], nl, count), want)),
                                          "baseline_over_this": round(bt["ms"] / t["ms"], 3), "margin_ok": bool(bt["ms"] - t["ms"] > bt["max_ms"] - bt["min_ms"])}
                r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
                keep(r)
                for buf in list(outs.values()) + [outP]:
                    buf.free()
            ones.close()
        # ---- (b) a 3 x 3 convolution of stride 2 against the parent's Toeplitz grid, (c) handle creation
        stride = (2, 2)
        K, b = rng.integers(0, p, size=(1, 1, 3, 3)).astype(np.int64), rng.integers(0, p, size=1).astype(np.int64)
        dK, db = DevTensor(ctx, K), DevTensor(ctx, b)
        forms, info = {}, {}
        for name, form in (("flat", 1), ("split", 2)):
            made, plains = [], []

            def create():
                made.append(S.conv2d(dK, db, (H, W), (1, 1), form, device=True, stride=stride))
                while len(made) > 1:
                    made.pop(0).close()

            def create_numpy():
                w = (LM.prepared(K, H, W, (1, 1), (1, 1), stride, (1, 1), 2, cols, form) % p).astype(np.int64).reshape(-1, n)
                plains.append(S.plain(w, False))
                while len(plains) > 1:
                    plains.pop(0).close()
            create()
            ctx.sync()
            t_dev = spread([once(create, ctx.sync) for _ in range(3)])
            t_np = spread([once(create_numpy, ctx.sync) for _ in range(2)])
            plains.pop().close()
            cv = forms[name] = made[-1]
            info[name] = {"key_switches": cv.key_switches, "matrices": len(set(cv.amounts) - {0}), "terms": cv.terms, "plaintexts": 9, "plaintext_bytes": 9 * new.L * n * 8,
                          "matrix_bytes": new.matrix_bytes(cv.amounts), "create_dev": t_dev, "create_numpy_plain": t_np,
                          "create_numpy_over_dev": round(t_np["ms"] / t_dev["ms"], 2)}
        M = strided_toeplitz(np, K[0][0], H, W, stride, p)
        bias_rows = (int(b[0]) * (LM.lattice(H, W, stride, 1, P_) == 1)).astype(np.int64)
        lin = old.S.linear_grid(M, bias_rows, (P_, P_))
        hg = [old.matrix(t) for t in lin.amounts]
        info["grid"] = {"key_switches": lin.key_switches, "matrices": len(set(lin.amounts)), "B": lin.B, "G": lin.G, "plaintexts": lin.T, "plaintext_bytes": lin.T * old.L * n * 8,
                        "matrix_bytes": old.matrix_bytes(lin.amounts)}
        hc = {name: [new.matrix(t) for t in cv.amounts] for name, cv in forms.items()}
        for count in (a.count or COUNTS):
            outs = {name: ctx.alloc(count * ctb) for name in forms}
            outP = old.ctx.alloc(count * ctb)
            calls = {"flat": (lambda: forms["flat"].apply(hc["flat"], logQ, src, nl, count, outs["flat"]), ctx.sync),
                     "split": (lambda: forms["split"].apply(hc["split"], logQ, src, nl, count, outs["split"]), ctx.sync),
                     "grid": (lambda: lin.apply(hg, logQ, srcP, nl, count, outP), old.ctx.sync)}
            ts = alternately(calls, a.reps)
            want = strided_direct(np, K[0][0], b[0], xs[:count], H, W, stride, 2, p)
            gt = spread(ts["grid"])
            r = dict(base, workload="conv_stride2", kh=3, kw=3, Cin=1, Cout=1, count=count, fresh_noise_budget=fresh,
                     planner_form=F.conv2d_lattice_plan(cols, H, W, 1, 1, 3, 3, 1, 1, stride=stride)["form"], baseline_spread_ms=round(gt["max_ms"] - gt["min_ms"], 4))
            r["grid"] = dict(info["grid"], time=gt, min_noise_budget=old.budget(np, outP, nl, count), correct=bool(np.array_equal(old.decrypt(outP, nl, count), want)))
            for name in forms:
                t = spread(ts[name])
                r[name] = dict(info[name], time=t, min_noise_budget=new.budget(np, outs[name], nl, count), correct=bool(np.array_equal(new.decrypt(outs[name], nl, count), want)),
                               baseline_over_this=round(gt["ms"] / t["ms"], 3), margin_ok=bool(gt["ms"] - t["ms"] > gt["max_ms"] - gt["min_ms"]))
            r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
            keep(r)
            for buf in list(outs.values()) + [outP]:
                buf.free()
        lin.close()
        for cv in forms.values():
            cv.close()
        S.close()
        old.S.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="root of a built checkout of the parent commit: its binding and library run the baselines (default: this tree's)")
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    run(ap.parse_args())
