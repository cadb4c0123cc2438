#!/usr/bin/env python3
"""Dense layers larger than a row of slots, measured: fhesi_ct_linear_grid_dev (babies shared across output blocks, giants and folds behind the sum over
input blocks) against the form the parent commit has -- one fhesi_linear per block, nI nJ calls of fhesi_ct_linear_dev with fhesi_ct_add_dev between
them.

    python3 tools/bench_linear_grid.py --tree <checkout of the parent commit, built> --out profiles/linear_grid_bench.json

Workload: count in {1, 8} items (real encryptions of SlotSpace.replicate_blocks of random vectors) on the two-row rings (4096, 65537, logQ 128) --
blocks of 64 x 64 in 2 x 2 and 4 x 4 grids and blocks of 1024 x 1024 (the whole row) in a 2 x 2 grid, the matrix a row cannot hold -- and
(2^16, 65537, logQ 512) -- 64 x 64 in a 4 x 4 grid; M and b uniform in [0, p); rotation amount t is k = g^t, its matrix generated on the device from a
seed that depends on t alone, so both forms hold the same keys.  The per-block form runs through the package imported from --tree under another name:
the parent's own binding and library, in the same process, on a context of its own (without --tree: this tree's, and the record says so).  Per shape and
count both forms are warmed up once, then timed alternately -- grid, per block, grid, .. -- `--reps` times each; times are host clocks around a call that
ends in a stream synchronise: median / min / max.  Recorded beside them: the key switches of both forms, the time to make the grid's handle from a
matrix in HBM (and the per-block handles'), the least decrypted noise budget of both results, the check of every decrypted slot against M x + b, and
"margin_ok": the grid's median is below the per-block median by more than the per-block form's spread (max - min)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (m, p, g, logQ, [(Rb, Cb, nI, nJ)]); Rb = Cb = 0 stands for the whole row
RINGS = [(4096, 65537, 3, 128, [(64, 64, 2, 2), (64, 64, 4, 4), (0, 0, 2, 2)]), (1 << 16, 65537, 3, 512, [(64, 64, 4, 4)])]
COUNTS = (1, 8)
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def spread(ts):
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def once(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def load_parent(tree):
    """the package of another checkout under a name of its own: its binding, its library"""
    d = os.path.join(tree, "fhe-si_amd")
    spec = importlib.util.spec_from_file_location("fhe_si_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fhe_si_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


class DevTensor:
    """an int64 array in HBM as SlotSpace.linear(device=True) takes it"""

    def __init__(self, ctx, a):
        self.buf, self.shape, self.dtype = ctx.upload(a), a.shape, "int64"

    def data_ptr(self):
        return self.buf.ptr.value

    def is_contiguous(self):
        return True


class Side:
    """one package on one context: the two-row space, the keys from the shared seeds, the derived matrices by amount"""

    def __init__(self, F, m, p, g, logQ):
        import fhesi_pyref as R
        import oracle_lib as O
        import params as P
        import numpy as np
        self.F, self.g, self.m, self.logQ = F, g, m, logQ
        primes, roots = P.chain_for(m, logQ, p)
        self.primes = primes
        self.ctx = F.Context(m, primes, roots)
        self.S = F.SlotSpace.pow2(self.ctx, p, g)
        n, nl = self.ctx.phim, (logQ + 63) // 64
        self.nd = R.ndigits(logQ)
        # slots_common.device_keys with this side's package
        self.sk1 = F.DoubleCRT(self.ctx).sample(0, 64, SEED, 7)
        c1 = F.DoubleCRT.from_poly(self.ctx, P.rand_limbs(np.random.default_rng(SEED), (n,), nl, logQ))
        self.pk0 = self.sk1.copy().op(c1, F.OP_MUL).op(F.DoubleCRT(self.ctx).sample(1, 0, SEED, 9), F.OP_ADD)
        self.pk1 = F.DoubleCRT.from_poly(self.ctx, O.ints_to_limbs([0] * n, 1)).op(c1, F.OP_SUB)
        self.one = F.DoubleCRT.from_poly(self.ctx, O.ints_to_limbs([1] + [0] * (n - 1), 1))
        self.mats = {0: None}

    def matrix(self, e):
        if e not in self.mats:
            k = pow(self.g, e, self.m)
            w = self.F.KeySwitchMatrix(self.ctx, 2, self.nd).init_batch_seeded([self.one, self.sk1.copy().automorph(k)], self.sk1, self.logQ, SEED, PUB, 2000 + 100 * e)
            self.mats[e] = w.hoist(k)
        return self.mats[e]


def run(a):
    for d in (os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), HERE):
        sys.path.insert(0, d)
    import numpy as np
    import fhe_si_amd as F
    from slots_common import View
    FP = load_parent(a.tree) if a.tree else F
    lines = []

    def keep(rec):
        """print the record and rewrite --out, so that a run cut short leaves what it measured"""
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)

    for m, p, g, logQ, shapes in RINGS:
        if a.m and m not in a.m:
            continue
        new, old = Side(F, m, p, g, logQ), Side(FP, m, p, g, logQ)
        ctx, S = new.ctx, new.S
        n, nl, cols = ctx.phim, (logQ + 63) // 64, S.cols
        ctb = 2 * n * nl * 8
        for Rb, Cb, nI, nJ in shapes:
            Rb, Cb = Rb or cols, Cb or cols
            Rr, Cc = nI * Rb, nJ * Cb
            rng = np.random.default_rng(m + Rr + 7 * Cc)
            M, b = rng.integers(0, p, size=(Rr, Cc)).astype(np.int64), rng.integers(0, p, size=Rr).astype(np.int64)
            pl, pb = F.linear_grid_plan(cols, Rr, Cc, Rb, Cb), FP.linear_plan(cols, Rb, Cb)
            base = {"workload": "linear_grid", "m": m, "p": p, "logQ": logQ, "chain_primes": len(new.primes), "digits": new.nd, "cols": cols, "R": Rr, "C": Cc,
                    "Rb": Rb, "Cb": Cb, "nI": nI, "nJ": nJ, "grid": {k: pl[k] for k in ("T", "B", "G", "nfold", "key_switches")},
                    "per_block": {"B": pb["B"], "G": pb["G"], "nfold": pb["nfold"], "key_switches": nI * nJ * len(pb["amounts"])},
                    "per_block_library": "parent checkout" if a.tree else "this tree"}
            # the handles: the grid's from the matrix in HBM, timed; the per-block form's nI nJ layers from their blocks in HBM, timed as one
            dM, db = DevTensor(ctx, M), DevTensor(ctx, b)
            made = []

            def create_grid():
                made.append(S.linear_grid(dM, db, (Rb, Cb), device=True))
                while len(made) > 1:
                    made.pop(0).close()
            create_grid()
            ctx.sync()
            base["create_grid_dev"] = spread([once(create_grid, ctx.sync) for _ in range(3)])
            base["diagonal_bytes"] = nI * nJ * pl["T"] * n * 8
            lin = made[-1]
            blocks = [[(DevTensor(old.ctx, np.ascontiguousarray(M[I * Rb:(I + 1) * Rb, J * Cb:(J + 1) * Cb])),
                        DevTensor(old.ctx, np.ascontiguousarray(b[I * Rb:(I + 1) * Rb])) if J == 0 else None) for J in range(nJ)] for I in range(nI)]
            layers = []

            def create_layers():
                while layers:
                    layers.pop().close()
                for I in range(nI):
                    for J in range(nJ):
                        layers.append(old.S.linear(blocks[I][J][0], blocks[I][J][1], device=True))
            create_layers()
            old.ctx.sync()
            base["create_per_block_dev"] = spread([once(create_layers, old.ctx.sync) for _ in range(3)])
            hs, hp = [new.matrix(t) for t in lin.amounts], [old.matrix(t) for t in pb["amounts"]]
            for count in (a.count or COUNTS):
                x = rng.integers(0, p, size=(count, 2, Cc)).astype(np.int64)
                xs = S.replicate_blocks(x, Cb).reshape(nJ * count, n)
                src, out = ctx.alloc(nJ * count * ctb), ctx.alloc(nI * count * ctb)
                srcp, outp, tmp = old.ctx.alloc(nJ * count * ctb), old.ctx.alloc(nI * count * ctb), old.ctx.alloc(count * ctb)
                S.encrypt_batch_seeded(new.pk0, new.pk1, logQ, 99, 0, xs, src, nl, only_usable=False)
                old.S.encrypt_batch_seeded(old.pk0, old.pk1, logQ, 99, 0, xs, srcp, nl, only_usable=False)

                def grid():
                    lin.apply(hs, logQ, src, nl, count, out)

                def per_block():
                    for I in range(nI):
                        y = View(outp, I * count * ctb)
                        for J in range(nJ):
                            layers[I * nJ + J].apply(hp, logQ, View(srcp, J * count * ctb), nl, count, tmp if J else y)
                            if J:
                                old.ctx.ct_add_dev(logQ, y, tmp, 2, nl, count)

                once(grid, ctx.sync)
                once(per_block, old.ctx.sync)
                tg, tp = [], []
                for _ in range(a.reps):
                    tg.append(once(grid, ctx.sync))
                    tp.append(once(per_block, old.ctx.sync))
                r = dict(base, count=count, grid_time=spread(tg), per_block_time=spread(tp))
                r["per_block_over_grid"] = round(r["per_block_time"]["ms"] / r["grid_time"]["ms"], 3)
                r["key_switch_ratio"] = round(base["per_block"]["key_switches"] / max(1, pl["key_switches"]), 3)
                r["margin_ok"] = bool(r["per_block_time"]["ms"] - r["grid_time"]["ms"] > r["per_block_time"]["max_ms"] - r["per_block_time"]["min_ms"])
                r["min_noise_budget_grid"] = int(np.asarray(S.noise_budget(new.sk1, logQ, out, nl, nI * count)).min())
                r["min_noise_budget_per_block"] = int(np.asarray(old.S.noise_budget(old.sk1, logQ, outp, nl, nI * count)).min())
                # every decrypted slot: slot (r, i) of block I = (M x_r + b)[I Rb + (i mod Rb)] (the sums stay below 2^63: p^2 C < 2^44)
                y = np.stack([x[:, r0, :] @ M.T + b for r0 in range(2)], axis=1) % p          # [count][2][R]
                want = np.stack([np.tile(y[:, :, I * Rb:(I + 1) * Rb], cols // Rb).reshape(count, n) for I in range(nI)])
                got = S.decrypt_batch(new.sk1, logQ, out, nl, nI * count, only_usable=False).reshape(nI, count, n)
                gotp = old.S.decrypt_batch(old.sk1, logQ, outp, nl, nI * count, only_usable=False).reshape(nI, count, n)
                r["correct_grid"], r["correct_per_block"] = bool(np.array_equal(got, want)), bool(np.array_equal(gotp, want))
                r["collect_blocks_correct"] = bool(np.array_equal(S.collect_blocks(got, Rb), y))
                r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
                keep(r)
                for buf in (src, out, srcp, outp, tmp):
                    buf.free()
            lin.close()
            while layers:
                layers.pop().close()
        S.close()
        old.S.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="root of a built checkout of the parent commit: its binding and library run the per-block form (default: this tree's)")
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    run(ap.parse_args())
