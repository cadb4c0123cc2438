#!/usr/bin/env python3
"""Convolution layers on packed slots, measured: fhesi_ct_conv2d_dev (kh kw rotations per input channel from one digit set, masked weight plaintexts, one
exact plaintext sum) against the only form the library had before -- the same map as a fhesi_linear_grid on its Toeplitz matrix, P diagonals per channel
pair.  Both go through this library, in the same process, on the same context and keys.

    python3 tools/bench_conv.py --out profiles/conv_bench.json

Workload: count in {1, 8} items (real encryptions of one random image per row, replicated in every block where the row holds several: the input both
forms take) on the two-row rings (4096, 65537, logQ 128) -- plane 32 x 32, a whole row, 3 x 3 centred, Cin = Cout = 1 and 4 -- and (2^15, 65537, logQ 512)
-- the same plane, eight images per row, Cin = Cout = 1; K and b uniform in [0, p); rotation amount t is k = g^t, its matrix generated on the device.
Per configuration and count the flat form, the split form and the Toeplitz grid are warmed up once, then timed alternately -- flat, split, grid, flat,
.. -- `--reps` times each; times are host clocks around a call that ends in a stream synchronise: median / min / max.  Recorded beside them: the key
switches and the distinct matrices of each form, the resident bytes of the prepared plaintexts and of the matrices, the time to make the handle from a
tensor in HBM against SlotSpace.plain of masks built in numpy, the least decrypted noise budget of each result, the check of every decrypted slot against
the direct convolution, and per form "margin_ok": its median is below the grid's by more than the grid's own spread (max - min)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (m, p, g, logQ, (H, W), (kh, kw), [(Cin, Cout)])
RINGS = [(4096, 65537, 3, 128, (32, 32), (3, 3), [(1, 1), (4, 4)]), (1 << 15, 65537, 3, 512, (32, 32), (3, 3), [(1, 1)])]
COUNTS = (1, 8)
SEED, PUB = 0x51A7E5EED, 0x5DEECE66D


def spread(ts):
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def once(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


class DevTensor:
    """an int64 array in HBM as SlotSpace.conv2d(device=True) takes it"""

    def __init__(self, ctx, a):
        self.buf, self.shape, self.dtype = ctx.upload(a), a.shape, "int64"

    def data_ptr(self):
        return self.buf.ptr.value

    def is_contiguous(self):
        return True


class Side:
    """one context: the two-row space, the keys, the derived matrices by amount"""

    def __init__(self, F, m, p, g, logQ):
        import fhesi_pyref as R
        import oracle_lib as O
        import params as P
        from slots_common import device_keys
        self.F, self.g, self.m, self.logQ = F, g, m, logQ
        primes, roots = P.chain_for(m, logQ, p)
        self.primes = primes
        self.ctx = F.Context(m, primes, roots)
        self.S = F.SlotSpace.pow2(self.ctx, p, g)
        self.nd = R.ndigits(logQ)
        self.sk1, self.pk0, self.pk1 = device_keys(self.ctx, logQ, SEED)
        self.one = F.DoubleCRT.from_poly(self.ctx, O.ints_to_limbs([1] + [0] * (self.ctx.phim - 1), 1))
        self.mats = {0: None}

    def matrix(self, e):
        if e not in self.mats:
            k = pow(self.g, e, self.m)
            w = self.F.KeySwitchMatrix(self.ctx, 2, self.nd).init_batch_seeded([self.one, self.sk1.copy().automorph(k)], self.sk1, self.logQ, SEED, PUB, 2000 + 100 * e)
            self.mats[e] = w.hoist(k)
        return self.mats[e]

    def matrix_bytes(self, amounts):
        return sum(int(self.matrix(e).nbytes) for e in set(amounts) if e)


def toeplitz(K, H, W, anchor, p, np):
    """[Cout P][Cin P], row I P + y W + x, column J P + yy W + xx (conv_model.toeplitz, by offset instead of by pixel)"""
    Cout, Cin, kh, kw = K.shape
    P_ = H * W
    M = np.zeros((Cout * P_, Cin * P_), dtype=np.int64)
    y, x = np.divmod(np.arange(P_), W)
    for dy in range(kh):
        for dx in range(kw):
            yy, xx = y + dy - anchor[0], x + dx - anchor[1]
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            for I in range(Cout):
                for J in range(Cin):
                    M[I * P_ + np.arange(P_)[ok], J * P_ + (yy * W + xx)[ok]] = int(K[I][J][dy][dx]) % p
    return M


def direct(K, b, xs, H, W, anchor, p, rows, np):
    """conv_model.direct in int64 by shifted planes (p^2 Cin kh kw stays far below 2^63): xs [Cin][rows * cols] -> [Cout][rows * cols]"""
    Cout, Cin, kh, kw = K.shape
    img = xs.reshape(Cin, rows, -1, H, W)
    pad = np.zeros(img.shape[:3] + (H + kh - 1, W + kw - 1), dtype=np.int64)
    pad[..., anchor[0]:anchor[0] + H, anchor[1]:anchor[1] + W] = img
    out = np.zeros((Cout,) + img.shape[1:], dtype=np.int64) + b.reshape(Cout, 1, 1, 1, 1)
    for dy in range(kh):
        for dx in range(kw):
            out += np.einsum("ij,jrnyx->irnyx", K[:, :, dy, dx] % p, pad[..., dy:dy + H, dx:dx + W])
    return (out % p).reshape(Cout, -1)


def run(a):
    for d in (os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), HERE):
        sys.path.insert(0, d)
    import numpy as np
    import conv_model as CM
    import fhe_si_amd as F
    lines = []

    def keep(rec):
        """print the record and rewrite --out, so that a run cut short leaves what it measured"""
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)

    for m, p, g, logQ, (H, W), (kh, kw), channels in RINGS:
        if a.m and m not in a.m:
            continue
        side = Side(F, m, p, g, logQ)
        ctx, S = side.ctx, side.S
        n, nl, cols, P_ = ctx.phim, (logQ + 63) // 64, S.cols, H * W
        ctb, L = 2 * n * nl * 8, len(side.primes)
        anchor = ((kh - 1) // 2, (kw - 1) // 2)
        for Cin, Cout in channels:
            rng = np.random.default_rng(m + 10 * Cin + Cout)
            K, b = rng.integers(0, p, size=(Cout, Cin, kh, kw)).astype(np.int64), rng.integers(0, p, size=Cout).astype(np.int64)
            base = {"workload": "conv2d", "m": m, "p": p, "logQ": logQ, "chain_primes": L, "digits": side.nd, "cols": cols, "H": H, "W": W, "kh": kh, "kw": kw,
                    "Cin": Cin, "Cout": Cout, "planner_form": F.conv2d_plan(cols, H, W, Cin, Cout, kh, kw, anchor[0], anchor[1])["form"]}
            dK, db = DevTensor(ctx, K), DevTensor(ctx, b)
            forms = {}
            for name, form in (("flat", 1), ("split", 2)):
                made = []

                def create():
                    made.append(S.conv2d(dK, db, (H, W), anchor, form, device=True))
                    while len(made) > 1:
                        made.pop(0).close()
                create()
                ctx.sync()
                t_dev = spread([once(create, ctx.sync) for _ in range(3)])
                plains = []

                def create_numpy():
                    w = (CM.prepared(K, H, W, anchor, 2, cols, form) % p).astype(np.int64).reshape(-1, n)
                    plains.append(S.plain(w, False))
                    while len(plains) > 1:
                        plains.pop(0).close()
                t_np = spread([once(create_numpy, ctx.sync) for _ in range(2)])
                plains.pop().close()
                cv = made[-1]
                forms[name] = cv
                base[name] = {"key_switches": cv.key_switches, "matrices": len(set(cv.amounts) - {0}), "terms": cv.terms, "plaintexts": Cout * Cin * kh * kw,
                              "plaintext_bytes": Cout * Cin * kh * kw * L * n * 8, "matrix_bytes": side.matrix_bytes(cv.amounts),
                              "create_dev": t_dev, "create_numpy_plain": t_np}
            M = toeplitz(K, H, W, anchor, p, np)
            t0 = time.perf_counter()
            lin = S.linear_grid(DevTensor(ctx, M), DevTensor(ctx, np.repeat(b, P_)), (P_, P_), device=True)
            ctx.sync()
            base["grid"] = {"key_switches": lin.key_switches, "matrices": len(set(lin.amounts)), "B": lin.B, "G": lin.G, "plaintexts": Cout * Cin * lin.T,
                            "plaintext_bytes": Cout * Cin * lin.T * L * n * 8, "matrix_bytes": side.matrix_bytes(lin.amounts),
                            "create_dev_ms": round((time.perf_counter() - t0) * 1e3, 3)}
            hs = {name: [side.matrix(t) for t in cv.amounts] for name, cv in forms.items()}
            hg = [side.matrix(t) for t in lin.amounts]
            for count in (a.count or COUNTS):
                img = rng.integers(0, p, size=(count, 2, Cin, H, W)).astype(np.int64)
                xs = np.stack([S.pack_images(np.broadcast_to(img[:, :, J][:, :, None], (count, 2, cols // P_, H, W))) for J in range(Cin)])      # [Cin][count][n]
                src = ctx.alloc(Cin * count * ctb)
                outs = {name: ctx.alloc(Cout * count * ctb) for name in ("flat", "split", "grid")}
                S.encrypt_batch_seeded(side.pk0, side.pk1, logQ, 99, 0, xs.reshape(Cin * count, n), src, nl, only_usable=False)
                calls = {"flat": lambda: forms["flat"].apply(hs["flat"], logQ, src, nl, count, outs["flat"]),
                         "split": lambda: forms["split"].apply(hs["split"], logQ, src, nl, count, outs["split"]),
                         "grid": lambda: lin.apply(hg, logQ, src, nl, count, outs["grid"])}
                times = {name: [] for name in calls}
                for name, fn in calls.items():
                    once(fn, ctx.sync)
                for _ in range(a.reps):
                    for name, fn in calls.items():
                        times[name].append(once(fn, ctx.sync))
                r = dict(base, count=count, fresh_noise_budget=int(np.asarray(S.noise_budget(side.sk1, logQ, src, nl, Cin * count)).min()))
                want = np.stack([direct(K, b, xs[:, i], H, W, anchor, p, 2, np) for i in range(count)], axis=1)      # [Cout][count][n]
                for name in calls:
                    r[name + "_time"] = spread(times[name])
                    r["min_noise_budget_" + name] = int(np.asarray(S.noise_budget(side.sk1, logQ, outs[name], nl, Cout * count)).min())
                    got = S.decrypt_batch(side.sk1, logQ, outs[name], nl, Cout * count, only_usable=False).reshape(Cout, count, n)
                    r["correct_" + name] = bool(np.array_equal(got, want))
                gt = r["grid_time"]
                for name in ("flat", "split"):
                    r["grid_over_" + name] = round(gt["ms"] / r[name + "_time"]["ms"], 3)
                    r["margin_ok_" + name] = bool(gt["ms"] - r[name + "_time"]["ms"] > gt["max_ms"] - gt["min_ms"])
                r["loadavg"] = [round(v, 2) for v in os.getloadavg()]
                keep(r)
                for buf in [src] + list(outs.values()):
                    buf.free()
            lin.close()
            for cv in forms.values():
                cv.close()
        S.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="*")
    ap.add_argument("--count", type=int, nargs="*")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    run(ap.parse_args())
