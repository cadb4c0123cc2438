#!/usr/bin/env python3
"""Slot packing on the device, measured: embeds/s and decodes/s on HBM buffers, the fused encrypt-from-slots against encrypt-from-coefficients
on the same batch, and parity of a sample against the model (tests/slots_model.py).  One JSON line per ring.

    python3 tools/bench_slots.py [--p 32603 65543] [--count 256] [--logQ 128] [--warmup 2] [--reps 7]
    python3 tools/bench_slots.py --pow2 [--m 32768 65536] [--pow2-p 65537] [--out profiles/slots_pow2_bench.json]

--pow2: the two-row spaces of the power-of-two rings (tests/slots_pow2_model.py).  Every ring is measured twice in the same process, on the
path the plan picks (the direct negacyclic transform where it applies) and with the chirp forced (SlotSpace.set_path), one JSON line each;
the outputs of the two paths are compared word for word.  --out also writes the lines to a file.

--basis K: a slot basis of K primes below 2^--prime-bits on every ring of --m (integer slots, fhe-si_amd/csrc/kernels_slots_basis.hip):
logical embeds/s (limb reduction in the loader + K inverse transforms, one launch) and decodes/s (K forward transforms + the recombination)
on HBM buffers, and the fused encryption against K single-prime fused encryptions of the residues (reduced on the host, outside the
clock) on the same keys; round trip and channel-by-channel ciphertext equality are checked.

Times are host clocks around work that ends in a stream synchronise; every figure is the median of --reps calls after --warmup calls.
`bytes` are algorithmic (slot values in, message polynomials out, 8 bytes each -- the basis of bench.py's roofline lines), `bound` is
"unknown": no counter pass exists for these kernels."""
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
import params as P  # noqa: E402
import slots_model as M  # noqa: E402
import slots_pow2_model as M2  # noqa: E402


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
    return statistics.median(ts), min(ts), max(ts)


def pow2_case(a, m, p, g, out_lines):
    logQ, count = a.logQ, a.count
    primes, roots = P.chain_for(m, logQ, p)
    ctx = F.Context(m, primes, roots)
    S = F.SlotSpace.pow2(ctx, p, g)
    mod = M2.slot_space(m, p, g)
    n, nl = S.total, (logQ + 63) // 64
    rng = np.random.default_rng(m)
    vals = rng.integers(0, p, size=(count, n)).astype(np.int64)
    d_vals, d_msg, d_back = ctx.upload(vals), ctx.alloc(count * n * 8), ctx.alloc(count * n * 8)
    pk = []
    rows = P.rand_rows(rng, primes, n, 2)
    for r in range(2):
        d = F.DoubleCRT(ctx)
        for i in range(len(primes)):
            d.set_row(i, np.ascontiguousarray(rows[r, i]))
        pk.append(d)
    out_a, out_b = ctx.alloc(count * 2 * n * nl * 8), ctx.alloc(count * 2 * n * nl * 8)
    planned, first_msg = S.path, None
    for forced in ([False, True] if planned == 0 else [False]):
        if forced:
            S.set_path(1)
        t_emb = median_time(lambda: S.embed_dev(d_vals, n, count, d_msg), ctx.sync, a.warmup, a.reps)
        t_dec = median_time(lambda: S.decode_dev(d_msg, count, n, d_back), ctx.sync, a.warmup, a.reps)
        msg = d_msg.download((count, n), np.int64)
        back = d_back.download((count, n), np.int64)
        sample = [0, 1, n // 2 - 1, n // 2, n - 1]
        parity = bool(np.array_equal(back, vals)) and all(M2.decode_slot(mod, [int(x) for x in msg[c]], j) == vals[c, j] for c in (0, count - 1) for j in sample)
        if first_msg is None:
            first_msg = msg
        t_es = median_time(lambda: S.encrypt_batch_seeded(pk[0], pk[1], logQ, 11, 0, vals, out_a, nl), ctx.sync, a.warmup, a.reps)
        t_ec = median_time(lambda: ctx.encrypt_batch_seeded(pk[0], pk[1], logQ, p, 11, 0, msg, out_b, nl), ctx.sync, a.warmup, a.reps)
        same = bool(np.array_equal(out_a.download((count, 2, n, nl)), out_b.download((count, 2, n, nl))))
        emb_bytes = count * 2 * n * 8
        line = json.dumps({
            "workload": "slots_pow2", "p": p, "m": m, "generator": g, "slots": n, "rows": S.rows, "cols": S.cols, "planned_path": planned, "path": S.path,
            "path_name": "direct" if S.path == 0 else "chirp, %d auxiliary prime(s)" % S.path, "logQ": logQ, "chain_primes": len(primes),
            "count": count, "warmup": a.warmup, "reps": a.reps,
            "embeds_per_s": round(count / t_emb[0], 1), "embed_ms": [round(x * 1e3, 3) for x in t_emb],
            "decodes_per_s": round(count / t_dec[0], 1), "decode_ms": [round(x * 1e3, 3) for x in t_dec],
            "encrypt_slots_per_s": round(count / t_es[0], 1), "encrypt_slots_ms": [round(x * 1e3, 3) for x in t_es],
            "encrypt_coeffs_per_s": round(count / t_ec[0], 1), "encrypt_coeffs_ms": [round(x * 1e3, 3) for x in t_ec],
            "encrypt_slots_over_coeffs_time": round(t_es[0] / t_ec[0], 3), "fused_equals_embed_then_encrypt": same, "parity": parity,
            "paths_agree": bool(np.array_equal(msg, first_msg)),
            "roofline": {"embed_algorithmic_bytes": emb_bytes, "embed_GBps": round(emb_bytes / t_emb[0] / 1e9, 2), "bound": "unknown"},
            "loadavg": [round(x, 2) for x in os.getloadavg()],
        })
        print(line, flush=True)
        out_lines.append(line)
    S.close()


def basis_case(a, m, K, out_lines):
    g, logQ, count = 3, a.logQ, a.count
    primes, bits = [], 1
    while len(primes) < K:                # the plan's primes: the largest below 2^prime_bits, descending
        primes = F.slots_basis_plan(m, bits, a.prime_bits, g)["primes"]
        bits += 8
    primes = primes[:K]
    chain, roots = P.chain_for(m, logQ, max(primes))
    ctx = F.Context(m, chain, roots)
    B = F.SlotBasis.pow2(ctx, primes, g)
    n, L, nl = B.total, B.limbs, (logQ + 63) // 64
    rng = np.random.default_rng(m + K)
    # signed values of L limbs inside (-P/2, P/2): uniform low limbs, the top limb below the top limb of P/2
    top = ((B.modulus - 1) // 2) >> (64 * (L - 1))
    limbs = rng.integers(-(1 << 63), (1 << 63) - 1, size=(count, n, L), dtype=np.int64, endpoint=True)
    limbs[..., L - 1] = rng.integers(-top + 1, top - 1, size=(count, n), dtype=np.int64, endpoint=True)
    d_vals, d_msg, d_back = ctx.upload(limbs), ctx.alloc(K * count * n * 8), ctx.alloc(count * n * L * 8)
    t_emb = median_time(lambda: B.embed_dev(d_vals, L, n, count, d_msg), ctx.sync, a.warmup, a.reps)
    t_dec = median_time(lambda: B.decode_dev(d_msg, count, n, d_back), ctx.sync, a.warmup, a.reps)
    parity = bool(np.array_equal(d_back.download((count, n, L), np.int64), limbs))
    rows = P.rand_rows(rng, chain, n, 2)
    pk = []
    for r in range(2):
        d = F.DoubleCRT(ctx)
        for i in range(len(chain)):
            d.set_row(i, np.ascontiguousarray(rows[r, i]))
        pk.append(d)
    words = count * 2 * n * nl
    out_a, out_b = ctx.alloc(K * words * 8), ctx.alloc(K * words * 8)
    red = []                               # the residues the single-prime calls take, by Horner over the limbs on the host (outside the clock)
    for p in primes:
        r = (limbs[..., L - 1] % p).astype(np.uint64)
        for l in range(L - 2, -1, -1):
            r = (r * np.uint64((1 << 64) % p) + limbs[..., l].view(np.uint64) % np.uint64(p)) % np.uint64(p)
        red.append(r.astype(np.int64))
    views = [type("View", (), {"ptr": F.binding._vp(out_b.ptr.value + c * words * 8)})() for c in range(K)]

    def singles():
        for c in range(K):
            B.channel(c).encrypt_batch_seeded(pk[0], pk[1], logQ, 11, c * count, red[c], views[c], nl, False)

    t_ei = median_time(lambda: B.encrypt_batch_seeded(pk[0], pk[1], logQ, 11, 0, limbs, out_a, nl), ctx.sync, a.warmup, a.reps)
    t_es = median_time(singles, ctx.sync, a.warmup, a.reps)
    same = bool(np.array_equal(out_a.download((K, count, 2, n, nl)), out_b.download((K, count, 2, n, nl))))
    emb_bytes = count * n * (L + K) * 8
    line = json.dumps({
        "workload": "slots_basis", "m": m, "generator": g, "slots": n, "k": K, "primes": primes, "modulus_bits": B.modulus.bit_length(), "limbs": L, "logQ": logQ,
        "chain_primes": len(chain), "count": count, "warmup": a.warmup, "reps": a.reps,
        "embeds_per_s": round(count / t_emb[0], 1), "embed_ms": [round(x * 1e3, 3) for x in t_emb],
        "decodes_per_s": round(count / t_dec[0], 1), "decode_ms": [round(x * 1e3, 3) for x in t_dec],
        "encrypt_int_per_s": round(count / t_ei[0], 1), "encrypt_int_ms": [round(x * 1e3, 3) for x in t_ei],
        "encrypt_k_singles_per_s": round(count / t_es[0], 1), "encrypt_k_singles_ms": [round(x * 1e3, 3) for x in t_es],
        "encrypt_int_over_k_singles_time": round(t_ei[0] / t_es[0], 3), "embed_over_encrypt_int_time": round(t_emb[0] / t_ei[0], 4),
        "channels_equal_single_prime_encryptions": same, "parity": parity,
        "roofline": {"embed_algorithmic_bytes": emb_bytes, "embed_GBps": round(emb_bytes / t_emb[0] / 1e9, 2), "bound": "unknown"},
        "loadavg": [round(x, 2) for x in os.getloadavg()],
    })
    print(line, flush=True)
    out_lines.append(line)
    B.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basis", type=int, default=0, metavar="K", help="integer slots over K primes on the rings of --m")
    ap.add_argument("--prime-bits", type=int, default=31)
    ap.add_argument("--pow2", action="store_true", help="the two-row spaces of power-of-two rings: planned path and forced chirp")
    ap.add_argument("--m", type=int, nargs="+", default=[1 << 15, 1 << 16])
    ap.add_argument("--pow2-p", type=int, default=65537)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--p", type=int, nargs="+", default=[32603, 65543])
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--logQ", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.basis:
        lines = []
        for m in a.m:
            basis_case(a, m, a.basis, lines)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.pow2:
        lines = []
        for m in a.m:
            pow2_case(a, m, a.pow2_p, 3, lines)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    for p in a.p:
        m, logQ, count = p - 1, a.logQ, a.count
        g = M.least_generator(m)
        primes, roots = P.chain_for(m, logQ, p)
        ctx = F.Context(m, primes, roots)
        S = F.SlotSpace(ctx, p, g)
        n, nl = S.total, (logQ + 63) // 64
        rng = np.random.default_rng(p)
        vals = rng.integers(0, p, size=(count, S.usable)).astype(np.int64)
        d_vals, d_msg, d_back = ctx.upload(vals), ctx.alloc(count * n * 8), ctx.alloc(count * S.usable * 8)
        t_emb = median_time(lambda: S.embed_dev(d_vals, S.usable, count, d_msg), ctx.sync, a.warmup, a.reps)
        t_dec = median_time(lambda: S.decode_dev(d_msg, count, S.usable, d_back), ctx.sync, a.warmup, a.reps)
        msg = d_msg.download((count, n), np.int64)
        back = d_back.download((count, S.usable), np.int64)
        mod = M.slot_space(m, p, g)
        sample = [0, 1, S.usable - 1]
        parity = bool(np.array_equal(back, vals)) and all(M.decode_slot(mod, [int(x) for x in msg[c]], j) == vals[c, j] for c in (0, count - 1) for j in sample)
        pk = []
        rows = P.rand_rows(rng, primes, n, 2)
        for r in range(2):
            d = F.DoubleCRT(ctx)
            for i in range(len(primes)):
                d.set_row(i, np.ascontiguousarray(rows[r, i]))
            pk.append(d)
        out_a, out_b = ctx.alloc(count * 2 * n * nl * 8), ctx.alloc(count * 2 * n * nl * 8)
        t_es = median_time(lambda: S.encrypt_batch_seeded(pk[0], pk[1], logQ, 11, 0, vals, out_a, nl), ctx.sync, a.warmup, a.reps)
        t_ec = median_time(lambda: ctx.encrypt_batch_seeded(pk[0], pk[1], logQ, p, 11, 0, msg, out_b, nl), ctx.sync, a.warmup, a.reps)
        same = bool(np.array_equal(out_a.download((count, 2, n, nl)), out_b.download((count, 2, n, nl))))
        emb_bytes = count * (S.usable + n) * 8
        print(json.dumps({
            "workload": "slots", "p": p, "m": m, "generator": g, "slots": n, "usable": S.usable, "aux_primes": S.aux_primes, "logQ": logQ, "chain_primes": len(primes),
            "count": count, "warmup": a.warmup, "reps": a.reps,
            "embeds_per_s": round(count / t_emb[0], 1), "embed_ms": [round(x * 1e3, 3) for x in t_emb],
            "decodes_per_s": round(count / t_dec[0], 1), "decode_ms": [round(x * 1e3, 3) for x in t_dec],
            "encrypt_slots_per_s": round(count / t_es[0], 1), "encrypt_slots_ms": [round(x * 1e3, 3) for x in t_es],
            "encrypt_coeffs_per_s": round(count / t_ec[0], 1), "encrypt_coeffs_ms": [round(x * 1e3, 3) for x in t_ec],
            "encrypt_slots_over_coeffs_time": round(t_es[0] / t_ec[0], 3), "fused_equals_embed_then_encrypt": same, "parity": parity,
            "roofline": {"embed_algorithmic_bytes": emb_bytes, "embed_GBps": round(emb_bytes / t_emb[0] / 1e9, 2), "bound": "unknown"},
            "loadavg": [round(x, 2) for x in os.getloadavg()],
        }), flush=True)
        S.close()


if __name__ == "__main__":
    main()
