#!/usr/bin/env python3
"""Generates tests/golden/noise.json: a key, three two-part ciphertexts and their noise (maximal decryption residual, budget) at m = 64, p = 257,
logQ = 100.  Run from the repo root:  python tests/golden/gen_noise.py

The expected values are NOT taken from tests/noise_model.py, which tests/test_noise_model.py compares with this file: z = c0 + c1 t is formed
here by the schoolbook negacyclic product modulo X^32 + 1 in Python integers (no transform, no CRT), the residual straight from its definition
r = (2 p z + q) mod 2q - q."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import fhesi_pyref as R  # noqa: E402

M, P, LOGQ = 64, 257, 100


def negacyclic(a, b, n):
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] += x * y
            else:
                out[i + j - n] -= x * y
    return out


def main():
    _, n = R.zms_idx(M)
    primes = R.add_primes_by_size(M, R.si_context_size(LOGQ, P, n))
    roots = [R.find_root_2m(q, M) for q in primes]
    ctx = R.Ctx(M, LOGQ, P, primes, roots)
    rng = R.SplitMix64(20261018)
    q = 1 << LOGQ
    t, pk = R.keygen(ctx, rng)
    msg = [rng.bnd(P) for _ in range(n)]
    fresh = R.encrypt(ctx, pk, msg, rng)                                                  # a valid encryption: a large budget
    uniform = [R.sample_random(rng, q, n), R.sample_random(rng, q, n)]                   # no structure: residuals all over [-q, q)
    inv = pow(P, -1, q)
    crafted = [[R.reduce_logq(inv * (r // 2), LOGQ) for r in [2, -(1 << 64), (1 << 64) - 2] + [0] * (n - 3)], [0] * n]      # max |r| = 2^64 exactly
    cases = []
    for parts in (fresh, uniform, crafted):
        z = [a + b for a, b in zip(parts[0], negacyclic(parts[1], t, n))]
        res = [(2 * P * c + q) % (2 * q) - q for c in z]
        mx = max(abs(r) for r in res)
        cases.append({"parts": [[str(c) for c in part] for part in parts], "maxres": str(mx), "budget": max(0, LOGQ - mx.bit_length()),
                      "message": [((2 * P * c + q) // (2 * q)) % P for c in z]})
    assert cases[0]["message"] == msg and cases[0]["budget"] > 60 and cases[2]["maxres"] == str(1 << 64) and cases[2]["budget"] == LOGQ - 65
    obj = {"m": M, "p": P, "logQ": LOGQ, "primes": [str(x) for x in primes], "roots": [str(x) for x in roots], "t": t, "cases": cases}
    path = os.path.join(HERE, "noise.json")
    with open(path, "w") as f:
        json.dump(obj, f, separators=(",", ":"))
    print("wrote noise.json", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
