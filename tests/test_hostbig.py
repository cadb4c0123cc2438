"""CPU (no GPU): the host's big-integer helpers (fhe-si_amd/csrc/hostbig.h: the one set every table builder of the library uses) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_hostbig.cpp), against Python's integers.  Operands:
1, 2 and 45 limbs; 0, 1, 2^64 - 1, 2^(64k) - 1; the most negative two's complement value for bn_mod; shifts by 0, 63, 64 and 65; the products
and (P - 1) / 2 of the first 2, 18 and 45 chain primes below 2^60 (the context's rule: primes 1 mod 2m descending from 2^60, m = 32).  inv_mod (the extended Euclid for any modulus, 0 off the units): every k of
a prime, a prime power, twice a prime power and a power of two, and k = 1, m - 1 and neighbours at m near 2^20."""
import math
import os
import subprocess

import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
WIDTHS = (1, 2, 45)
WORDS = (1, 2, 3, (1 << 64) - 1, (1 << 60) - 93, (1 << 30) - 35)


def operand(v: int, n: int) -> str:
    assert 0 <= v < 1 << (64 * n)
    return f"{n}:{v:x}"


def limbs_hex(v: int, n: int) -> str:
    return f"{v:0{16 * n}x}"


def cases():
    """(operation line, expected output line)"""
    out = []
    prods = []
    primes = P.first_primes(32, 45)[0]
    for k in (2, 18, 45):
        prod = 1
        for q in primes[:k]:
            prod *= q
        prods.append(prod)
    for n in WIDTHS:
        full = (1 << (64 * n)) - 1
        values = sorted({0, 1, (1 << 64) - 1 if n > 1 else 1, full, full >> 1, 1 << (64 * n - 1), (1 << (64 * (n - 1))) - 1 if n > 1 else 0,
                         0x0123456789ABCDEFFEDCBA9876543210 % (full + 1)} | {p for p in prods if p <= full})
        for v in values:
            a = operand(v, n)
            for b in WORDS:
                r = v * b                                # (bn_mul_small trims the product to its significant limbs, at least one)
                out.append((f"mul_small {a} {b}", limbs_hex(r, max(1, (r.bit_length() + 63) // 64))))
                out.append((f"mod_small {a} {b}", str(v % b)))
                signed = v - (1 << (64 * n)) if v >> (64 * n - 1) else v
                out.append((f"mod {a} {b}", str(signed % b)))
            out.append((f"bitlen {a}", str(v.bit_length())))
            out.append((f"half {a}", limbs_hex(v >> 1, n)))
            for s in (0, 63, 64, 65, 64 * n - 1, 64 * n):
                out.append((f"shl {a} {s}", limbs_hex((v << s) & full, n)))
            for w in values:
                out.append((f"sub {a} {operand(w, n)}", limbs_hex((v - w) & full, n)))
                out.append((f"ge {a} {operand(w, n)}", str(int(v >= w))))
        # operands of two widths: the narrower one counts as zero-extended
        out.append((f"sub {operand(full, n)} {operand(1, 1)}", limbs_hex(full - 1, n)))
        out.append((f"ge {operand(1, 1)} {operand(full, n)}", str(int(1 >= full))))
        out.append((f"ge {operand(full, n)} {operand((1 << 64) - 1, 1)}", "1"))
    for k, prod in zip((2, 18, 45), prods):
        n = (prod.bit_length() + 63) // 64 + 1          # the CRT tables' width: one spare limb
        acc = 1
        for q in primes[:k]:                             # the product, one prime at a time
            out.append((f"mul_small {operand(acc, max(1, (acc.bit_length() + 63) // 64))} {q}", limbs_hex(acc * q, ((acc * q).bit_length() + 63) // 64)))
            acc *= q
        out.append((f"half {operand(prod, n)}", limbs_hex((prod - 1) // 2, n)))
        out.append((f"bitlen {operand(prod, n)}", str(prod.bit_length())))
        for q in primes[:3] + primes[k - 1:k]:
            out.append((f"mod_small {operand(prod // q, n)} {q}", str(prod // q % q)))
            out.append((f"mod {operand((1 << (64 * n)) - (prod - 1) // 2, n)} {q}", str(-((prod - 1) // 2) % q)))
            out.append((f"pow64 {q} {n} 1", limbs_hex(sum(pow(2, 64 * j, q) << (64 * j) for j in range(n)), n)))
            out.append((f"pow64 {q} {n} {(1 << 64) - 1}", limbs_hex(sum(((1 << 64) - 1) * pow(2, 64 * j, q) % q << (64 * j) for j in range(n)), n)))
        out.append((f"sub {operand(prod << 3, n)} {operand(prod, n)}", limbs_hex(7 * prod, n)))
        out.append((f"ge {operand(prod, n)} {operand(prod, n - 1)}", "1"))
        out.append((f"ge {operand((prod - 1) // 2, n)} {operand(prod, n)}", "0"))
    for m in (1, 2, 23, 27, 25, 18, 250, 32, 1024):
        for k in range(-2, m + 3):
            out.append((f"inv_mod {k} {m}", str(pow(k, -1, m) if math.gcd(k, m) == 1 and m > 1 else 0)))
    for m in ((1 << 20) - 3, 1 << 20, 1042441, 2 * 3 ** 12, (1 << 20) + 7):      # (1042441 = 1021^2)
        for k in (1, 2, 3, 1021, m - 2, m - 1, m // 2, m // 2 + 1, 5 * m + 1):
            out.append((f"inv_mod {k} {m}", str(pow(k, -1, m) if math.gcd(k, m) == 1 else 0)))
    return out


def test_host_big_integers_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test_hostbig"], stdout=subprocess.DEVNULL)
    cs = cases()
    ops = tmp_path / "ops.txt"
    ops.write_text("".join(line + "\n" for line, _ in cs))
    r = subprocess.run([os.path.join(HOST, "test_hostbig"), str(ops)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(cs)
    wrong = [(line, want, have) for (line, want), have in zip(cs, got) if want != have]
    assert not wrong, wrong[:5]
    assert {line.split()[0] for line, _ in cs} == {"mul_small", "mod_small", "mod", "bitlen", "shl", "sub", "ge", "half", "pow64", "inv_mod"}
