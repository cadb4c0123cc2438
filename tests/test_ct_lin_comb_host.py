"""CPU (no GPU): the scalar linear combination of the coefficient-domain ciphertext kernels (ctw_lin_comb in fhe-si_amd/csrc/ct_wide.h: what one thread of
ct_lin_comb_kernel computes) behind the host's term lists (lin_comb_lists, fhe-si_amd/csrc/poly_plan.h), as the stand-alone program
tests/host/ct_lin_comb_check.cpp runs them on the host under AddressSanitizer + UndefinedBehaviorSanitizer, against Python integers.

Every limb class of the launcher (2, 8, 16, 32) with nl at both ends of the class; logQ at 64 nl, 64 nl - 1, 64 (nl - 1) + 1 and in between -- where the
scaled constant has limbs above the class, which the quotient must drop; operands of all ones, the extremes of the centred range, 0 and random;
coefficients 0, +-1, p - 1, +-2^62 and the extremes of a machine word; no term, one term, 40 terms, a term twice; constants 0, p - 1, p, -1, -p."""
import os
import random
import subprocess

import pytest

from test_ct_wide import HOST, W, limbs, logqs, operands, stored

CLASSES = (2, 8, 16, 32)
SHAPES = sorted({(M, nl) for i, M in enumerate(CLASSES) for nl in {CLASSES[i - 1] + 1 if i else 1, M}})


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-C", HOST, "-f", "ct_lin_comb.mk", "ct_lin_comb_check"], stdout=subprocess.DEVNULL)

    def run(cases):
        """cases: [(input line, expected words)]"""
        text = "\n".join(line for line, _ in cases) + "\n"
        r = subprocess.run([os.path.join(HOST, "ct_lin_comb_check")], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        got = [[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()]
        assert len(got) == len(cases)
        for (line, want), g in zip(cases, got):
            assert g == want, line[:300]
    return run


def case(M, nl, logQ, p, konst, terms):
    """terms [(coef, a)]; konst None: no constant"""
    total = sum(c * a_signed for c, a_signed in ((c, a - (1 << (64 * nl)) if a >> (64 * nl - 1) else a) for c, a in terms))
    if konst is not None:
        total += (konst << logQ) // p
    line = f"{M} {nl} {logQ} {p} {int(konst is not None)} {konst or 0} {len(terms)} " + " ".join(f"{c} {limbs(a, nl)}" for c, a in terms)
    return line, stored(total, nl, logQ)


def test_linear_combinations_with_a_constant(check):
    rng, cases = random.Random(11), []
    lim = 1 << 63
    for M, nl in SHAPES:
        for logQ in logqs(nl):
            for p in (2, 257, 65537, lim - 25):
                ops = operands(rng, nl, logQ)
                coefs = [0, 1, -1, p - 1, 1 << 62, -(1 << 62), lim - 1, -lim, rng.randrange(-lim, lim)]
                konsts = [None, 0, p - 1, p, -1, -p, lim - 1, -lim]
                cases.append(case(M, nl, logQ, p, None, []))                                   # the zero ciphertext
                for k in konsts[1:]:
                    cases.append(case(M, nl, logQ, p, k, []))                                  # the trivial ciphertext of a constant
                for c in coefs:
                    for a in ops[:4] + ops[6:7]:
                        cases.append(case(M, nl, logQ, p, rng.choice(konsts), [(c, a)]))       # one term
                a = rng.choice(ops)
                cases.append(case(M, nl, logQ, p, rng.choice(konsts), [(rng.choice(coefs), a), (rng.choice(coefs), rng.choice(ops)), (rng.choice(coefs), a)]))
                for signs in ((-1,), (1,), (-1, 1)):                                           # all negative, all positive, mixed
                    terms = [(rng.choice(signs) * rng.randrange(1, lim), rng.choice(ops)) for _ in range(40)]
                    cases.append(case(M, nl, logQ, p, rng.choice(konsts), terms))
    check(cases)
