"""CPU (no GPU): the Paterson-Stockmeyer planner and schedule of fhe-si_amd/csrc/poly_plan.h as the stand-alone program tests/host/poly_plan_check.cpp
runs them on the host under AddressSanitizer + UndefinedBehaviorSanitizer, against the model (tests/poly_model.py).  The cases are drawn here; the
program reads them from standard input and prints one line per case."""
import os
import random
import subprocess

import pytest

import poly_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-C", HOST, "-f", "poly_plan.mk", "poly_plan_check"], stdout=subprocess.DEVNULL)

    def run(cases):
        """cases: [(input line, expected line)]"""
        text = "\n".join(line for line, _ in cases) + "\n"
        r = subprocess.run([os.path.join(HOST, "poly_plan_check")], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        got = r.stdout.splitlines()
        assert len(got) == len(cases)
        for (line, want), g in zip(cases, got):
            assert g.split() == want.split(), line[:300]
    return run


def rendered(s):
    """the model's schedule as the program prints the header's: pool entries for the powers, the inner sums behind them, W behind those"""
    B, G = s["B"], s["G"]
    npowers, where = B + G - 2, {g: B + G - 2 + i for i, (g, _, _) in enumerate(s["inner"])}
    out = [f"{B} {G} {npowers} {len(s['inner'])}"]
    for level in s["levels"]:
        out.append("L " + " ".join(f"{PM.pool_entry(k, B)} {PM.pool_entry(a, B)} {PM.pool_entry(b, B)}" for k, a, b in level))
    for g, terms, konst in s["inner"]:
        out.append(f"I {g} {konst} " + " ".join(f"{c} {PM.pool_entry(j, B)}" for c, j in terms))
    assert [g for g, _ in s["pairs"]] == list(where) and all(k == g * B for g, k in s["pairs"])
    terms, konst = s["final"]
    out.append(f"F {konst} " + " ".join(f"{c} {npowers + len(s['inner']) if ref[0] == 'W' else PM.pool_entry(ref[1], B)}" for c, ref in terms))
    return " | ".join(out)


def test_planner_equals_the_model(check):
    cases = []
    for d in list(range(1, 300)) + [1024, 4095, 4096]:
        for baby in sorted({0, 1, min(3, d), d}):
            c = PM.plan(d, baby)
            cases.append((f"plan {d} {baby}", f"{c['B']} {c['G']} {c['nprod']} {c['nks']} {c['depth']}"))
    check(cases)


def test_schedule_equals_the_model(check):
    rng, cases = random.Random(7), []
    for p in (2, 257, 65537, (1 << 61) - 1):
        for d in list(range(1, 34)) + [64, 255]:
            dense = [rng.randrange(-3 * p, 3 * p) for _ in range(d + 1)]
            special = [0, p - 1, p, -1, -p, 1 << 62, -(1 << 62), (1 << 63) - 1, -(1 << 63), p // 2, p // 2 + 1]
            for i, v in zip(rng.sample(range(d + 1), min(d + 1, len(special))), special):
                dense[i] = v
            sparse = [c if rng.random() < 0.4 else 0 for c in dense]
            for coef in (dense, sparse, dense[:d] + [p], [0] * (d + 1), [0] * d + [1]):
                for baby in sorted({0, 1, min(3, d), d} | ({rng.randrange(1, d + 1)})):
                    cases.append((f"sched {p} {baby} {d} " + " ".join(map(str, coef)), rendered(PM.schedule(coef, p, baby))))
    check(cases)
