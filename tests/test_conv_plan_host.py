"""CPU (no GPU): the convolution plan, its refusals and the index lists of the plaintext sum of fhe-si_amd/csrc/conv_plan.h as the stand-alone program
tests/host/conv_plan_check.cpp runs them on the host under AddressSanitizer + UndefinedBehaviorSanitizer, against the model (tests/conv_model.py).  The
cases are drawn here; the program reads them from standard input and prints one line per case."""
import os
import random
import subprocess

import pytest

import conv_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-C", HOST, "-f", "conv_plan.mk", "conv_plan_check"], stdout=subprocess.DEVNULL)

    def run(cases):
        """cases: [(input line, expected line)]; an expected line "refused <word>" asks for the word anywhere in the condition"""
        text = "\n".join(line for line, _ in cases) + "\n"
        r = subprocess.run([os.path.join(HOST, "conv_plan_check")], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        got = r.stdout.splitlines()
        assert len(got) == len(cases)
        for (line, want), g in zip(cases, got):
            if want.startswith("refused "):
                assert g.startswith("refused ") and want[len("refused "):] in g, (line, g)
            else:
                assert g.split() == want.split(), (line, g[:300])
    return run


def rendered(args):
    word = CM.refused(*args)
    if word is not None:
        return "refused " + word
    pl = CM.plan(*args)
    return f"{pl['form']} {pl['nh']} {pl['key_switches']} {pl['terms']} " + " ".join(map(str, pl["amounts"]))


def test_plan_and_refusals_equal_the_model(check):
    cases = []
    for cols, H, W in [(16, 4, 4), (16, 2, 4), (16, 4, 2), (16, 2, 8), (16, 1, 16), (16, 16, 1), (16, 2, 2), (16, 1, 1), (1024, 32, 32), (1024, 2, 4), (256, 8, 8),
                       (16, 3, 4), (16, 8, 4), (0, 1, 1), ((1 << 20) + 1, 1, 1), (16, 0, 4), (16, 4, -1)]:
        for kh in range(0, 8):
            for kw in range(0, 8):
                for ah, aw in sorted({(0, 0), ((kh - 1) // 2, (kw - 1) // 2), (kh - 1, kw - 1), (kh, 0), (0, -1)}):
                    for Cin, Cout in ((1, 1), (2, 3), (3, 2)):
                        for form in (0, 1, 2):
                            args = (cols, H, W, Cin, Cout, kh, kw, ah, aw, form)
                            cases.append(("plan " + " ".join(map(str, args)), rendered(args)))
    # what only the counts decide: channels, the rows of one handle, the form, sizes no product of which may leave 64 bits
    for args in [(1024, 32, 32, 0, 1, 3, 3, 1, 1, 0), (1024, 32, 32, 1, 0, 3, 3, 1, 1, 0), (1024, 32, 32, 86, 86, 3, 3, 1, 1, 0), (1024, 32, 32, 85, 85, 3, 3, 1, 1, 0),
                 (1024, 32, 32, 65536, 1, 1, 1, 0, 0, 0), (1024, 32, 32, 1 << 40, 1 << 40, 1, 1, 0, 0, 0), (1024, 32, 32, 1, 1, 3, 3, 1, 1, 3), (1024, 32, 32, 1, 1, 3, 3, 1, 1, -1),
                 (1024, 32, 32, 1, 1, 1 << 62, 1 << 62, 1 << 61, 1 << 61, 0), (1024, 1 << 40, 1 << 40, 1, 1, 1, 1, 0, 0, 0), (1024, 32, 32, 1, 1, 63, 63, 31, 31, 0),
                 (1024, 32, 32, 4, 4, 3, 3, 1, 1, 0), (1024, 32, 32, 1, 8, 3, 3, 1, 1, 0), (1024, 32, 32, 8, 1, 3, 3, 1, 1, 0)]:
        cases.append(("plan " + " ".join(map(str, args)), rendered(args)))
    assert sum(want.startswith("refused") for _, want in cases) > 1000 and sum(not want.startswith("refused") for _, want in cases) > 1000
    check(cases)


def test_sum_lists_equal_the_model(check):
    rng, cases = random.Random(11), []
    shapes = [(1, 1, 1, 1, 1), (3, 2, 9, 9, 1), (3, 2, 9, 3, 3), (1, 1, 5, 2, 3), (2, 2, 7, 3, 3), (1, 3, 4, 1, 4), (2, 1, 6, 8, 1)]
    for _ in range(40):
        nk, B = rng.randrange(1, 30), rng.randrange(1, 12)
        shapes.append((rng.randrange(1, 5), rng.randrange(1, 5), nk, B, -(-nk // B)))
    for nI, nJ, nk, B, G in shapes:
        for cnt in (1, 3):
            a, b, seg = CM.sum_lists(nI, nJ, nk, B, G, cnt)
            assert len(a) == nI * nJ * nk * cnt and len(seg) == nI * G * cnt + 1
            cases.append((f"lists {nI} {nJ} {nk} {B} {G} {cnt}", f"{len(a)} {len(seg) - 1} | " + " ".join(map(str, a)) + " | " + " ".join(map(str, b)) + " | " + " ".join(map(str, seg))))
    check(cases)
