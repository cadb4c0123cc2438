"""GPU: FHESISecKey::NoiseBudget / NoiseBudgetBatch on the C++ mirror (tests/host/test_noise.cpp): the budget of a ciphertext in HBM (recording
on), of the same ciphertext uploaded for the call (recording off) and from toPoly in ZZ are one number -- fresh, after a multiplication, and on a
recorded product nobody looked at before the call."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
EXE = os.path.join(HOST, "test_noise")


@pytest.mark.parametrize("m,logQ,p,g", [(64, 100, 257, 3), (46, 90, 47, 5)])
def test_noise_budget_on_the_mirror(m, logQ, p, g):
    # the program has its own makefile next to the harness's (same flags and link line): built here on first use
    subprocess.check_call(["make", "-C", HOST, "-f", "noise.mk", "test_noise"], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, str(m), str(logQ), str(p), str(g)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout and r.stdout.count("  ok   ") == 10
    for line in ("NoiseBudget equals NoiseBudgetBatch with recording on", "... equals the budget from toPoly in ZZ",
                 "a recorded product that was not looked at before the call has the budget of the same product evaluated"):
        assert line in r.stdout, line
    assert r.stdout.strip().endswith("OK")
