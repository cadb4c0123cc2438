"""GPU: the data-file regression driver on a power-of-two ring (tests/host/test_regression_pow2.cpp): m = 4096 / 8192, p = 65537, two rows of
m / 4 slots.  LoadData -> BatchData -> AddDataSlots -> RegressBatched (unmasked and masked) -> DecryptSlotsBatch; slot 0 of theta / det equals
the integer regression modulo p, the unmasked total sits in every slot, the masks replace all but slot 0.  More rows than one ciphertext holds."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
EXE = os.path.join(HOST, "test_regression_pow2")


def run(tmp_path, m, p, g, dim, nrows, seed, *extra):
    # the driver has its own makefile next to the harness's (same flags and link line): built here on first use
    subprocess.check_call(["make", "-C", HOST, "-f", "regression_pow2.mk", "test_regression_pow2"], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, str(m), str(p), str(g), str(dim), str(nrows), str(tmp_path / "data.txt"), str(seed), *extra], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    for line in ("two rows of m / 4 columns, every slot usable: yes", "BatchData plaintexts decode to the data: yes",
                 "Plaintext >>= 3 rotates both rows left by three, += / -= / == hold: yes", "SwapRows exchanges the rows and equals X -> X^(m-1) on the coefficients: yes",
                 "the exponents of the total sum are g, g^2, g^4, ..., then m - 1: yes", "batched, unmasked: slot 0 equals the integer regression modulo p: yes",
                 "unmasked: the total reaches every slot of both rows: yes", "batched, masked: slot 0 equals the integer regression modulo p: yes"):
        assert line in r.stdout, line
    if dim > 1:
        assert "the masks replace the other slots: yes" in r.stdout
    assert r.stdout.strip().endswith("OK")
    return r.stdout


@pytest.mark.parametrize("m,g,dim,nrows", [(4096, 3, 1, 3000), (4096, 5, 2, 3000), (8192, 3, 2, 5000)])
def test_regression_from_a_data_file_on_a_power_of_two_ring(tmp_path, m, g, dim, nrows):
    out = run(tmp_path, m, 65537, g, dim, nrows, 3)
    assert "blocks=2" in out and "rows=2 cols=%d" % (m // 4) in out


def test_regression_on_a_power_of_two_ring_on_a_loopback_group(tmp_path):
    out = run(tmp_path, 4096, 65537, 3, 2, 3000, 5, "--devices=0,0")
    assert "group of ranks, masked: slot 0 equals the integer regression modulo p: yes" in out
