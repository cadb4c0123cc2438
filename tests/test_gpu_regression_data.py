"""GPU: the reference's Test_Regression driver end to end on the C++ mirror (tests/host/test_regression_data.cpp): a data file in the
reference's format -> LoadData -> BatchData -> AddDataSlots -> RegressBatched masked with GenerateNoise -> DecryptSlotsBatch, and slot 0 of
theta / det equals the integer regression adj(X^T X) X^T y, det(X^T X) modulo p.  More rows than one batch holds, and not a multiple of it."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
EXE = os.path.join(HOST, "test_regression_data")


def run(tmp_path, *args):
    # the driver has its own makefile next to the harness's (same flags and link line): built here on first use
    subprocess.check_call(["make", "-C", HOST, "-f", "regression_data.mk", "test_regression_data"], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, *args[:4], str(tmp_path / "data.txt"), *args[4:]], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "BatchData plaintexts decode to the data: yes" in r.stdout
    assert "batched, masked: slot 0 equals the integer regression modulo p: yes" in r.stdout
    assert r.stdout.strip().endswith("OK")
    return r.stdout


@pytest.mark.parametrize("p,g,dim,nrows", [(2027, 3, 1, 700), (2027, 3, 2, 700), (2027, 3, 3, 1100), (8423, 7, 2, 5000)])
def test_regression_from_a_data_file(tmp_path, p, g, dim, nrows):
    out = run(tmp_path, str(p), str(g), str(dim), str(nrows), "3")
    assert "blocks=%d" % (2 if p == 8423 or nrows == 700 else 3) in out
    if dim > 1:
        assert "the masks replace the other slots: yes" in out


def test_regression_from_a_data_file_object_at_a_time_and_on_a_loopback_group(tmp_path):
    out = run(tmp_path, "2027", "3", "2", "700", "5", "--literal", "--devices=0,0")
    assert "object at a time, masked: slot 0 equals the integer regression modulo p: yes" in out
    assert "group of ranks, masked: slot 0 equals the integer regression modulo p: yes" in out
