"""CPU: the helpers behind bench.py's roofline record -- what the line says about the binding roof must follow from the committed counter files
by arithmetic a reader can redo (issue ceiling, K2' bytes, min / median over blocks), and must degrade to nulls, not guesses, when the committed
pass is not the run's kernel or batch.  And --dump-outputs: its sample and file format on the CPU, one run against the oracle on the GPU."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B


def test_issue_ceiling_and_bound():
    sq = {"valu_busy": 0.946, "valu_instr_per_wave": 1706.0, "eff_clock_ghz_median": 1.891, "source": "x"}
    f = B.valu_fields(sq, "fwd30", 33.6e6)
    # 2^14-point row: 14 stages x 8192 butterflies = 1792 wave-butterflies of 24 issue cycles on 1024 SIMDs
    assert abs(f["issue_ceiling"]["rows_per_s_at_ceiling"] - 1024 * 1.891e9 / (1792 * 24.0)) < 1.0
    assert f["valu_instr_per_butterfly"] == round(1706.0 / 224, 2) and abs(f["issue_ceiling_frac"] - 33.6e6 / (1024 * 1.891e9 / (1792 * 24.0))) < 1e-3
    assert B.bound_of(0.946) == "valu" and B.bound_of(0.73) == "hbm" and B.bound_of(None) == "hbm"
    none = B.valu_fields(None, "fwd30", 1.0)
    assert none["valu_busy"] is None and none["issue_ceiling_frac"] is None
    # primes below 2^29: 8 of 14 stages without the 6-cycle range step
    assert abs(B.BFLY_ISSUE_CYCLES["fwd29"] - (8 * 18 + 6 * 24) / 14) < 1e-9 and B.BFLY_ISSUE_CYCLES["fwd29"] < B.BFLY_ISSUE_CYCLES["fwd30"]


def test_committed_counter_files_match_the_kernels_of_the_metric_step():
    """profiles/sq_main_kernels.json and profiles/pmc_*.json are what the driver-run line quotes: they must name the kernels the library launches
    today (a renamed template parameter silently turns every field into null) and carry the fields bench.py reads."""
    sq = json.load(open(os.path.join(ROOT, "profiles", "sq_main_kernels.json")))
    assert sq["batch"] == 1024 and len(sq["kernels"]) >= 8
    names = list(sq["kernels"])
    for needle in ("ntt32_fwd_kernel3<true, 0, false, Aux32Primes, true, true, 30>", "ntt32_fwd_kernel3<false, 0, false, T32Primes, true, false, 30>", "dot32_kernel4<7, 6, 12, 3, 8, 1, 6>"):
        assert needle in names, (needle, names)
        k = sq["kernels"][needle]
        assert 0.5 < k["valu_busy"] < 1.1 and k["valu_instr_per_wave"] > 100 and 1.0 < k["eff_clock_ghz_median"] < 2.5
    assert B.offline_sq(names[0], 1024)["source"].startswith("profiles/sq_main_kernels.json") and B.offline_sq(names[0], 64) is None and B.offline_sq("no_such_kernel", 1024) is None
    t, src = B.offline_traffic("pmc_ntt_fwd.json", "ntt32_fwd_kernel3<true, 0, false, Aux32Primes, true, true, 30>", "rows_per_launch", 270336)
    assert t and 2.0e10 < t < 3.0e10 and "pmc_ntt_fwd.json" in src
    assert B.offline_traffic("pmc_ntt_fwd.json", "ntt32_fwd_kernel3<true, 0, false, Aux32Primes, true, true, 30>", "rows_per_launch", 1000) == (None, None)


class _FakeCtx:
    def __init__(self):
        self.t = {"dot": (0, 0.0, 0.0)}

    def prof_read(self, k):
        return self.t[k]


def test_kernel_clock_block_statistics():
    ctx = _FakeCtx()
    clk = B.KernelClock(ctx, ("dot",))
    for launches, ms in ((20, 100.0), (40, 196.0), (60, 300.0)):      # blocks of 20 launches: 5.0, 4.8, 5.2 ms per launch
        ctx.t["dot"] = (launches, float(launches), ms)
        clk.mark()
    assert clk.stats("dot") == (4.8, 5.0)
    clk2 = B.KernelClock(ctx, ("dot",))
    assert clk2.stats("dot") == (None, None)


def _words(path):
    """a --dump-outputs file back as the 64-bit words it holds"""
    f = np.load(path)
    assert f.dtype == np.float32 and f.shape[-1] == 4 and np.array_equal(f, np.floor(f)) and f.min() >= 0 and f.max() < 65536
    return (f.astype(np.uint64) << np.arange(0, 64, 16, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def test_dump_outputs_keeps_every_bit_of_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: the kept word positions are the same in every run and on every rank and bound the run's files to 32 MiB; the float32
    pieces give the words back exactly; a device buffer larger than one 256 MiB piece is fetched piece by piece."""
    assert np.array_equal(B.dump_pick(1000, 8, 1), np.arange(1000))                                      # all of a small output
    pick = B.dump_pick(1 << 18, 1024, 1)
    assert len(pick) == 2048 == len(set(pick)) and np.array_equal(pick, np.sort(pick)) and np.array_equal(pick, B.dump_pick(1 << 18, 1024, 1))
    assert len(B.dump_pick(1 << 18, 1024, 8)) == 256 and 1024 * 8 * 256 * 16 == 1 << 25                  # 8 ranks share the 32 MiB
    rng = np.random.default_rng(3)
    dev = rng.integers(0, 1 << 64, size=(3, 1 << 24), dtype=np.uint64)                                   # 3 items of 128 MiB: pieces of 2 and 1
    dev[0, :3] = (0, 1, (1 << 64) - 1)
    calls = []

    def fake_download_at(ctx, buf, offset, out):
        calls.append((offset, out.shape[0]))
        out[...] = dev.reshape(-1)[offset // 8:offset // 8 + out.size].reshape(out.shape)
    monkeypatch.setattr(B, "download_at", fake_download_at)
    pick = np.concatenate([np.arange(3), B.dump_pick(1 << 24, 3, 1)[:1000]])
    got = B.download_picked(None, None, 3, 1 << 24, pick)
    assert calls == [(0, 2), (1 << 28, 1)] and np.array_equal(got, dev[:, pick])
    args = types.SimpleNamespace(dump_outputs=str(tmp_path / "made" / "here"))
    B.dump_outputs(args, 0, 1, "x", got)
    B.dump_outputs(args, 1, 2, "x", got)
    assert sorted(os.listdir(args.dump_outputs)) == ["x.npy", "x_rank1.npy"]
    assert np.array_equal(_words(os.path.join(args.dump_outputs, "x.npy")), got)


@pytest.mark.gpu
def test_dump_outputs_is_the_timed_buffer_and_repeats(tmp_path):
    """Two runs of bench.py with the same workload arguments write the same file (the inputs are seeded; the number of timed steps does not
    enter), and the file holds the product of the run's inputs: ciphertexts of the batch against the oracle at the kept word positions."""
    n, nl, nd, batch = B.M_RING // 2, (B.LOGQ + 63) // 64, (B.LOGQ + 8 * B.DECOMP - 1) // (8 * B.DECOMP), 16
    got = []
    for tag, steps in (("a", "2"), ("b", "3")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", steps, "--warmup", "1", "--batch", str(batch), "--keys", "uniform",
                            "--cpu-sample", "0", "--no-surface", "--gpu-seconds", "0", "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["steps"] == int(steps)
        assert os.listdir(tmp_path / tag) == ["ct_mul_relin.npy"] and os.path.getsize(tmp_path / tag / "ct_mul_relin.npy") <= 64 << 20
        got.append(_words(tmp_path / tag / "ct_mul_relin.npy"))
    pick = B.dump_pick(2 * n * nl, batch, 1)
    assert got[0].shape == (batch, len(pick)) and len(pick) < 2 * n * nl and np.array_equal(got[0], got[1])
    primes = B.prime_chain(B.M_RING, B.LOGQ, B.P_PLAIN, n)
    roots = [B.root_2m(q, B.M_RING) for q in primes]
    rng = np.random.default_rng(7)
    a = B.rand_coeffs(rng, (batch, 2, n), nl)
    b = B.rand_coeffs(rng, (batch, 2, n), nl)
    ksm = B.rand_residue_rows(np.random.default_rng(8), primes, (2, 3 * nd), n)
    for i in (0, batch - 1):
        want = B.oracle_outputs(primes, roots, ksm, a[i:i + 1], b[i:i + 1], 1)
        assert np.array_equal(got[0][i], want.reshape(-1)[pick]), i
