"""The fast pass of the tensor half's CRT on the int8 matrix cores (crt32_mfma_kernel, kernels_tensor32.hip; option crt32_mfma) and the redo pass
over the list of flagged workgroups.  The kernel is compiled for one shape -- rows of 2^14, logQ = 512: m = 2^15, p = 23 -- so that is the
smallest shape it can go wrong at; the ring, the operands and the oracle's results are those of tests/test_gpu_crt_fold.py, built once.

crt32_mfma = 1 (the default) takes the matrix cores from 128 polynomials per launch on (the operand load per workgroup); the counts here are
1 .. 9, so the tests set 2 (any size) and compare with 0 (crt32_scale_kernel) bit for bit: the two form the same integer F, hence the same limbs,
the same rounding and the same flags, with and without the exact pass behind them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import oracle_lib as O
import params as P
import test_crt32_fold_model as W
import test_gpu_crt_fold as T

LOGQ, PT = T.LOGQ, T.PT
MFMA, VALU = "crt32_mfma_kernel<512>", "crt32_scale_kernel<512, false, 28, 38, 0>"


def device(**options):
    ctx, ksk = T.device()
    for name, v in options.items():
        ctx.set_option(name, v)
    return ctx, ksk


def mul_dev(ctx, ksk, a, b):
    n, nl = a.shape[2], a.shape[3]
    da, db, dout = ctx.upload(a), ctx.upload(b), ctx.alloc(a.nbytes)
    ctx.prof_enable(True)
    ctx.ct_mul_relin_dev(ksk, LOGQ, PT, da, db, dout, nl, a.shape[0])
    ctx.sync()
    crt = ctx.prof_kernel_name("crt")
    ctx.prof_enable(False)
    return dout.download(a.shape), crt


@pytest.mark.gpu
@pytest.mark.parametrize("count,lanes", [(1, 1), (3, 1), (9, 2)])
def test_random_ciphertexts(count, lanes):
    """pairs 1 and 2 of the shared batch hold -2^511 and 2^511 - 1 in every coefficient (the extremes of the centred range)"""
    _, _, _, _, a, b, *_ = T.ring()
    ctx, ksk = device(crt32_mfma=2, lanes=lanes)
    got, crt = mul_dev(ctx, ksk, a[:count], b[:count])
    assert crt == MFMA, crt
    ref_ctx, ref_ksk = device(crt32_mfma=0, lanes=lanes)
    ref, crt0 = mul_dev(ref_ctx, ref_ksk, a[:count], b[:count])
    assert crt0 == VALU, crt0
    for c in [c for c in T.ORACLE_CHECKED if c < count]:
        assert np.array_equal(ref[c], T.want(c)), ("crt32_mfma = 0", c)
        assert np.array_equal(got[c], T.want(c)), ("crt32_mfma = 2", c)
    assert np.array_equal(got, ref)


@pytest.mark.gpu
def test_default_takes_the_matrix_cores_from_128_polynomials_on():
    """43 products = 129 polynomials: the default option; 3 products keep crt32_scale_kernel (tests/test_gpu_crt_fold.py pins that name)"""
    _, _, _, _, a, b, *_ = T.ring()
    ctx, ksk = device()
    assert ctx.get_option("crt32_mfma") == 1
    idx = np.arange(43) % T.COUNT
    got, crt = mul_dev(ctx, ksk, a[idx], b[idx])
    assert crt == MFMA, crt
    for k in (0, 1, 2, 24, 25, 26, 27, 42):
        assert np.array_equal(got[k], T.want(int(idx[k])) if int(idx[k]) in T.ORACLE_CHECKED else got[int(idx[k])]), k
    _, crt = mul_dev(ctx, ksk, a[:3], b[:3])
    assert crt == VALU, crt


@pytest.mark.gpu
def test_rounding_edges_same_raw_output_and_same_flags():
    """the crafted pairs of tests/test_gpu_crt_fold.py: without the exact pass both kernels misround the same coefficients (the same F); with it
    both equal the oracle -- the redo pass saw the same flags"""
    _, _, orc, ksm, *_ = T.ring()
    pairs = [T.crafted_pair(W.NEW_ONES + W.NEW_CROSS, 1), T.crafted_pair(W.OLD_DELTAS, 2)]
    a, b = np.stack([pr[0] for pr in pairs]), np.stack([pr[1] for pr in pairs])
    exp = np.stack([orc.ct_mul_relin(ksm, a[c], b[c], LOGQ, PT) for c in range(2)])
    out = {}
    for mode in (2, 0):
        ctx, ksk = device(crt32_mfma=mode)
        full, crt = mul_dev(ctx, ksk, a, b)
        assert crt == (MFMA if mode else VALU), crt
        ctx.set_option("crt_skip_cleanup", 1)
        raw, _ = mul_dev(ctx, ksk, a, b)
        out[mode] = (full, raw)
    assert np.array_equal(out[2][1], out[0][1]), "the fast passes alone differ"
    assert not np.array_equal(out[2][1][0], exp[0]) and not np.array_equal(out[2][1][1], exp[1]), "the crafted inputs must need the exact pass"
    assert np.array_equal(out[2][0], exp) and np.array_equal(out[0][0], exp)


@pytest.mark.gpu
def test_primes_below_2_29():
    """36 primes: kappa and the constant move one slot up in the last depth step"""
    _, _, _, _, a, b, *_ = T.ring()
    ctx, ksk = device(crt32_mfma=2, tensor_bits=29)
    got, crt = mul_dev(ctx, ksk, a[:3], b[:3])
    assert crt == MFMA, crt
    for c in range(3):
        assert np.array_equal(got[c], T.want(c)), c


@pytest.mark.gpu
def test_generic_shape_keeps_its_kernel():
    """m = 1006, logQ = 512: zero-padded rows, the generic kernel, whatever the option says"""
    m, logQ, p, count = 1006, 512, 23, 2
    primes, roots = P.chain_for(m, logQ, p)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    ctx.set_option("crt32_mfma", 2)
    n, nd, nl = ctx.phim, R.ndigits(logQ), (logQ + 63) // 64
    rng = np.random.default_rng(1006)
    ksm = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)])
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    a = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (count, 2, n), nl, logQ)
    da, db, dout = ctx.upload(a), ctx.upload(b), ctx.alloc(a.nbytes)
    ctx.prof_enable(True)
    ctx.ct_mul_relin_dev(ksk, logQ, p, da, db, dout, nl, count)
    ctx.sync()
    assert ctx.prof_kernel_name("crt") == "crt32_scale_generic_kernel<24, false, 0, 1>", ctx.prof_kernel_name("crt")
    ctx.prof_enable(False)
    got = dout.download((count, 2, n, nl))
    for c in range(count):
        assert np.array_equal(got[c], orc.ct_mul_relin(ksm, a[c], b[c], logQ, p)), c


def worklist_batch():
    """two ciphertexts with rounding-edge coefficients in several workgroups of BOTH crafted components: a0 b0 = p A in component 0 and
    a1 b1 = p A' in component 2 (b0 = b1 = 1), so component 1 = a0 + a1 carries edge-free sums"""
    n, nl = T.ring()[6], T.ring()[8]
    a = np.zeros((2, 2, n, nl), dtype=np.uint64)
    b = np.zeros((2, 2, n, nl), dtype=np.uint64)
    for c, (d0, d1) in enumerate(((W.NEW_ONES + W.NEW_CROSS, W.OLD_DELTAS), (W.OLD_DELTAS, W.NEW_ONES))):
        for part, deltas in ((0, d0), (1, d1)):
            v = [0] * n
            for k, x in enumerate(W.crafted(deltas, PT)):
                v[(k * 1021 + 5 + 300 * part + 77 * c) % n] = x
            a[c, part] = O.ints_to_limbs(v, nl)
            b[c, part] = O.ints_to_limbs([1] + [0] * (n - 1), nl)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 0], ids=["mfma", "valu"])
def test_redo_list_over_several_flagged_workgroups(mode):
    """more than one flagged workgroup in two polynomials of each of two ciphertexts: the redo pass walks the list both fast passes write.
    FHESI_AB_LIB (optional: a build of the parent commit, whose redo pass runs over the full grid) is compared in a child process."""
    _, _, orc, ksm, *_ = T.ring()
    a, b = worklist_batch()
    exp = np.stack([orc.ct_mul_relin(ksm, a[c], b[c], LOGQ, PT) for c in range(2)])
    ctx, ksk = device(crt32_mfma=mode)
    got, _ = mul_dev(ctx, ksk, a, b)
    assert np.array_equal(got, exp)
    ctx.set_option("crt_skip_cleanup", 1)
    raw, _ = mul_dev(ctx, ksk, a, b)
    assert not np.array_equal(raw[0], exp[0]) and not np.array_equal(raw[1], exp[1]), "both ciphertexts must need the redo pass"
    ab = os.environ.get("FHESI_AB_LIB")
    if ab and mode:
        code = ("import sys, numpy as np; sys.path[:0] = %r; import test_gpu_crt32_mfma as X; a, b = X.worklist_batch(); ctx, ksk = X.T.device(); "
                "np.save(sys.argv[1], ctx.ct_mul_relin(ksk, X.LOGQ, X.PT, a, b))" % [p for p in sys.path if p])
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "crt32_mfma_ab_%d.npy" % os.getpid())
        subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, FHESI_LIB=ab), timeout=600)
        assert np.array_equal(np.load(path), got)
        os.remove(path)
