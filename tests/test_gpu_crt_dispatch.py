"""Every closing kernel of kernels_crt.hip, one row per kernel-selecting branch of its launchers (launch_crt, launch_crt_sum, launch_ks_recombine,
launch_ks_recombine_centred, launch_rns_reduce, launch_modswitch_delta, launch_digits), and the refusals an entry point can reach.  (One refusal of
launch_rns_reduce has no row: "scalar lift only supported on the full prime set" -- no caller passes a scalar together with a prime subset.)

A row names the instantiation the library must record (fhesi_prof_kernel_name: reaching the branch is part of the test, so a dispatch change that
reroutes a shape fails it), the smallest ring and chain that reach the branch, and the entry point that drives it.  Every case is bit-exact: against
the C oracle on the rings it can afford, against the per-prime device path (option ks_direct = 1: what the small rings here and test_gpu_general_m.py
pin to the oracle) above m = 20000.  Inputs: two ciphertexts of random coefficients with the extremes of the centred range at coefficients 0 and
n - 1, and for the key switch the crafted form of ks_crafted.py.

test_every_compiled_instantiation_is_accounted_for (no GPU) lists the instantiations from the library's symbol table: each is named by a row or by
NOT_RUN with its reason, so a kernel added to kernels_crt.hip cannot arrive without a test."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fhe_si_amd as F
import fhesi_pyref as R
import ks_crafted as K
import oracle_lib as O
import params as P

FAMILIES = ("crt_kernel", "crt_sum_kernel", "ks_recombine_kernel", "ks_recombine_generic_kernel", "ks_recombine_centred_kernel", "rns_reduce_kernel",
            "rns_reduce_kernel_t", "modswitch_delta_kernel", "digits_kernel")

# compiled instantiations no row of this file runs
NOT_RUN = {
    "ks_recombine_kernel<34, 1024, 72, 30, true, 0>": "unreachable: the limb plan gives B = 72, NLB = 30 only with n = 2^15 (n = 2^14: B = 73), and on a power-of-two ring with rows of "
                                                      "2^15 ks_recombine_takes_tail always hands this shape to <..., true, 1>",
}

# ---------------------------------------------------------------------------------------------------------------------------------- the table
# (id, {name class: recorded kernel name}, runner, arguments).  Name classes: binding.PROF_CLASSES / PROF_NAMES.
ROWS = []


def row(rid, names, runner, **kw):
    ROWS.append(pytest.param(names, runner, kw, id=rid))


def limbs_of(v: int) -> int:
    return (v.bit_length() + 63) // 64


def crt_bucket(W: int) -> str:
    for mw in (4, 8, 12, 20, 28, 44):
        if W <= mw:
            return f"crt_kernel<{mw}, 0, 0, 0>"
    raise ValueError(W)


M_CHAIN, NPRIMES = 32, 46        # the chain-only branches: n = 16, the first 46 primes below 2^60 (45 of them fill the widest accepted product: 44 limbs)


def chain_count_for_W(W: int) -> int:
    """how many of the first primes give a CRT table of W limbs (product limbs + 1)"""
    primes, _ = P.first_primes(M_CHAIN, NPRIMES)
    return max(k for k in range(1, NPRIMES + 1) if limbs_of(K.chain_product(primes[NPRIMES - k:])) + 1 <= W)


# launch_crt, mode 0 (DoubleCRT::toPoly over an index set), centred and positive: every bucket, both neighbours of every boundary, the widest chain
for _W in (4, 5, 8, 9, 12, 13, 20, 21, 28, 29, 44):
    for _pos in (0, 1):
        row(f"to_poly-W{_W}-positive{_pos}", {"crt_exact": crt_bucket(_W), ("rns_reduce" if _W <= 20 else "rns_generic"): f"rns_reduce_kernel_t<{_W}>" if _W <= 20 else "rns_reduce_kernel"},
            "to_poly", W=_W, positive=_pos)
row("to_poly-18-primes", {"crt_exact": "crt_kernel<18, 18, 18, 0>"}, "to_poly", W=18, positive=0)
row("to_poly-W45-refused", {}, "to_poly", W=45, positive=0)

# launch_rns_reduce: every compile-time limb count, the run-time form past 20 limbs
for _NL in list(range(1, 21)):
    row(f"from_poly-NL{_NL}", {"rns_reduce": f"rns_reduce_kernel_t<{_NL}>"}, "from_poly", NL=_NL)
for _NL in (21, 44):
    row(f"from_poly-NL{_NL}", {"rns_generic": "rns_reduce_kernel"}, "from_poly", NL=_NL)
row("from_poly-NL81-refused", {}, "from_poly", NL=81)
# ... with the `poly * p` lift of Ciphertext::operator*= (fhesi_ct_mul_dev): folded into the power tables, or the residue table of the run-time form
row("ct_mul-lift-NL2", {"rns_reduce": "rns_reduce_kernel_t<2>"}, "ct_mul", NL=2)
row("ct_mul-lift-NL21", {"rns_generic": "rns_reduce_kernel"}, "ct_mul", NL=21)

# launch_crt, modes 1 and 2 (ScaleDown, ReduceCoefficients: fhesi_apply_key_switch_dev on the per-prime form) and mode 3 (the automorphism key switch
# on evaluation rows) over the same chains; `positive` exists for mode 0 only (no entry point passes it with another mode)
for _W in (4, 5, 8, 9, 12, 13, 20, 21, 28, 29, 44):
    row(f"key_switch-W{_W}", {"crt_exact": crt_bucket(_W)}, "ks_small", m=M_CHAIN, W=_W, logQ=100, matrix="uniform", form=0)
    row(f"automorph-W{_W}", {"crt_exact": crt_bucket(_W)}, "automorph", W=_W, logQ=100)
# the compiled chain shapes: 18 primes at logQ = 512 (sum form, its exact clean-up, the exact form alone), 35 primes at logQ = 1024
row("key_switch-18-primes-512", {"crt": "crt_sum_kernel<18, 18, 512, false>", "crt_exact": "crt_kernel<18, 18, 18, 512>"}, "ks_small", m=M_CHAIN, nprimes=18, logQ=512, matrix="uniform", form=0)
row("key_switch-18-primes-512-exact", {"crt": "", "crt_exact": "crt_kernel<18, 18, 18, 512>"}, "ks_small", m=M_CHAIN, nprimes=18, logQ=512, matrix="uniform", form=0, options={"crt_exact": 1})
row("key_switch-18-primes-100", {"crt_exact": "crt_kernel<18, 18, 18, 0>"}, "ks_small", m=M_CHAIN, nprimes=18, logQ=100, matrix="uniform", form=0)
row("automorph-18-primes-512", {"crt": "crt_sum_kernel<18, 18, 512, false>"}, "automorph", nprimes=18, logQ=512)
row("key_switch-35-primes-1024", {"crt": "crt_sum_kernel<35, 34, 1024, false>", "crt_exact": "crt_kernel<35, 35, 34, 1024>"}, "ks_small", m=M_CHAIN, nprimes=35, logQ=1024, matrix="uniform", form=0)
row("key_switch-35-primes-1024-exact", {"crt": "", "crt_exact": "crt_kernel<44, 0, 0, 0>"}, "ks_small", m=M_CHAIN, nprimes=35, logQ=1024, matrix="uniform", form=0, options={"crt_exact": 1})

# launch_modswitch_delta: W = limbs of the dropped primes' product + 2
for _W, _k in ((8, 8), (9, 24), (24, 24), (25, 66), (45, 66)):
    row(f"modswitch-W{_W}", {"modswitch": f"modswitch_delta_kernel<{_k}>"}, "modswitch", W=_W)

# launch_digits: the per-prime form off the power-of-two rings
row("digits-m22", {"digits_kernel": "digits_kernel"}, "ks_small", m=22, logQ=100, matrix="uniform", form=0, options={"ks_direct": 1})

# launch_ks_recombine, two 60-bit auxiliary primes (power-of-two rings of 2^11 .. 2^14 coefficients: the smallest is m = 4096), run-time form.
# The sum form's mode-1 kernel is the last of its class here (the recombination closes the key switch): <..., true>.
row("aux60-W-below-20", {"ks_recombine": "ks_recombine_generic_kernel<20, false>"}, "ks_small", m=4096, logQ=128, matrix="uniform", form=2)
row("aux60-W-above-20", {"ks_recombine": "ks_recombine_generic_kernel<44, false>"}, "ks_small", m=4096, logQ=600, matrix="uniform", form=2)
row("aux60-metric-chain-n2048", {"ks_recombine": "ks_recombine_generic_kernel<20, false>", "crt": "crt_sum_kernel<18, 18, 512, true>"}, "ks_small", m=4096, logQ=512, matrix="uniform", form=2, crafted=False)
# the linear-convolution rings, general limbs (uniform matrix): m = 2Q (fold > 0), odd prime m (fold < 0), prime powers (stride > 1)
row("fold-2q-W-below-20", {"ks_recombine": "ks_recombine_generic_kernel<20, true>"}, "ks_small", m=46, logQ=120, matrix="uniform", form=1)
for _m in (46, 101, 54, 27):
    row(f"fold-m{_m}-W-above-20", {"ks_recombine": "ks_recombine_generic_kernel<44, true>"}, "ks_small", m=_m, logQ=700, matrix="uniform", form=1)
# ... and centred limbs (generated matrix): the run-time forms take the fold on the residues (rows of 2^14: no tail stage)
for _m in (46, 101, 54):
    row(f"centred-fold-m{_m}-logQ200", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 0>"}, "ks_small", m=_m, logQ=200, matrix="generated", form=1)
    row(f"centred-fold-m{_m}-logQ700", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 0>"}, "ks_small", m=_m, logQ=700, matrix="generated", form=1)

# rows of 2^14 without a fold (m = 2^15), generated matrix away from the compiled limb plans
row("centred-m32768-logQ300", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 0>"}, "ks_big", m=1 << 15, logQ=300, centred=True, form=1)
row("centred-m32768-logQ700", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 0>"}, "ks_big", m=1 << 15, logQ=700, centred=True, form=1)
row("centred-m32768-logQ1024", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 0>"}, "ks_big", m=1 << 15, logQ=1024, centred=True, form=1)
# host logic: a generated matrix just above logQ = 1024 keeps the general limbs (ksaux_build never hands launch_ks_recombine_centred more than 1024, so
# its own guard cannot fire) ...
row("generated-m32768-logQ1030", {"ks_recombine": "ks_recombine_generic_kernel<44, true>"}, "ks_big", m=1 << 15, logQ=1030, centred=False, form=1)
# ... and centred limbs exist with the four 30-bit primes only: the same matrix under the two 60-bit primes takes the general limbs
row("generated-m32768-aux60", {"ks_recombine": "ks_recombine_generic_kernel<20, false>"}, "ks_big", m=1 << 15, logQ=300, centred=False, form=2, options={"ks_aux60": 1})
# rows of 2^15 on a linear-convolution ring, left as two sub-inverses: fold and tail stage in the loader
# (m = 16381 and m = 15625 lie below m = 20000 but are held to the per-prime form too: one oracle key switch there is 75 digit columns x 21 chain primes of
#  Bluestein rows of 2^15 points per part, minutes of CPU; the per-prime form is pinned to the oracle on these very rings at logQ = 120 / 128 by
#  test_gpu_pipeline.py::test_key_switch_on_safe_prime_rings[16381-120] and test_gpu_primepower.py::test_mul_relin_on_long_rows[15625-128-True])
row("fold-tail-m16381-logQ300", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 2>"}, "ks_big", m=16381, logQ=300, centred=True, form=1)
row("fold-tail-m32602-logQ300", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 1>"}, "ks_big", m=32602, logQ=300, centred=True, form=1)
row("fold-tail-m16381-logQ600", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 2>"}, "ks_big", m=16381, logQ=600, centred=True, form=1)
row("fold-tail-m32602-logQ600", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 1>"}, "ks_big", m=32602, logQ=600, centred=True, form=1)
row("fold-tail-m15625-logQ600", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 2>"}, "ks_big", m=15625, logQ=600, centred=True, form=1)
# rows of 2^15 without a fold (m = 2^16), generated matrix off the stress limb plan: the run-time forms take the tail stage in their loader (S = 1)
row("centred-tail-m65536-logQ300", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 0>"}, "ks_big", m=1 << 16, logQ=300, p=65537, centred=True, form=1)
row("centred-tail-m65536-logQ700", {"ks_recombine": "ks_recombine_centred_kernel<16, 0, 0, 0, 0>"}, "ks_big", m=1 << 16, logQ=700, p=65537, centred=True, form=1)
# the compiled shapes of the metric and stress rings (the benchmarks' and the older tests' shapes: pinned by name here, so that a dispatch change cannot
# move them to the run-time forms unnoticed); option ks_long_keys cuts the general limbs from the generated matrix
row("metric-general-limbs", {"ks_recombine": "ks_recombine_kernel<18, 512, 74, 15, true, 0>"}, "ks_big", m=1 << 15, logQ=512, centred=False, form=1, options={"ks_long_keys": 1})
row("metric-general-limbs-aux60", {"ks_recombine": "ks_recombine_kernel<18, 512, 74, 15, false, 0>"}, "ks_big", m=1 << 15, logQ=512, centred=False, form=2, options={"ks_aux60": 1})
row("metric-centred-limbs", {"ks_recombine": "ks_recombine_centred_kernel<8, 7, 74, 512, 0>"}, "ks_big", m=1 << 15, logQ=512, centred=True, form=1)
row("stress-general-limbs", {"ks_recombine": "ks_recombine_kernel<34, 1024, 72, 30, true, 1>"}, "ks_big", m=1 << 16, logQ=1024, p=65537, centred=False, form=1, options={"ks_long_keys": 1})
row("stress-centred-limbs", {"ks_recombine": "ks_recombine_centred_kernel<16, 15, 72, 1024, 0>"}, "ks_big", m=1 << 16, logQ=1024, p=65537, centred=True, form=1)
# the stress chain through the two 60-bit auxiliary primes (m = 2^16: the ring whose limb plan is 30 x 72 bits)
row("aux60-stress-chain", {"ks_recombine": "ks_recombine_kernel<34, 1024, 72, 30, false, 0>", "crt": "crt_sum_kernel<35, 34, 1024, true>"}, "ks_big", m=1 << 16, logQ=1024, p=65537,
    centred=False, form=2, options={"ks_aux60": 1})

# More output limbs than the value has (nl_extra: every row above asks for ceil(logQ / 64)): the sign fill beyond bit logQ, and on whole waves
# the direct stores beside the staged path.  One row per store body of kernels_crt.hip (crt_wide.h), at the smallest ring that reaches it.
row("wide-out-runtime-epilogue", {"crt_exact": crt_bucket(4)}, "ks_small", m=M_CHAIN, W=4, logQ=100, matrix="uniform", form=0, nl_extra=1)
row("wide-out-runtime-epilogue-mode3", {"crt_exact": crt_bucket(4)}, "automorph", W=4, logQ=100, nl_extra=1)
row("wide-out-fixed-store", {"crt": "crt_sum_kernel<18, 18, 512, false>", "crt_exact": "crt_kernel<18, 18, 18, 512>"}, "ks_small", m=M_CHAIN, nprimes=18, logQ=512,
    matrix="uniform", form=0, nl_extra=1)
row("wide-out-generic-recombination", {"ks_recombine": "ks_recombine_generic_kernel<20, false>"}, "ks_small", m=4096, logQ=128, matrix="uniform", form=2, nl_extra=1)
row("wide-out-centred", {"ks_recombine": "ks_recombine_centred_kernel<8, 0, 0, 0, 0>"}, "ks_big", m=1 << 15, logQ=300, centred=True, form=1, nl_extra=1)


# ---------------------------------------------------------------------------------------------------------------------------------- runners
@functools.lru_cache(maxsize=None)
def chain_ring():
    primes, roots = P.first_primes(M_CHAIN, NPRIMES)
    return F.Context(M_CHAIN, primes, roots), O.Oracle(M_CHAIN, primes, roots), primes


def check_names(ctx, names):
    """the kernel the last profiled launch of each class ran, spelled exactly ('' = none)"""
    got = {cls: ctx.prof_kernel_name(cls) for cls in names}
    assert got == names, got


def centred_values(rng, n, W, prod):
    """[n][W] limbs: random values of the centred range of `prod`, its extremes (and their neighbours beyond, which wrap) at both ends"""
    h = (prod - 1) // 2
    limbs = P.rand_limbs(rng, (n,), W, prod.bit_length() - 2)
    for j, v in ((0, h), (1, -h), (2, 0), (n - 3, h + 1), (n - 2, -h - 1), (n - 1, -h)):
        limbs[j] = O.ints_to_limbs([v], W)[0]
    return limbs


def run_to_poly(names, W, positive):
    ctx, orc, primes = chain_ring()
    k = chain_count_for_W(W)
    idx = list(range(NPRIMES - k, NPRIMES))            # not a prefix of the chain: the rows are picked through slot_of
    prod = K.chain_product(primes[NPRIMES - k:])
    assert limbs_of(prod) + 1 == W and (k == 18) == (W == 18)
    rng = np.random.default_rng(W)
    limbs = centred_values(rng, ctx.phim, W, prod)
    d = F.DoubleCRT.from_poly(ctx, limbs)
    ctx.prof_enable(True)
    if W > 44:
        with pytest.raises(F.FhesiError, match="exceeds the supported 44"):
            d.to_poly(W, idx, bool(positive))
        ctx.prof_enable(False)
        return
    got = d.to_poly(W, idx, bool(positive))
    check_names(ctx, {c: v for c, v in names.items() if c == "crt_exact"})
    ctx.prof_enable(False)
    rows = orc.dcrt_from_poly(limbs)
    assert np.array_equal(d.rows(), rows)
    assert np.array_equal(got, orc.dcrt_to_poly(rows, W, idx, bool(positive)))
    # the same set as the object's own index set: the input of W limbs through launch_rns_reduce
    ctx.prof_enable(True)
    e = F.DoubleCRT.from_poly(ctx, limbs, index_set=idx)
    check_names(ctx, {c: v for c, v in names.items() if c != "crt_exact"})
    ctx.prof_enable(False)
    assert np.array_equal(e.rows(), rows[idx])
    assert np.array_equal(e.to_poly(W + 1, None, bool(positive)), orc.dcrt_to_poly(rows, W + 1, idx, bool(positive)))      # one limb more: the sign fill


def run_from_poly(names, NL):
    m = 1024                                         # n = 512: two workgroups of 256 coefficients, the second one partly beyond the polynomial
    primes, roots = P.first_primes(m, 3)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    rng = np.random.default_rng(NL)
    ncoeffs = 300
    limbs = P.rand_limbs(rng, (ncoeffs,), NL, 64 * NL)
    lo = -(1 << (64 * NL - 1))
    for j, v in ((0, lo), (1, -lo - 1), (2, -1), (ncoeffs - 2, -lo - 1), (ncoeffs - 1, lo)):
        limbs[j] = O.ints_to_limbs([v], NL)[0]
    ctx.prof_enable(True)
    if NL > 80:                                      # 256 coefficients of the workgroup no longer fit the LDS: refused by the host, nothing launched
        with pytest.raises(F.FhesiError, match="too wide"):
            F.DoubleCRT.from_poly(ctx, limbs)
        assert ctx.prof_kernel_name("rns_generic") == ""
        ctx.prof_enable(False)
        return
    d = F.DoubleCRT.from_poly(ctx, limbs)
    check_names(ctx, names)
    ctx.prof_enable(False)
    assert np.array_equal(d.rows(), orc.dcrt_from_poly(limbs))


def run_ct_mul(names, NL, p=23):
    """the tensor product of two ciphertexts of NL-limb coefficients: DoubleCRT(poly * p) and DoubleCRT(poly) through launch_rns_reduce"""
    primes, roots = P.first_primes(M_CHAIN, 3)
    ctx, orc = F.Context(M_CHAIN, primes, roots), O.Oracle(M_CHAIN, primes, roots)
    n, L = ctx.phim, ctx.L
    a, b = two_ciphertexts(np.random.default_rng(NL), n, NL, 64 * NL)
    tp = ctx.alloc(2 * 3 * L * n * 8)
    ctx.prof_enable(True)
    ctx.ct_mul_dev(p, ctx.upload(a), ctx.upload(b), NL, 2, tp)
    check_names(ctx, names)
    ctx.prof_enable(False)
    got = tp.download((2, 3, L, n))
    for c in range(2):
        assert np.array_equal(got[c], orc.ct_mul(a[c], b[c], p)), c


def two_ciphertexts(rng, n, nl, logQ):
    a = P.rand_limbs(rng, (2, 2, n), nl, logQ)
    b = P.rand_limbs(rng, (2, 2, n), nl, logQ)
    lo, hi = O.ints_to_limbs([-(1 << (logQ - 1))], nl)[0], O.ints_to_limbs([(1 << (logQ - 1)) - 1], nl)[0]
    a[0, 0, 0], a[0, 0, n - 1], a[1, 1, 0], a[1, 1, n - 1] = lo, hi, hi, lo
    b[0, 1, 0], b[0, 1, n - 1], b[1, 0, 0], b[1, 0, n - 1] = hi, lo, lo, lo
    return a, b


def small_chain(m, logQ, p, W, nprimes):
    if W:
        nprimes = chain_count_for_W(W)
    if nprimes:
        primes, roots = P.first_primes(m, nprimes)
        assert not W or limbs_of(K.chain_product(primes)) + 1 == W
        return primes, roots
    return P.chain_for(m, logQ, p, 1, 60)


def generated_like(orc, rng, n, L, ncol, logQ):
    """a matrix shaped like KeySwitchSI::Init's: integer coefficients in [-2^(logQ-1), 2^(logQ-1))"""
    ksm = np.empty((2, ncol, L, n), dtype=np.uint64)
    for r in range(2):
        for c in range(ncol):
            ksm[r, c] = orc.dcrt_from_poly(P.rand_limbs(rng, (n,), L + 2, logQ))
    return ksm


def run_ks_small(names, m, logQ, matrix, form, p=23, W=0, nprimes=0, options=None, crafted=True, nl_extra=0):
    """fhesi_apply_key_switch_dev (ScaleDown = CRT mode 1, then the recombination or the per-prime form's CRT mode 2) against the oracle"""
    primes, roots = small_chain(m, logQ, p, W, nprimes)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    if m > 2000 and m & (m - 1):
        orc.set_bluestein_fft(True)
    n, L, nd, nl = ctx.phim, ctx.L, R.ndigits(logQ), (logQ + 63) // 64 + nl_extra
    for o, v in (options or {}).items():
        ctx.set_option(o, v)
    rng = np.random.default_rng(m + logQ + L)
    prod, Wl = K.chain_product(primes), L + 2
    if matrix == "uniform":
        ksm, edge = np.stack([P.rand_rows(rng, primes, n, 3 * nd) for _ in range(2)]), K.edge_values(prod)
    else:
        ksm, edge = generated_like(orc, rng, n, L, 3 * nd, logQ), K.key_range_values(logQ)
    for r in range(2):
        ksm[r, 0] = orc.dcrt_from_poly(K.edge_limbs(edge, n, Wl, r))
    ksk = F.KeySwitchMatrix(ctx, 3, nd).upload(ksm)
    a, b = two_ciphertexts(rng, n, nl, logQ)
    tp = ctx.alloc(2 * 3 * L * n * 8)
    ctx.ct_mul_dev(p, ctx.upload(a), ctx.upload(b), nl, 2, tp)
    tprod = tp.download((2, 3, L, n))
    out = ctx.alloc(2 * 2 * n * nl * 8)
    ctx.prof_enable(True)
    ctx.apply_key_switch_dev(ksk, logQ, tp, 2, out, nl)
    check_names(ctx, names)
    ctx.prof_enable(False)
    assert ksk.form()[0] == form and ksk.key_bits()[0] == (matrix == "generated"), (ksk.form(), ksk.key_bits())
    got = out.download((2, 2, n, nl))
    for c in range(2):
        assert np.array_equal(got[c], orc.apply_key_switch(ksm, tprod[c], logQ, nl)), c
    if not crafted:
        return
    s = max(F.lin_class(m)[1], 1)
    for i, pos in enumerate(K.fold_positions(n, s)):
        d = 1 if i == 0 else (1 << 24) - 1
        t1 = np.zeros((1, 3, L, n), dtype=np.uint64)
        t1[0, 0] = orc.dcrt_from_poly(K.monomial_limbs(n, Wl, pos, d << logQ))
        ctx.apply_key_switch_dev(ksk, logQ, ctx.upload(t1), 1, out, nl)
        assert np.array_equal(out.download((2, 2, n, nl))[0], orc.apply_key_switch(ksm, t1[0], logQ, nl)), (d, pos)


def run_automorph(names, logQ, W=0, nprimes=0, p=23, nl_extra=0):
    """fhesi_ct_automorph_key_switch_dev on evaluation rows (option automorph_rows): toPoly + the positive residue modulo 2^logQ = CRT mode 3"""
    m, k = M_CHAIN, 3
    primes, roots = small_chain(m, logQ, p, W, nprimes)
    ctx, orc = F.Context(m, primes, roots), O.Oracle(m, primes, roots)
    n, L, nd, nl = ctx.phim, ctx.L, R.ndigits(logQ), (logQ + 63) // 64 + nl_extra
    rng = np.random.default_rng(logQ + L)
    ksm = np.stack([P.rand_rows(rng, primes, n, 2 * nd) for _ in range(2)])
    ksk = F.KeySwitchMatrix(ctx, 2, nd).upload(ksm)
    a, _ = two_ciphertexts(rng, n, nl, logQ)
    out = ctx.alloc(2 * 2 * n * nl * 8)
    ctx.set_option("automorph_rows", 1)
    ctx.prof_enable(True)
    ctx.ct_automorph_key_switch_dev(ksk, logQ, k, ctx.upload(a), nl, 2, out, nl)
    check_names(ctx, names)
    ctx.prof_enable(False)
    got = out.download((2, 2, n, nl))
    for c in range(2):
        assert np.array_equal(got[c], orc.apply_key_switch_parts(ksm, orc.ct_automorph(a[c], k, nl + 1), logQ, nl)), c


def run_modswitch(names, W, p=23):
    """DoubleCRT::scaleDownToSet down to one prime: the dropped primes' product decides the limb count"""
    ctx, orc, primes = chain_ring()
    kd = max(k for k in range(1, NPRIMES) if limbs_of(K.chain_product(primes[1:1 + k])) + 2 <= W)
    assert limbs_of(K.chain_product(primes[1:1 + kd])) + 2 == W
    cur = list(range(kd + 1))
    prod = K.chain_product(primes[:kd + 1])
    limbs = centred_values(np.random.default_rng(W), ctx.phim, limbs_of(prod) + 1, prod)
    d = F.DoubleCRT.from_poly(ctx, limbs, index_set=cur)
    ctx.prof_enable(True)
    d.scale_down_to_set([0], p)
    check_names(ctx, names)
    ctx.prof_enable(False)
    want = orc.dcrt_scale_down_to_set(orc.dcrt_from_poly(limbs), cur, [0], p)
    assert d.index_set() == [0] and np.array_equal(d.rows()[0], want[0])


def run_ks_big(names, m, logQ, centred, form, p=23, options=None, nl_extra=0):
    """A matrix generated on the device (KeySwitchSI::Init) with the crafted column written over column 0, on rings where one oracle call takes minutes:
    the fused form against the per-prime form of the same matrix (one dot product per chain prime, the reference's structure)."""
    primes, roots = P.chain_for(m, logQ, p, 1, 60)
    ctx = F.Context(m, primes, roots)
    n, L, nd, nl = ctx.phim, ctx.L, R.ndigits(logQ), (logQ + 63) // 64 + nl_extra
    Wl, ncol = L + 2, 3 * nd
    rng = np.random.default_rng(m + logQ)
    one = np.zeros((n, 1), dtype=np.uint64)
    one[0, 0] = 1
    t = F.DoubleCRT(ctx).sample(0, 64, 77, 1)
    t2 = t.copy()
    t2.op(t, 2)
    kg = F.KeySwitchMatrix(ctx, 3, nd).init_batch_seeded([F.DoubleCRT.from_poly(ctx, one), t, t2], t, logQ, 77, 78, 100, 3)
    edge = K.key_range_values(logQ) if centred else K.edge_values(K.chain_product(primes))
    for r in range(2):
        col = ctx.upload(F.DoubleCRT.from_poly(ctx, K.edge_limbs(edge, n, Wl, r)).rows())
        ctx.dev_copy(kg.device_ptr + r * ncol * L * n * 8, col.ptr.value, L * n * 8)
    kg.mark_dirty()
    a, b = two_ciphertexts(rng, n, nl, logQ)
    tp = ctx.alloc(2 * 3 * L * n * 8)
    ctx.ct_mul_dev(p, ctx.upload(a), ctx.upload(b), nl, 2, tp)
    s = max(F.lin_class(m)[1], 1)
    crafted = []
    for i, pos in enumerate(K.fold_positions(n, s)):
        t1 = np.zeros((1, 3, L, n), dtype=np.uint64)
        t1[0, 0] = F.DoubleCRT.from_poly(ctx, K.monomial_limbs(n, Wl, pos, (1 if i == 0 else (1 << 24) - 1) << logQ)).rows()
        crafted.append(ctx.upload(t1))
    out = ctx.alloc(2 * 2 * n * nl * 8)

    def all_outputs():
        ctx.apply_key_switch_dev(kg, logQ, tp, 2, out, nl)
        res = [out.download((2, 2, n, nl))]
        for t1 in crafted:
            ctx.apply_key_switch_dev(kg, logQ, t1, 1, out, nl)
            res.append(out.download((2, 2, n, nl))[0])
        return res

    for o, v in (options or {}).items():
        ctx.set_option(o, v)
    ctx.prof_enable(True)
    fused = all_outputs()
    check_names(ctx, names)
    ctx.prof_enable(False)
    assert kg.form()[0] == form and kg.key_bits()[0] == centred, (kg.form(), kg.key_bits())
    for o in (options or {}):
        ctx.set_option(o, 0)
    ctx.set_option("ks_direct", 1)
    direct = all_outputs()
    assert kg.form()[0] == 0
    for i, (x, y) in enumerate(zip(fused, direct)):
        assert np.array_equal(x, y), i


RUNNERS = {"to_poly": run_to_poly, "from_poly": run_from_poly, "ct_mul": run_ct_mul, "ks_small": run_ks_small, "automorph": run_automorph, "modswitch": run_modswitch, "ks_big": run_ks_big}


@pytest.mark.gpu
@pytest.mark.parametrize("names,runner,kw", ROWS)
def test_dispatch(names, runner, kw):
    RUNNERS[runner](names, **kw)


@pytest.mark.gpu
def test_name_only_classes_have_no_stopwatch():
    ctx = chain_ring()[0]
    for cls, idx in F.binding.PROF_NAMES.items():
        with pytest.raises(F.FhesiError, match="unknown kernel class"):
            F.binding._ck(F.binding._load().fhesi_prof_read(ctx.h, idx, None, None, None))
        assert ctx.prof_kernel_name(cls) is not None
    with pytest.raises(F.FhesiError, match="bad argument"):
        F.binding._ck(F.binding._load().fhesi_prof_kernel_name(ctx.h, max(F.binding.PROF_NAMES.values()) + 1, None, 0))


def test_name_only_classes_of_the_header_and_the_binding_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fhesi_hip.h")).read()
    public = {k.lower(): int(v) for k, v in re.findall(r"FHESI_PROF_NAME_(\w+) = (\d+)", header)}
    timed = {k.lower(): int(v) for k, v in re.findall(r"FHESI_PROF_(?!NAME_)(\w+) = (\d+)", header)}
    assert public == {"crt_exact": 9, "ks_recombine": 10, "rns_generic": 11, "modswitch": 12, "digits": 13}
    assert sorted(F.binding.PROF_NAMES.values()) == sorted(public.values()) and F.binding.PROF_NAMES["digits_kernel"] == public["digits"]
    assert {k: v for k, v in F.binding.PROF_NAMES.items() if k != "digits_kernel"} == {k: v for k, v in public.items() if k != "digits"}
    assert sorted(timed.values()) == sorted(F.binding.PROF_CLASSES.values()) and not set(timed.values()) & set(public.values())


# ---------------------------------------------------------------------------------------------------------------------------------- completeness
def compiled_instantiations():
    """the kernels of the families above, from the host stubs in the library's symbol table, spelled as fhesi_prof_kernel_name spells them"""
    lib = os.path.join(os.path.dirname(os.path.abspath(F.binding.__file__)), "csrc", "libfhesi_hip.so")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    found = set()
    for line in out.splitlines():
        mt = re.search(r"__device_stub__(\w+)(<.*>)?\(", line)
        if mt and mt.group(1) in FAMILIES:
            name, depth = mt.group(1), 0
            for ch in (mt.group(2) or ""):           # the template arguments up to their closing bracket (the parameter list may hold brackets too)
                name += ch
                depth += (ch == "<") - (ch == ">")
                if depth == 0:
                    break
            found.add(name)
    return found


def test_every_compiled_instantiation_is_accounted_for():
    compiled = compiled_instantiations()
    assert len(compiled) >= 55, sorted(compiled)
    named = {v for prm in ROWS for v in prm.values[0].values() if v}
    assert not named - compiled, f"rows name kernels the library does not hold: {sorted(named - compiled)}"
    assert not set(NOT_RUN) - compiled, f"NOT_RUN names kernels the library does not hold: {sorted(set(NOT_RUN) - compiled)}"
    assert not set(NOT_RUN) & named, f"both run and listed as not run: {sorted(set(NOT_RUN) & named)}"
    assert all(reason.startswith(("covered by ", "unreachable: ")) for reason in NOT_RUN.values())
    missing = compiled - named - set(NOT_RUN)
    assert not missing, f"kernels of kernels_crt.hip without a row or a NOT_RUN entry: {sorted(missing)}"
