"""CPU: the ring identity behind the hoisted rotations on the model (tests/hoist_model.py over oracle/fhesi_pyref.py), and the symbols the feature
adds to the header and the binding.  Exact."""
import os
import re

import pytest

import fhesi_pyref as R
import hoist_model as H
import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fhesi_ksk_hoist", "fhesi_ct_rotations_dev", "fhesi_ct_matvec_dev")


@pytest.mark.parametrize("m,p,ks", [(256, 257, (3, 9, 255)),        # power of two: sigma is a signed permutation of the coefficients
                                    (250, 251, (3, 7, 249)),        # 2 x 5^3: sigma reduces modulo Phi_m
                                    (101, 607, (2, 51, 100))])      # a prime m
def test_hoisted_form_equals_the_independent_form_and_decrypts_like_the_reference(m, p, ks):
    logQ = 128
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, primes, roots)
    rng = R.SplitMix64(1000 + m)
    t, pk = R.keygen(ctx, rng)
    n = ctx.phim
    msg = [(7 * i * i + 3 * i + 1) % p for i in range(n)]
    ct = R.encrypt(ctx, pk, msg, rng)
    assert R.decrypt(ctx, t, ct) == msg
    for k in ks:
        ksm = R.key_switch_init_automorph(ctx, t, k, rng)
        hoisted = H.hoist_matrix(ctx, ksm, k)
        got = H.rotation(ctx, hoisted, k, ct)
        assert got == H.rotation_independent(ctx, ksm, k, ct), k       # the identity, bit for bit
        ref = H.rotation_reference(ctx, ksm, k, ct)
        want = H.automorph_message(ctx, msg, k)
        assert R.decrypt(ctx, t, got) == want == R.decrypt(ctx, t, ref), k
        assert got != ref, k                                            # ... and not the reference's words: it decomposes sigma_k(c)
        assert H.rotations(ctx, [hoisted, None], [k, 1], [ct]) == [[got], [ct]]      # the shared-digit form is the same function
        # sigma_k o sigma_k^-1 = id on the matrix
        assert H.hoist_matrix(ctx, hoisted, pow(k, -1, m)) == ksm
    # the identity entry is the reduced copy
    wide = [[c + (1 << logQ) * ((i % 3) - 1) for i, c in enumerate(part)] for part in ct]
    assert H.rotation(ctx, None, 1, wide) == ct


def test_matvec_on_the_model_decrypts_to_the_sum_of_rotated_products():
    m, p, logQ = 256, 257, 128
    primes, roots = P.chain_for(m, logQ, p)
    ctx = R.Ctx(m, logQ, p, primes, roots)
    rng = R.SplitMix64(77)
    t, pk = R.keygen(ctx, rng)
    n = ctx.phim
    msg = [(5 * i + 2) % p for i in range(n)]
    ct = R.encrypt(ctx, pk, msg, rng)
    ks = (1, 3, 255)
    hoisted = [None] + [H.hoist_matrix(ctx, R.key_switch_init_automorph(ctx, t, k, rng), k) for k in ks[1:]]
    diags = [[(3 * j + i) % p for i in range(n)] for j in range(len(ks))]
    got = R.decrypt(ctx, t, H.matvec(ctx, hoisted, ks, diags, ct))
    want = [0] * n
    for k, w in zip(ks, diags):
        term = R.poly_mul_mod_phi(ctx, H.automorph_message(ctx, msg, k), w)
        want = [(a + b) % p for a, b in zip(want, term)]
    assert got == want


def test_header_and_binding_name_the_new_entries():
    import fhe_si_amd as F
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhesi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fhesi_[a-z0-9_]+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in F.binding.ABI_SYMBOLS, s
    assert re.search(r"#define\s+FHESI_ABI_VERSION\s+9\b", src) and F.binding.ABI_VERSION == 9      # entries are only added
    for name in ("hoist",):
        assert hasattr(F.KeySwitchMatrix, name)
    for name in ("ct_rotations_dev", "ct_matvec_dev"):
        assert hasattr(F.Context, name)
    for name in ("rotations", "matvec"):
        assert hasattr(F.SlotSpace, name) and hasattr(F.SlotBasis, name)


def test_the_mirror_header_compiles_on_top_of_the_class_surface(tmp_path):
    """fhe-si_amd/host/fhesi_hoist.h is not part of fhesi_host.h (nothing the recording evaluator instantiates may call the new entries): a caller's
    translation unit that includes it and uses KeySwitchSI::Hoisted and HoistedRotations has to compile.  Syntax only: no library, no device."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host harness of this project"
    src = tmp_path / "use_hoist.cpp"
    src.write_text('#include "fhesi_hoist.h"\n'
                   "using namespace fhesi;\n"
                   "std::vector<Ciphertext> rotate(const KeySwitchSI& w3, const KeySwitchSI& w9, const Ciphertext& c) {\n"
                   "  HoistedKey h3 = w3.Hoisted(3), h9 = w9.Hoisted(9);\n"
                   "  return HoistedRotations(c, {nullptr, &h3, &h9});\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wno-unused-function", "-fsyntax-only", "-I", os.path.join(ROOT, "fhe-si_amd", "host"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
