"""CPU: the arithmetic of crt32_mfma_kernel (fhe-si_amd/csrc/kernels_tensor32.hip) -- the fast pass of the tensor half's CRT as an int8 matrix
product -- on the operand tables the library's own host routines build (fhe-si_amd/csrc/crt32_bytes.h over the table rows of hm::crt32_mw,
fhe-si_amd/csrc/ring32_tables.h: the rows t32_config uploads, not a restatement of them; printed by the stand-alone program
tests/host/crt32_bytes_dump.cpp, built here with -fsanitize=address,undefined), against Python's integers and against the model of
crt32_scale_kernel<512, false, 28, 38, 0> in tests/test_crt32_fold_model.py.

What is modelled, step for step as the kernel does it: the depth of 40 slots x 4 bytes (primes, kappa, the constant slot with bytes 1, 0, 0, 0,
padding), residues as signed bytes y ^ 0x80808080, operand A read in the instruction's lane layout (row m of a tile lands in half (m / 4) % 2,
register 4 (m / 8) + m % 4: tools/mfma_i8_layout.hip), accumulators starting at the bias 2^22, 36 columns per half wave joined to nine words with
one add-with-carry each, the rounding limb and the undecided test in the low half, the carry (with the rounding carry, decided by an all-ones
test) handed to the high half.  kappa: the kernel sums the same floors umulhi(y_i, inv57_i) as crt32_scale_kernel, split over the two half waves,
modulo 2^32 -- the same value for every input, asserted below."""
import os
import random
import subprocess

import numpy as np
import pytest

import test_arith32_models as A
import test_crt32_fold_model as W

HERE = os.path.dirname(os.path.abspath(__file__))
LQ, R, WT, J0, NW = 512, 28, 38, 16, 21
SLOTS, COLS, HALF, BIAS = 40, 72, 36, 1 << 22
MOD = 1 << (8 * COLS)
M32 = (1 << 32) - 1


def tensor_primes(bits):
    """t32_plan_search at the metric ring: 35 primes below 2^30, or 36 below 2^29 (option tensor_bits = 29)"""
    return A.primes_below_2_30(35, 1 << 15) if bits == 30 else A.primes_below_2_29(36, 1 << 15)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crt32_bytes") / "crt32_bytes_dump")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "host", "crt32_bytes_dump.cpp")])

    def run(primes):
        r = subprocess.run([exe] + [str(p) for p in primes], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        d = np.zeros((SLOTS, 4, COLS), dtype=np.int64)
        aop = np.zeros((3, 5, 64, 4), dtype=np.int64)
        for line in r.stdout.splitlines():
            f = line.split()
            if f[0] == "d":
                d[int(f[1]), int(f[2])] = [int(v) for v in f[3:]]
            else:
                aop[int(f[1]), int(f[2]), int(f[3])] = [int(v, 16) for v in f[4:]]
        return d, aop
    return run


class Shape:
    def __init__(self, bits, dump):
        self.primes = tensor_primes(bits)
        self.NP = len(self.primes)
        self.tb = W.tables(self.primes, R, WT)
        M, self.cinv, self.inv57, Mw, Nw = self.tb
        window = lambda row: sum(row[J0 + l] << (R * l) for l in range(NW))
        self.C = [window(row) for row in Mw] + [window(Nw)]              # C_i, then C_kappa: what crt32_scale_kernel multiplies
        self.d, self.aop = dump(self.primes)
        # operand A as a matrix [tile][row m][depth byte (slot, a)], read back from the lane layout
        self.Amat = np.zeros((3, 32, SLOTS * 4), dtype=np.int64)
        for tile in range(3):
            for ks in range(5):
                for lane in range(64):
                    for tt in range(4):
                        s, w = ks * 8 + (lane >> 5) * 4 + tt, int(self.aop[tile, ks, lane, tt])
                        for a in range(4):
                            v = (w >> (8 * a)) & 255
                            self.Amat[tile, lane & 31, 4 * s + a] = v - 256 if v >= 128 else v


@pytest.fixture(scope="module", params=[30, 29])
def shape(request, dump):
    return Shape(request.param, dump)


def test_prime_sets():
    assert tensor_primes(30) == list(W.METRIC_PRIMES) and len(tensor_primes(29)) == 36 and max(tensor_primes(29)) < 1 << 29


def test_balanced_bytes_recombine(shape):
    d, NP = shape.d, shape.NP
    assert d.min() >= -128 and d.max() <= 127
    val = lambda s, a: sum(int(d[s, a, c]) << (8 * c) for c in range(COLS)) % MOD
    for s in range(NP + 1):
        for a in range(4):
            assert val(s, a) == (shape.C[s] << (8 * a)) % MOD, (s, a)
    K = (0x80808080 * sum(shape.C) - BIAS * sum(1 << (8 * c) for c in range(COLS))) % MOD
    assert val(NP + 1, 0) == K
    assert not d[NP + 1, 1:].any() and not d[NP + 2:].any()


def test_operand_layout_holds_every_column_once(shape):
    """row m of tile t is column ((m / 4) % 2) * 36 + 16 t + 4 (m / 8) + m % 4 while that register index is below 36, a zero row otherwise"""
    seen = set()
    for tile in range(3):
        for m in range(32):
            q = tile * 16 + 4 * (m >> 3) + (m & 3)
            row = shape.Amat[tile, m]
            if q >= HALF:
                assert not row.any()
                continue
            col = ((m >> 2) & 1) * HALF + q
            seen.add(col)
            assert np.array_equal(row.reshape(SLOTS, 4), shape.d[:, :, col]), (tile, m)
    assert seen == set(range(COLS))


def kernel_model(shape, y):
    """-> (round(x / 2^512) mod 2^512, undecided, kappa, F mod 2^576, largest |partial sum|) as crt32_mfma_kernel computes them"""
    NP, inv57 = shape.NP, shape.inv57
    fs = [0, 0]
    for s in range(NP):                                   # each half wave sums the floors of its slots, then one exchange
        fs[(s >> 2) & 1] = (fs[(s >> 2) & 1] + ((y[s] * inv57[s]) >> 32)) & M32
    kappa = (((fs[0] + fs[1]) & M32) + (1 << 24) & M32) >> 25
    B = np.zeros(SLOTS * 4, dtype=np.int64)
    for s in range(SLOTS):
        if s == NP + 1:
            word = 1
        else:
            word = ((y[s] if s < NP else kappa if s == NP else 0) ^ 0x80808080) & M32
        for a in range(4):
            v = (word >> (8 * a)) & 255
            B[4 * s + a] = v - 256 if v >= 128 else v
    # the accumulators: bias, then five depth steps of 32 bytes (the order the instruction adds them in is its own; every prefix over whole
    # steps and every prefix in depth order is bounded here)
    prod = shape.Amat * B                                 # [tile][m][depth]
    partial = BIAS + np.cumsum(prod, axis=2)
    worst = int(np.abs(partial).max())
    acc = partial[:, :, -1]
    S = [[0] * HALF, [0] * HALF]
    for tile in range(3):
        for m in range(32):
            q = tile * 16 + 4 * (m >> 3) + (m & 3)
            if q < HALF:
                S[(m >> 2) & 1][q] = int(acc[tile, m])
    F = sum((S[h][q] << (8 * (HALF * h + q))) for h in range(2) for q in range(HALF)) % MOD
    Wd, Hp, cy = [[0] * 9, [0] * 9], [0, 0], [0, 0]
    for h in range(2):
        for w in range(9):
            s0, s1, s2, s3 = S[h][4 * w:4 * w + 4]
            assert 0 < min(s0, s1, s2, s3) and max(s0, s1, s2, s3) < 1 << 23
            lo, hi2 = s0 + (s1 << 8), s2 + (s3 << 8)
            assert lo <= M32 and hi2 <= M32
            v = lo + (hi2 << 16)
            t = (v & M32) + Hp[h] + cy[h]
            Wd[h][w], cy[h], Hp[h] = t & M32, t >> 32, v >> 32
    G = (Wd[0][1] << 32) | Wd[0][0]
    undecided = (G >> (64 - W.WIN)) == (1 << (W.WIN - 1)) - 1
    rnd = Wd[0][1] >> 31
    ones = all(Wd[0][w] == M32 for w in range(2, 9))
    cout = Hp[0] + cy[0] + (1 if rnd and ones else 0)
    for h in range(2):
        c = 0
        for w in range(9):
            t = Wd[h][w] + ((cout if h else 0) if w == 0 else (rnd if w == 2 and not h else 0)) + c
            Wd[h][w], c = t & M32, t >> 32
    words = Wd[0][2:] + Wd[1]
    return sum(v << (32 * i) for i, v in enumerate(words)), undecided, kappa, F, worst


def residue_sets(shape, rng):
    primes = shape.primes
    yield "zeros", [0] * len(primes)
    yield "p-1", [p - 1 for p in primes]
    for pos in range(4):                                  # one byte value in one position of every residue, the other bytes random (below p: the top byte is cut)
        for v in (0x00, 0x7f, 0x80, 0xff):
            y = []
            for p in primes:
                t = (rng.getrandbits(32) & ~(255 << (8 * pos))) | (v << (8 * pos))
                y.append(t % p if t >= p else t)
            yield "byte%d=%02x" % (pos, v), y
    for v in (0x00, 0x7f, 0x80, 0xff):                    # the same value in all of the three low bytes, top byte at the largest the prime allows
        yield "all=%02x" % v, [min(p - 1, ((p >> 24) << 24) | (v * 0x010101)) for p in primes]
    M, cinv = shape.tb[0], shape.cinv
    bound = 1 << 1042
    for k in range(40):                                   # residues of integers of the tensor product's size (kappa as the pipeline sees it)
        x = rng.randrange(-bound, bound) if k else -bound
        yield "x%d" % k, [(x % p) * c % p for p, c in zip(primes, cinv)]
    for x in W.boundary_values(rng, LQ, bound)[:40]:
        yield "edge", [(x % p) * c % p for p, c in zip(primes, cinv)]
    for k in range(20):
        yield "rand%d" % k, [rng.randrange(p) for p in primes]


def test_byte_planes_match_the_integers_and_the_valu_kernel(shape):
    rng = random.Random(20 + shape.NP)
    worst, flagged = 0, 0
    for name, y in residue_sets(shape, rng):
        out, und, kappa, F, w = kernel_model(shape, y)
        o_ref, und_ref, kappa_ref = W.crt32_scale(y, shape.primes, shape.tb, LQ, R, False, 62)
        assert kappa == kappa_ref, name                   # the sum of floors, whatever the order
        assert F == (sum(yi * c for yi, c in zip(y, shape.C)) + kappa * shape.C[shape.NP]) % MOD, name
        assert (out, und) == (o_ref, und_ref), name
        worst, flagged = max(worst, w), flagged + und
    assert worst < 1 << 31 and worst < BIAS + (shape.NP + 1) * 4 * 128 * 128 + 128 + 1
    assert flagged > 0, "the edge values must reach the undecided branch"


def test_exact_sum_would_give_the_same_kappa(shape):
    """x / M is within 0.36 of an integer (1/8 with primes of 30 bits); the sum of floors and the floor of the exact sum differ by less than NP
    units of 2^-25, so either rounds to the same kappa -- the kernel keeps the sum of floors"""
    rng = random.Random(7)
    M, cinv = shape.tb[0], shape.cinv
    for _ in range(200):
        x = rng.randrange(-(1 << 1042), 1 << 1042)
        y = [(x % p) * c % p for p, c in zip(shape.primes, cinv)]
        floors = sum((yi * iv) >> 32 for yi, iv in zip(y, shape.inv57))
        exact = sum(yi * iv for yi, iv in zip(y, shape.inv57)) >> 32
        assert 0 <= exact - floors < shape.NP
        assert (floors + (1 << 24)) >> 25 == (exact + (1 << 24)) >> 25 == (sum(yi * (M // p) for yi, p in zip(y, shape.primes)) - x) // M
