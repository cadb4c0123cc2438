"""Crafted inputs of the key-switch tests, shared by test_gpu_pipeline.py, test_gpu_primepower.py and test_gpu_crt_dispatch.py.

Scaled-down parts = (d X^pos, 0, 0) against a key row (r, 0) that holds an `edge` polynomial: the dot product is d X^pos e mod Phi_m, so the
integer the recombination reduces sits on the edges of its ranges in every coefficient -- +-(P-1)/2, (P-1)/2 +- 1 (wraps), 0, +-1, P-1, ... for a
matrix of general limbs; the extremes of [-2^(logQ-1), 2^(logQ-1)] for a matrix of centred limbs (larger values would change the form that runs)."""
import numpy as np

import oracle_lib as O


def chain_product(primes) -> int:
    prod = 1
    for q in primes:
        prod *= int(q)
    return prod


def edge_values(Pprod: int):
    """the edges of the reduction modulo the chain product P"""
    h, pb = (Pprod - 1) // 2, Pprod.bit_length()
    return [h, -h, h + 1, h - 1, 0, 1, -1, Pprod - 1, h + 2, 12345, -(1 << (pb * 4 // 7)), (1 << (pb - 8)) + 17]


def key_range_values(logQ: int):
    """the edges of the coefficient range of a generated matrix (KeySwitchSI::Init, FHE-SI.cpp:176-204): [-2^(logQ-1), 2^(logQ-1)]"""
    half = 1 << (logQ - 1)
    return [-half, half - 1, half, -half + 1, 0, 1, -1, half - 2, -(half >> 1), (half >> 1) + 1, 12345, -(1 << (logQ * 4 // 7))]


def edge_limbs(values, n: int, W: int, r: int = 0) -> np.ndarray:
    """the n coefficients `values` rotated by r and repeated, as [n][W] two's complement limbs (only len(values) big integers are converted)"""
    rot = values[r:] + values[:r]
    return O.ints_to_limbs(rot, W)[np.arange(n) % len(rot)]


def monomial_limbs(n: int, W: int, pos: int, value: int) -> np.ndarray:
    """value X^pos as [n][W] limbs"""
    out = np.zeros((n, W), dtype=np.uint64)
    out[pos] = O.ints_to_limbs([value], W)[0]
    return out


def fold_positions(n: int, s: int):
    """positions of the unit digit at which every residue class j mod s and both parities of floor(j / s) reach the fold (s: the ring's stride)"""
    return sorted({0, s - 1, s % n, n - s, n - 1, n // 2})
