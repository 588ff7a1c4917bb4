"""Inputs of the brute-force matcher tests, generated from seeds (nothing is committed).  A case is a dict
{name, norm, q, t} (+ `planted`: the (query, train) pairs a planted case must find)."""
import zlib

import numpy as np

import bf_ref

SIZES = ((1, 1), (1, 300), (63, 65), (64, 64), (257, 191))     # below / at / above the kernel's 64-row tile, several tiles
HAMMING_D = (1, 32, 61)                                         # 1: ties everywhere; 61: no multiple of the 4-byte word
L2_D = (1, 3, 127, 128, 129, 512)                               # around the 32-float chunk and the largest


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def hamming_cases():
    out = []
    for M, N in SIZES:
        for D in HAMMING_D:
            name = f"ham_{M}x{N}_d{D}"
            r = _rng(name)
            out.append(dict(name=name, norm=bf_ref.NORM_HAMMING, q=r.integers(0, 256, (M, D), dtype=np.uint8),
                            t=r.integers(0, 256, (N, D), dtype=np.uint8)))
    return out


def planted_hamming(M=300, N=280, D=32, n_planted=200, seed=7):
    """n_planted train rows are query rows with 1..3 flipped bits, in shuffled order; the rest is random"""
    r = np.random.default_rng(seed)
    q = r.integers(0, 256, (M, D), dtype=np.uint8)
    t = r.integers(0, 256, (N, D), dtype=np.uint8)
    qi, tj = r.permutation(M)[:n_planted], r.permutation(N)[:n_planted]
    for a, b in zip(qi, tj):
        row = q[a].copy()
        for bit in r.permutation(8 * D)[:r.integers(1, 4)]:
            row[bit >> 3] ^= np.uint8(1 << (bit & 7))
        t[b] = row
    order = np.argsort(qi)
    planted = np.stack([qi[order], tj[order]], 1).astype(np.int32)
    return dict(name=f"ham_planted_{M}x{N}_d{D}", norm=bf_ref.NORM_HAMMING, q=q, t=t, planted=planted)


def l2_exact_cases():
    """integer-valued float32 in -8..8: every sum is below 2^24, so float32 is exact in any order; ties and ties that only the
    root makes are real"""
    out = []
    for M, N in SIZES:
        for D in L2_D:
            name = f"l2int_{M}x{N}_d{D}"
            r = _rng(name)
            out.append(dict(name=name, norm=bf_ref.NORM_L2, q=r.integers(-8, 9, (M, D)).astype(np.float32),
                            t=r.integers(-8, 9, (N, D)).astype(np.float32)))
    return out


def l2_unit_case(seed=0, M=257, N=191, D=128):
    """unit rows, normalised in float64 and cast to float32 (seed 0: the smallest gap between the best and the second-best
    SQUARED distance is 2.4e-4 over the rows and 2.7e-4 over the columns, 114 mutual pairs; seed 1 fails the gap test)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, D))
    b = rng.standard_normal((N, D))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return dict(name=f"l2unit_s{seed}_{M}x{N}_d{D}", norm=bf_ref.NORM_L2, q=a.astype(np.float32), t=b.astype(np.float32))


NONFINITE_QUERY, NONFINITE_TRAIN = 7, 11


def l2_nonfinite_case():
    """one query row of NaN and one train row of +inf: neither may appear in a match"""
    r = np.random.default_rng(3)
    q = r.integers(-8, 9, (40, 16)).astype(np.float32)
    t = r.integers(-8, 9, (50, 16)).astype(np.float32)
    q[NONFINITE_QUERY] = np.nan
    t[NONFINITE_TRAIN] = np.inf
    return dict(name="l2_nonfinite_40x50_d16", norm=bf_ref.NORM_L2, q=q, t=t)


def exact_cases():
    """every case whose result is exact: the GPU must return the restatement's bits"""
    return hamming_cases() + [planted_hamming()] + l2_exact_cases() + [l2_nonfinite_case()]


_memo = {}


def expected(case, cross_check, l2="f32"):
    """the restatement's (ij, dist) of a case, computed once"""
    key = (case["name"], bool(cross_check), l2)
    if key not in _memo:
        ij, dist = bf_ref.match(case["q"], case["t"], case["norm"], cross_check, l2)
        ij.setflags(write=False)
        dist.setflags(write=False)
        _memo[key] = (ij, dist)
    return _memo[key]
