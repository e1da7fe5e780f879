"""Seeded cases of the greedy partition shared by the CPU suite (kp_greedy_host against
greedy_ref) and the GPU suite (kp_greedy against both).  The expected values are computed
once per process with tests/greedy_ref.py and kept unchanged."""
import functools
import struct

import numpy as np

from kmerpapa_amd import engine
from kmerpapa_amd.pattern_utils import generality
from tests import greedy_ref as R

FIXED_PATTERNS = ["NMA", "RYS", "NNMNN", "NNNNNN"]
ONE, TWO, THREE = "ACGT", "RYSWKM", "BDHV"


def bits(x):
    return struct.pack("<d", float(x))


def _random_pattern(rng):
    k = int(rng.randint(2, 7))
    letters = []
    for _ in range(k):
        kind = rng.randint(0, 10)
        pool = "N" if kind < 4 else TWO if kind < 7 else THREE if kind < 9 else ONE
        letters.append(pool[int(rng.randint(0, len(pool)))])
    pat = "".join(letters)
    return pat if generality(pat) > 1 else pat[:-1] + "N"


def _table(rng, kind, n, cols):
    if kind == "zero":
        return np.zeros((n, cols), np.uint64), np.zeros((n, cols), np.uint64)
    if kind == "uniform":  # every position ties exactly: the first candidate must win
        return np.full((n, cols), 3, np.uint64), np.full((n, cols), 100, np.uint64)
    if kind == "big":  # totals past 2^32
        M = rng.randint(0, 1 << 28, size=(n, cols)).astype(np.uint64) * np.uint64(64)
        U = rng.randint(0, 1 << 30, size=(n, cols)).astype(np.uint64) * np.uint64(64)
        return M, U
    bg = rng.randint(1, 20000, size=(n, cols))
    M = rng.binomial(bg, rng.uniform(0.001, 0.05, size=(n, 1))).astype(np.uint64)
    U = bg.astype(np.uint64)
    if kind == "sparse":  # empty k-mers (used with alpha = 0)
        hole = rng.uniform(size=(n, 1)) < 0.3
        M = np.where(hole, 0, M).astype(np.uint64)
        U = np.where(hole, 0, U).astype(np.uint64)
    return M, U


def _beta(alpha, M, U, fold):
    trM, trU = int(M.sum()), int(U.sum())
    if fold >= 0:
        trM -= int(M[:, fold].sum())
        trU -= int(U[:, fold].sum())
    if trM == 0 or trM + trU == 0:
        return 1.0  # (get_betas would divide by zero: any beta serves the comparison)
    return R.get_betas(alpha, trM, trU)


@functools.lru_cache(maxsize=None)
def cases(n_cases=200, seed=20240611):
    """``n_cases`` cases ``(gen_pat, nf, M, U, lanes)``; lanes = (fold, chain, alpha, beta, c)."""
    rng = np.random.RandomState(seed)
    kinds = ["random", "random", "random", "zero", "uniform", "big", "sparse"]
    out = []
    for i in range(n_cases):
        gp = FIXED_PATTERNS[i % 4] if i % 3 == 0 else _random_pattern(rng)
        if gp == "NNNNNN" and i % 48 != 3:  # (4,096 k-mers: a few cases are enough for the plain-Python reference)
            gp = "NNNN"
        n = generality(gp)
        kind = kinds[i % len(kinds)]
        nf = int(rng.choice([0, 2, 3, 5]))
        M, U = _table(rng, kind, n, max(nf, 1))
        lanes = []
        for q in range(3):
            fold = -1 if nf == 0 or q == 0 else int(rng.randint(0, nf))
            alpha = 0.0 if kind == "sparse" and q < 2 else float(rng.choice([0.5, 1.0, 2.0, 10.0]))
            pens = [0.0, 1e9, 1.0, 3.0, 6.0] if n <= 1024 else [1e9, 3.0, 6.0, 12.0]
            c = float(pens[int(rng.randint(0, len(pens)))])
            lanes.append((fold, (q % 2) if fold >= 0 else -1, alpha, _beta(alpha, M, U, fold), c))
        out.append((gp, nf, M, U, tuple(lanes)))
    return tuple(out)


_expected = {}


def expected(gp, nf, M, U, lanes, key):
    """greedy_ref's result of one call: ``(loss bits, names, n_leaves, chain bits)``; cached by ``key``."""
    if key in _expected:
        return _expected[key]
    n_chains = max([ln[1] + 1 for ln in lanes] + [0])
    chain = [0.0] * n_chains
    losses, names = [], []
    for fold, ch, alpha, beta, c in lanes:
        loss, nm, terms = R.lane(gp, M, U, fold, alpha, beta, c)
        losses.append(bits(loss))
        names.append(nm)
        if ch >= 0:
            for t in terms:
                chain[ch] += t
    _expected[key] = (losses, names, [len(x) for x in names], [bits(x) for x in chain])
    return _expected[key]


def observed(gp, loss, chain, nl, leaves):
    """A greedy call's outputs in :func:`expected`'s form (``leaves[lane]`` = pattern words)."""
    k = len(gp)
    return ([bits(x) for x in loss], [[engine.word_pattern(w, k) for w in lv] for lv in leaves],
            [int(x) for x in nl], [bits(x) for x in chain])
