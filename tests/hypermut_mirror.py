"""The per-read hypermutation counters, their exact test and the keep rule of docs/SPEC.md §26 restated without a device: the
counters as a few numpy comparisons over the three shifted views of a [n_reads][n_cols] code array — nothing of the kernel's shape
in it —, the p-value as an exact rational sum of hypergeometric masses, and the rule p < alpha.  The expectations of
tests/test_hypermut_host.py, tests/test_gpu_hypermut.py and tests/test_gpu_hypermut_cli.py."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

TARGET_SITES, TARGET_MUT, CONTROL_SITES, CONTROL_MUT = range(4)
A, C, G, T = range(4)


def counts(rows, ref):
    """rows[n_reads, n_cols] codes 0..6; ref[n_cols] codes (only G makes a site).  uint32 [4, n_reads]."""
    rows = np.asarray(rows, dtype=np.uint8)
    ref = np.asarray(ref, dtype=np.uint8)
    assert rows.ndim == 2 and ref.shape == (rows.shape[1],)
    if rows.shape[1] < 3:
        return np.zeros((4, rows.shape[0]), dtype=np.uint32)
    x, y, z = rows[:, :-2], rows[:, 1:-1], rows[:, 2:]
    site = (ref[:-2] == G)[None, :] & ((x == A) | (x == G)) & (y < 4) & (z < 4)
    target = site & ((y == A) | (y == G)) & (z != C)
    control = site & ~target
    mut = x == A
    return np.stack([m.sum(axis=1) for m in (target, target & mut, control, control & mut)]).astype(np.uint32)


@lru_cache(maxsize=None)
def exact_p(a, n, c, m):
    """P(X >= a) for X ~ Hypergeometric(n + m, a + c, n) as a Fraction; 1 when n == 0 or m == 0."""
    assert 0 <= a <= n and 0 <= c <= m
    if n == 0 or m == 0:
        return Fraction(1)
    k = a + c
    hi = min(k, n)
    num = sum(math.comb(n, x) * math.comb(m, k - x) for x in range(a, hi + 1))
    return Fraction(num, math.comb(n + m, k))


def log_of(fr):
    """ln of a positive Fraction, in double, without leaving its range."""
    if fr == 1:
        return 0.0
    n, d = fr.numerator, fr.denominator
    if 2 * n > d:                                    # near 1: ln p = log1p(-(1 - p)), the complement in full precision
        return math.log1p(-float(1 - fr))
    sn, sd = max(0, n.bit_length() - 1000), max(0, d.bit_length() - 1000)
    return math.log((n >> sn) / (d >> sd)) + (sn - sd) * math.log(2.0)


def p_values(cnt):
    """(p, log_p) as float64 arrays of counts[4, n], each the exact rational rounded once."""
    cnt = np.asarray(cnt)
    frs = [exact_p(int(cnt[TARGET_MUT, i]), int(cnt[TARGET_SITES, i]), int(cnt[CONTROL_MUT, i]), int(cnt[CONTROL_SITES, i])) for i in range(cnt.shape[1])]
    return np.array([float(f) for f in frs], dtype=np.float64), np.array([log_of(f) for f in frs], dtype=np.float64), frs


def keep(p, alpha=0.05):
    """(idx, n_flagged): the reads that are not hypermutated (p >= alpha: the rule is a strict p < alpha), ascending."""
    p = np.asarray(p)
    flagged = np.array([x < alpha for x in p], dtype=bool)
    return np.flatnonzero(~flagged).astype(np.uint32), int(flagged.sum())
