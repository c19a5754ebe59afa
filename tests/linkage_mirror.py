"""The rule of docs/SPEC.md §15 in plain numpy over uint8[N][L] rows: which reads can be read at a codon position, which carry a
variant, and the three count tables of every pair.  It shares nothing with the device code — no planes, no bit words — so that
what the tests compare the device with is the rule's own text.  The per-read flags are formed position by position and variant by
variant; only the last step, counting the reads that have two flags at once for every pair, is a matrix product (float64: the
sums are whole numbers far below 2**53, so it is exact) — 1024 x 1024 pairs in loops would take minutes otherwise.
The statistics of a pair's 2 x 2 table are computed with fractions.Fraction and math.comb, so they are exact."""
import math
from fractions import Fraction

import numpy as np


def flags(rows, pos_cols, var_pos, var_codon):
    """(informative bool[N][P], carries bool[N][V]) of the rule."""
    rows = np.asarray(rows)
    n = len(rows)
    informative = np.zeros((n, len(pos_cols)), dtype=bool)
    codon = np.zeros((n, len(pos_cols)), dtype=np.int64)
    for p, c in enumerate(pos_cols):
        c = int(c)
        s0, s1, s2 = rows[:, c].astype(np.int64), rows[:, c + 1].astype(np.int64), rows[:, c + 2].astype(np.int64)
        informative[:, p] = (s0 < 4) & (s1 < 4) & (s2 < 4)
        codon[:, p] = 16 * s0 + 4 * s1 + s2
    carries = np.zeros((n, len(var_pos)), dtype=bool)
    for v, (p, k) in enumerate(zip(var_pos, var_codon)):
        carries[:, v] = informative[:, int(p)] & (codon[:, int(p)] == int(k))
    return informative, carries


def linkage(rows, pos_cols, var_pos, var_codon):
    """rows uint8[N][L] (codes of SPEC §1), pos_cols[P] codon starts, var_pos[V] indices into pos_cols, var_codon[V].
    Returns dict(both uint32[P][P], carry uint32[V][P], joint uint32[V][V])."""
    informative, carries = flags(rows, pos_cols, var_pos, var_codon)
    i, c = informative.astype(np.float64), carries.astype(np.float64)
    return dict(both=(i.T @ i).astype(np.uint32), carry=(c.T @ i).astype(np.uint32), joint=(c.T @ c).astype(np.uint32))


def pair_table(t, var_pos, v, w):
    """(n, n11, n10, n01, n00) of the pair (v, w), variants at different positions, from the three tables."""
    p, q = int(var_pos[v]), int(var_pos[w])
    assert p != q
    n, n11 = int(t["both"][p][q]), int(t["joint"][v][w])
    n10, n01 = int(t["carry"][v][q]) - n11, int(t["carry"][w][p]) - n11
    return n, n11, n10, n01, n - n11 - n10 - n01


def hypergeometric_tails(n11, n10, n01, n00):
    """(P(X >= n11), P(X <= n11)) as Fractions: X = the reads with both variants when the margins are fixed."""
    n, row1, col1 = n11 + n10 + n01 + n00, n11 + n10, n11 + n01
    lo, hi = max(0, row1 + col1 - n), min(row1, col1)
    total = math.comb(n, row1)
    mass = {x: math.comb(col1, x) * math.comb(n - col1, row1 - x) for x in range(lo, hi + 1)}
    assert sum(mass.values()) == total
    return Fraction(sum(m for x, m in mass.items() if x >= n11), total), Fraction(sum(m for x, m in mass.items() if x <= n11), total)


def stats(n11, n10, n01, n00, p_values=True):
    """The statistics of §15 of one 2 x 2 table, exact (Fractions; D_num an int): dict(D_num, r2, d_prime, p_positive, p_negative)."""
    n = n11 + n10 + n01 + n00
    row1, row0, col1, col0 = n11 + n10, n01 + n00, n11 + n01, n10 + n00
    d_num = n11 * n - row1 * col1
    margins = row1 * row0 * col1 * col0
    r2 = Fraction(d_num * d_num, margins) if margins else Fraction(0)
    d_max = min(row1 * col0, row0 * col1) if d_num >= 0 else min(row1 * col1, row0 * col0)
    d_prime = Fraction(d_num, d_max) if d_max else Fraction(0)
    out = dict(D_num=d_num, r2=r2, d_prime=d_prime)
    if p_values:
        out["p_positive"], out["p_negative"] = hypergeometric_tails(n11, n10, n01, n00)
    return out


# ------------------------------------------------------------------------------------------------ designed tables for the tails
TAIL_READS = (1, 2, 10, 3000, 10 ** 5, 10 ** 7, 2 * 10 ** 9, 2 ** 31 - 1)
TAIL_SIGMAS = (1, 3, 6, 12, 20, 30, 38, 45)       # 38 sigma is about 1e-300 where the tail is Gaussian, 45 is beyond the doubles
MAX_TAIL_TABLES = 1200


def _isqrt_up(v):
    r = math.isqrt(v)
    return r if r * r == v else r + 1


def tail_margins(n):
    """(row1, col1) of n reads: rare x rare, rare x common, common x rare, common x common, both nearly everything."""
    rare, common = min(30, max(1, n // 3)), max(1, n // 2)
    out = [(rare, rare), (rare, common), (common, rare), (common, max(1, n // 3)), (n - rare, n - rare)]
    return [m for k, m in enumerate(out) if 0 < m[0] < n and 0 < m[1] < n and m not in out[:k]]


def tail_design():
    """[(n11, n10, n01, n00)], each once, no random draw: for n = 1 .. 2^31 - 1 reads and the margins of `tail_margins`, n11 at
    lo, lo + 1, either side of the mean, TAIL_SIGMAS standard deviations to either side of it, hi - 1 and hi (for equal margins
    hi is perfect linkage, lo with n11 = 0 perfect exclusion, the counts next to them near-perfect), and perfect and near-perfect
    linkage and exclusion of 10 reads, 1 % and half of 10^5, 10^7 and 2 10^9; the margins of n = 1 are 0."""
    out = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    for n in TAIL_READS[1:]:
        for row1, col1 in tail_margins(n):
            lo, hi = max(0, row1 + col1 - n), min(row1, col1)
            mean = row1 * col1 // n
            s = max(1, _isqrt_up(-(-row1 * (n - row1) * col1 * (n - col1) // (n * n * max(n - 1, 1)))))
            xs = {lo, lo + 1, mean - 1, mean, mean + 1, mean + 2, hi - 1, hi}
            xs |= {mean + z * s for z in TAIL_SIGMAS} | {mean - z * s for z in TAIL_SIGMAS}
            for x in sorted({min(max(x, lo), hi) for x in xs}):
                out.append((x, row1 - x, col1 - x, n - row1 - col1 + x))
        if n >= 10 ** 5:
            for k in (10, n // 100, n // 2):
                out += [(k, 0, 0, n - k), (k, 1, 2, n - k - 3), (k - 1, 1, 0, n - k), (k, 0, 1, n - k - 1)]      # linkage
                out += [(0, k, k, n - 2 * k), (1, k, k + 2, n - 2 * k - 3), (0, k, n - k, 0), (1, k - 1, n - k - 1, 1)]    # exclusion
    seen, uniq = set(), []
    for t in out:
        if min(t) >= 0 and t not in seen:      # (half of the reads twice, and three more, do not fit)
            seen.add(t)
            uniq.append(t)
    return uniq
