#!/usr/bin/env python3
"""Generates tests/golden/fisher_general_domain.json — run in the dev container only (needs mpmath).

The exact values of the designed tables of tests/fisher_general_domain.py: P(X >= a) of the table [[a, n - a], [c, m - c]],
X ~ Hypergeometric(n + m, a + c, n), and its logarithm, to 25 significant digits.

  * K = a + c <= K_EXACT: rationals.  The point masses are products of K integer factors (no binomial coefficient of the rows,
    which may hold 4e9 reads), the tail is the sum of every mass it holds.
  * above that: one point mass from mpmath's binomial at DPS digits, and the tail from it by the ratio of neighbouring masses
    on the side of the mean where the terms fall, until a term is below 1e-80 of the sum.  The recurrence runs on integers
    scaled by 2^FIX_BITS, each step rounded down: with at most a few 1e5 steps, each wrong by at most 2^-FIX_BITS of the FIRST
    (largest) term, the sum is good to far more than 100 digits, at a hundredth of the time of mpf arithmetic.
Every table with K <= K_EXACT is evaluated both ways and the two must agree to 1e-60 (relative, on p and on 1 - p).
A re-run reproduces the file byte for byte.  Nothing here travels to a GPU machine; only the JSON does.
"""
import json
import math
import os
import sys
from fractions import Fraction

import mpmath as mp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

DPS = 120
mp.mp.dps = DPS
K_EXACT = 400
FIX_BITS = 512
DIGITS = 25


def exact_pmf(x, K, n, m):
    """P(X = x) as a Fraction: C(K, x) prod_{i<x} (n - i) prod_{i<K-x} (m - i) / prod_{i<K} (n + m - i)."""
    M = n + m
    num = math.comb(K, x) * math.prod(n - i for i in range(x)) * math.prod(m - i for i in range(K - x))
    return Fraction(num, math.prod(M - i for i in range(K)))


def exact_upper_tail(a, n, c, m):
    K = a + c
    lo, hi = max(0, K - m), min(K, n)
    if a <= lo:
        return Fraction(1)
    if 2 * a > lo + hi:   # the shorter sum
        return sum(exact_pmf(x, K, n, m) for x in range(a, hi + 1))
    return 1 - sum(exact_pmf(x, K, n, m) for x in range(lo, a))


def mp_pmf(x, K, n, m):
    return mp.binomial(K, x) * mp.binomial(n + m - K, n - x) / mp.binomial(n + m, n)


def _sum_ratio(x0, stop, step, K, n, L):
    """sum_{x from x0 to stop} P(X = x) / P(X = x0) as an mpf, the terms falling from x0 on."""
    one = 1 << FIX_BITS
    term = total = one
    floor = one >> 270          # 2^-270 < 1e-80: once a term is below it (relative to a sum >= 1) the rest does not count
    x = x0
    while x != stop:
        if step > 0:
            term = term * ((K - x) * (n - x)) // ((x + 1) * (L - n + x + 1))
        else:
            term = term * (x * (L - n + x)) // ((K - x + 1) * (n - x + 1))
        total += term
        x += step
        if term < floor:
            break
    return mp.mpf(total) / mp.mpf(one)


def mp_upper_tail(a, n, c, m):
    """(p, 1 - p) as mpfs; the one that was summed is exact to the working precision, the other its complement."""
    K, M = a + c, n + m
    lo, hi = max(0, K - m), min(K, n)
    if a <= lo:
        return mp.mpf(1), mp.mpf(0)
    L = M - K
    if a * M >= n * K:
        p = mp_pmf(a, K, n, m) * _sum_ratio(a, hi, 1, K, n, L)
        return p, 1 - p
    q = mp_pmf(a - 1, K, n, m) * _sum_ratio(a - 1, lo, -1, K, n, L)
    return 1 - q, q


def to_mpf(fr):
    return mp.mpf(fr.numerator) / mp.mpf(fr.denominator)


def evaluate(a, n, c, m):
    """(p, ln p) as strings of DIGITS significant digits, and how they were made."""
    K = a + c
    p_mp, q_mp = mp_upper_tail(a, n, c, m)
    if K <= K_EXACT:
        fr = exact_upper_tail(a, n, c, m)
        p, q = to_mpf(fr), to_mpf(1 - fr)
        got, want = (p_mp, p) if a * (n + m) >= n * K or p == 1 else (q_mp, q)     # the tail the second evaluation summed
        assert abs(got - want) <= mp.mpf("1e-60") * want, (a, n, c, m, got, want)
        how = "rational"
    else:
        p, q = p_mp, q_mp
        how = "mpmath"
    assert 0 < p <= 1
    logp = mp.log(p) if p < mp.mpf("0.5") else mp.log1p(-q)
    return mp.nstr(p, DIGITS), mp.nstr(logp, DIGITS), how


def main():
    import fisher_general_domain as gd
    tabs = gd.tables()
    assert len(tabs) <= gd.MAX_TABLES, len(tabs)
    out, made = [], {"rational": 0, "mpmath": 0}
    for fam, a, n, c, m in tabs:
        p, lp, how = evaluate(a, n, c, m)
        made[how] += 1
        out.append({"fam": fam, "a": a, "n": n, "c": c, "m": m, "p": p, "log_p": lp})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fisher_general_domain.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_fisher_general_domain_golden.py", "dps": DPS, "k_exact": K_EXACT,
                   "tail": "greater", "tables": out}, f, indent=0)
        f.write("\n")
    print(len(out), "tables:", made)


if __name__ == "__main__":
    main()
