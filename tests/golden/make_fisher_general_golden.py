#!/usr/bin/env python3
"""Generates tests/golden/fisher_general_golden.json — run in the dev container only (needs mpmath + scipy).

The pin of the general-margin Fisher test of docs/SPEC.md §21 (minorseq_amd/csrc/jl_fisher_general.h), as make_fisher_golden.py
is the pin of the equal-row one: an independent 60-digit evaluation of the hypergeometric upper tail P(X >= a) of the table
[[a, cov_s - a], [c, cov_c - c]], cross-checked against scipy.stats.fisher_exact where scipy does not underflow (loosely: scipy
is good to ~1e-9 relative at 1e7 coverage; mpmath is the pin).  The tail is summed at 90 digits from one exact point mass by
the ratio of neighbouring masses, on the side of the mean where the terms fall (the other side is the complement, which is
never small there), until a term is below 1e-80 of the sum.  Nothing here travels to a GPU machine; only the JSON does.
"""
import json
import math
import random

import mpmath as mp
from scipy.stats import fisher_exact

mp.mp.dps = 90
CAP = 1500


def pmf(x, M, K, n):
    return mp.binomial(K, x) * mp.binomial(M - K, n - x) / mp.binomial(M, n)


def upper_tail(a, b, c, d):
    M, K, n = a + b + c + d, a + c, a + b
    lo, hi = max(0, K - (M - n)), min(K, n)
    if a <= lo:
        return mp.mpf(1)
    L = M - K
    if a * M >= n * K:   # at or above the mean: the terms fall upwards
        term = pmf(a, M, K, n)
        s = term
        for x in range(a, hi):
            term = term * (K - x) * (n - x) / ((x + 1) * (L - n + x + 1))
            s += term
            if term < s * mp.mpf("1e-80"):
                break
        return s
    term = pmf(a - 1, M, K, n)
    s = term
    for x in range(a - 1, lo, -1):
        term = term * x * (L - n + x) / ((K - x + 1) * (n - x + 1))
        s += term
        if term < s * mp.mpf("1e-80"):
            break
    return 1 - s


def main():
    rnd = random.Random(20210921)
    tables = []
    # tiny random tables, all regimes (rows of different size)
    for _ in range(150):
        tables.append(tuple(rnd.randint(0, 30) for _ in range(4)))
    # sample against control: coverages x row ratios x observed counts x the control's count
    for cov_s in (50, 2907, 6000, 100000, 10000000):
        for num, den in ((1, 100), (1, 10), (1, 1), (10, 1)):
            cov_c = max(1, cov_s * num // den)
            obs = sorted({1, 2, 3, 5, 8, 13, 21, 40, 75, max(1, cov_s // 1000), max(1, cov_s // 100), max(1, cov_s // 10),
                          max(1, cov_s // 2), cov_s - 1, cov_s})
            for a in obs:
                if not 1 <= a <= cov_s:
                    continue
                near = (a * cov_c + cov_s // 2) // cov_s
                above = near + max(2, math.isqrt(9 * (near + 1)))
                for c in sorted({0, 1, near, above}):
                    if c <= cov_c:
                        tables.append((a, cov_s - a, c, cov_c - c))
    out = []
    seen = set()
    for t in tables:
        if t in seen or t[0] + t[1] == 0 or t[2] + t[3] == 0 or t[0] + t[2] == 0:
            continue
        seen.add(t)
        a, b, c, d = t
        p = upper_tail(a, b, c, d)
        rec = {"a": a, "b": b, "c": c, "d": d, "p": mp.nstr(p, 25), "log_p": mp.nstr(mp.log(p), 25)}
        if p > mp.mpf("1e-290"):
            sp = fisher_exact([[a, b], [c, d]], alternative="greater")[1]
            assert abs(sp - float(p)) <= 1e-7 * float(p) + 1e-300, (t, sp, float(p))
            rec["scipy"] = repr(float(sp))
        out.append(rec)
    assert len(out) <= CAP, len(out)
    with open(__file__.replace("make_fisher_general_golden.py", "fisher_general_golden.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_fisher_general_golden.py", "dps": 60, "tail": "greater",
                   "tables": out}, f, indent=0)
    print(len(out), "tables")


if __name__ == "__main__":
    main()
