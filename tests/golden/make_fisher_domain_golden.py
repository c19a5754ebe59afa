#!/usr/bin/env python3
"""Generates tests/golden/fisher_domain.json: the designed tables of tests/fisher_domain.py (the whole count domain of
csrc/jl_fisher.h: a + c > n, expected fractions up to 100 %, every switch point of the saddle-point form, the direct products,
the underflow region, the two-sided form) with p and ln p in exact arithmetic.  Needs mpmath (for printing the 60-digit values
only); the tests read the JSON.

The method is make_call_edges_golden.py's: with both rows summing to n, P(X = x) = w(x) / D with the integers
    w(x) = C(K, x) * n!/(n-x)! * n!/(n-K+x)!,   D = (2n)!/(2n-K)!,   K = a + c,
w walked by its integer ratio recurrence from ONE product; the Vandermonde identity sum w = D is asserted for every table.
Upper tail (tail 0): the sum over x >= a.  Two-sided (tail 1): the sum of all w(x) <= w(a), the definition (SPEC §5), not the
symmetry the routine uses.  p and ln p are printed from the rationals at 60 digits, 17 significant digits kept.

K is bounded by 20000 (fisher_domain.K_MAX).  The one table above it, a = n = 10^7 against c = 1, has a single term,
p = (n + 1) n n! (n - 1)! / (2n)!, printed from mpmath's loggamma at 90 digits (the closed form is checked against the integers
at small n).

Run time: under a minute on 8 cores."""
import json
import math
import multiprocessing
import os
import sys
import time

import mpmath as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fisher_domain as fd  # noqa: E402

DIGITS = 17


def weights(a, c, n):
    """(lo, [w(lo) .. w(hi)], D) for the table [[a, n-a], [c, n-c]]."""
    K = a + c
    lo, hi = max(0, K - n), min(K, n)
    w = math.comb(K, lo) * math.perm(n, lo) * math.perm(n, K - lo)
    ws = [w]
    for x in range(lo, hi):
        w = w * (K - x) * (n - x)
        q = (x + 1) * (n - K + x + 1)
        assert w % q == 0
        w //= q
        ws.append(w)
    D = math.perm(2 * n, K)
    assert sum(ws) == D   # Vandermonde
    return lo, ws, D


def p_exact(a, c, n, tail):
    """(S, D): p = S / D."""
    lo, ws, D = weights(a, c, n)
    if tail == 0:
        return sum(ws[max(a, lo) - lo:]), D
    wa = ws[a - lo]
    return sum(w for w in ws if w <= wa), D


def single_term_log_p(n):
    """ln p of a = n against c = 1: K = n + 1, the support is [1, n] and the tail is its last term."""
    n = mp.mpf(n)
    return mp.log(n + 1) + mp.log(n) + mp.loggamma(n + 1) + mp.loggamma(n) - mp.loggamma(2 * n + 1)


def evaluate(row):
    fam, a, c, n, tail = row
    if a + c > fd.K_MAX:
        assert (a, c, tail) == (n, 1, 0)
        mp.mp.dps = 90
        lp = single_term_log_p(n)
        p = mp.exp(lp)
    else:
        mp.mp.dps = 60
        S, D = p_exact(a, c, n, tail)
        p = mp.mpf(S) / mp.mpf(D)
        lp = mp.log(p)
    return '{"fam":"%s","a":%d,"c":%d,"n":%d,"tail":%d,"p":"%s","log_p":"%s"}' % (
        fam, a, c, n, tail, mp.nstr(p, DIGITS), mp.nstr(lp, DIGITS))


def main():
    t0 = time.time()
    mp.mp.dps = 90
    for n in (2, 7, 50):   # the closed form against the integers
        S, D = p_exact(n, 1, n, 0)
        assert abs(single_term_log_p(n) - mp.log(mp.mpf(S) / mp.mpf(D))) < mp.mpf(10) ** -80
    rows = fd.tables()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        lines = pool.map(evaluate, rows, chunksize=4)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fisher_domain.json")
    with open(path, "w") as f:
        f.write('{"generator": "tests/golden/make_fisher_domain_golden.py", "dps": 60, "k_max": %d,\n"tables": [\n' % fd.K_MAX)
        f.write(",\n".join(lines))
        f.write("\n]}\n")
    count = {fam: sum(1 for r in rows if r[0] == fam) for fam in fd.FAMILIES}
    print("%d tables (%s; %d at tail 1), %.1f s" % (len(rows), ", ".join("%s %d" % kv for kv in count.items()),
                                                     sum(r[4] for r in rows), time.time() - t0))


if __name__ == "__main__":
    main()
