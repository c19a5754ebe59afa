"""The rule of docs/SPEC.md §16 in plain numpy over uint8[N][L] rows: at every codon start the reads with a whole codon, a whole-codon
deletion, a partly deleted codon, and the reads spanning it.  It shares nothing with the device code — no planes, no bit words —
so that what the tests compare the device with is the rule's own text.
The test of one position is exact: the hypergeometric tail in Python integers and fractions.Fraction, the expected
count by the same IEEE double product and rounding as the library, every decision in exact arithmetic."""
import math
from fractions import Fraction

import numpy as np

CODON, DEL3, PARTIAL, SPAN = 0, 1, 2, 3


def counts(rows):
    """rows uint8[N][L] (codes of SPEC §1) -> uint32[L - 2][4] = (codon, del3, partial, span) per codon start."""
    rows = np.asarray(rows)
    n_cols = rows.shape[1]
    out = np.zeros((max(0, n_cols - 2), 4), dtype=np.uint32)
    for c in range(n_cols - 2):
        three = rows[:, c:c + 3].astype(np.int64)
        base, gap, n, out_ = (three < 4), (three == 4), (three == 5), (three == 6)
        out[c, CODON] = base.all(axis=1).sum()
        out[c, DEL3] = gap.all(axis=1).sum()
        out[c, PARTIAL] = (~out_.any(axis=1) & ~n.any(axis=1) & gap.any(axis=1) & base.any(axis=1)).sum()
        out[c, SPAN] = (~out_.any(axis=1)).sum()
    return out


def expected(coverage, rate, round_mode):
    """round_mode(coverage * rate) clamped to [0, coverage]: the product in IEEE double, 0 ceil, 1 floor, 2 floor(x + 0.5)."""
    x = float(coverage) * float(rate)
    r = math.floor(x) if round_mode == 1 else math.floor(x + 0.5) if round_mode == 2 else math.ceil(x)
    return int(min(max(r, 0), coverage))


def tail(a, e, n, two_sided):
    """The p of the table [[a, n - a], [e, n - e]], exact: X ~ Hypergeometric(2n, a + e, n); one-sided P(X >= a), two-sided the sum
    of the probabilities of all tables no more likely than the observed one.  The masses are kept as integers over one common
    denominator, from the ratio P(x + 1) / P(x) = (K - x)(n - x) / ((x + 1)(n - K + x + 1)): their sum is that denominator's share
    of 1, so no binomial coefficient of 2n is ever formed."""
    k = a + e
    lo, hi = max(0, k - n), min(k, n)
    num = [(k - x) * (n - x) for x in range(lo, hi)]
    den = [(x + 1) * (n - k + x + 1) for x in range(lo, hi)]
    before, after = [1], [1]                                 # products of num below x, of den from x on
    for v in num:
        before.append(before[-1] * v)
    for v in reversed(den):
        after.append(after[-1] * v)
    after.reverse()
    mass = {lo + i: before[i] * after[i] for i in range(hi - lo + 1)}
    total = sum(mass.values())
    if two_sided:
        return Fraction(sum(m for m in mass.values() if m <= mass[a]), total)
    return Fraction(sum(m for x, m in mass.items() if x >= a), total)


def test(cnt, rate, n_tests, alpha=0.01, round_mode=0, two_sided=False, min_perc=-1.0, max_perc=-1.0):
    """One position: dict(count, coverage, expected, partial, called, p (Fraction, unadjusted), p_adj (Fraction))."""
    codon, del3, partial = int(cnt[CODON]), int(cnt[DEL3]), int(cnt[PARTIAL])
    cov = codon + del3
    out = dict(count=del3, coverage=cov, expected=0, partial=partial, called=False, p=Fraction(1), p_adj=Fraction(1))
    if cov == 0:
        return out
    e = expected(cov, rate, round_mode)
    p = tail(del3, e, cov, two_sided)
    p_adj = min(Fraction(1), p * Fraction(n_tests))
    called = del3 > 0 and p_adj < Fraction(alpha)
    if min_perc >= 0 and not Fraction(100 * del3, cov) > Fraction(min_perc):
        called = False
    if max_perc >= 0 and not Fraction(100 * del3, cov) < Fraction(max_perc):
        called = False
    out.update(expected=e, called=called, p=p, p_adj=p_adj)
    return out


test.__test__ = False   # (not a pytest test, whatever its name)


def smallest_called(coverage, rate, n_tests, alpha=0.01, round_mode=0, two_sided=False):
    """The smallest del3 above the expected count that the exact test calls at codon + del3 = coverage."""
    for d in range(expected(coverage, rate, round_mode) + 1, coverage + 1):
        if test((coverage - d, d, 0, coverage), rate, n_tests, alpha, round_mode, two_sided)["called"]:
            return d
    raise AssertionError("no count is called")
