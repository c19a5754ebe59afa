"""The count domain of the general-margin Fisher routine (minorseq_amd/csrc/jl_fisher_general.h; docs/SPEC.md §21), as designed
tables and a branch census (test infrastructure, like fisher_domain.py; nothing of the product imports it).

`classify` restates WHICH piece of the header a table [[a, n - a], [c, m - c]] takes, as a set of labels; it computes no
p-value.  `tables` is the designed list behind tests/golden/fisher_general_domain.json (exact values:
make_fisher_general_domain_golden.py): no random draw decides whether a label is covered.
tests/test_fisher_general_domain_host.py proves with a census that every reachable label is reached, and
tests/test_gpu_fisher_general_domain.py sends the same tables through the kernels.

Labels:
  early_one                              a <= lo = max(0, K - m), K = a + c: p = 1 before anything is computed
  upper lower mean_exact                 a M >= n K: the upper tail from a | 1 - the lower tail from a - 1; a M == n K exactly
  lo_pos                                 K > m: the support starts at lo > 0
  direct                                 K <= 64 and the direct product is above 1e-280: the point mass is that product
  direct_fallback:{upper,lower}          K <= 64 but the product is at most 1e-280: the saddle-point form after all
  saddle                                 K > 64
  zero_cell:{x,c,nx,mc}                  jl_log_pmf_general with a cell of 0 (deviance = the mean, one factor 2 pi less)
  stirlerr:{tab,s4,s3,s2,s1}@{K,L,n,m,M,x,c,nx,mc}   which form of stirlerr each of its nine arguments takes
  bd0:{series,log}@{x,c,nx,mc}           which form of bd0 each cell that is not 0 takes
  batch16:{0..4}                         jl_pmf_general_small: renormalisations of the product (K // 16)
  break no_break                         the tail loop left at `term < sum * 1e-17` before its own end, or not
  p_zero p_denormal p_normal             from the exact ln p (given as `log_p`): below -745 the routine returns 0
  beyond_2^53                            one of the products K n, K m, L n, L m, a M, n K is above 2^53
In the names, the point mass is taken at x (= a on the upper path, a - 1 on the lower one) of the table [[x, nx], [c, mc]] with
x + c = K, x + nx = n, c + mc = m, L = M - K, M = n + m; `c` there is K - x."""
import json
import math
import os
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fisher_general_domain.json")

# the constants of jl_fisher_general.h and jl_fisher.h this module mirrors (test_fisher_general_domain_host.py reads them back)
K_DIRECT = 64                       # K <= 64: direct products ...
PMF_MIN = 1e-280                    # ... if they are above this
STIRLERR_LAST = (15, 35, 80, 500)   # the last argument of tab | s4 | s3 | s2; above 500: s1
BD0_SERIES = 0.1                    # |x - np| < 0.1 (x + np): the series
BREAK_EPS = 1e-17                   # term < sum * 1e-17: leave the tail loop
LOGP_ZERO = -745.0                  # ln p below it: p = 0
LOGP_GATE = -700.0                  # the skipping form looks at the point mass only above it
BATCH = 16                          # factors between two renormalisations
LN_DBL_MIN = -708.3964185322641     # ln 2^-1022: below it p is a denormal
TWO_53 = 2 ** 53
U32 = 2 ** 32 - 1
MAX_TABLES = 1500

STIRLERR_FORMS = ("tab", "s4", "s3", "s2", "s1")
STIRLERR_ARGS = ("K", "L", "n", "m", "M", "x", "c", "nx", "mc")
CELLS = ("x", "c", "nx", "mc")
FAMILIES = ("margins", "extreme", "switch", "mean", "underflow", "beyond")

# Labels no table of uint32 counts can take, with the reason; everything else in `all_labels` must be reached.
#   The saddle-point form is evaluated for K > 64, or for K <= 64 where the direct product is at most 1e-280.  The smallest
#   product a K allows is all K in a row of K reads against the largest other row, K! / prod_{i<K} (2^32 - 1 + K - i): 1.5e-273
#   for K = 32, 1.2e-281 for K = 33.  So the form sees K >= 33 and M >= K >= 33, and M <= 80 only with K > 64.
UNREACHABLE = {
    "stirlerr:tab@K": "K >= 33 wherever the saddle-point form is evaluated",
    "stirlerr:tab@M": "M >= K >= 33",
    "stirlerr:s4@M": "M <= 35 leaves products far above 1e-280, so K > 64 and M >= 65",
    "lower_is_one": "the lower path has a below the mean, where P(X <= a - 1) < 1 - P(X >= mean): the sum cannot pass 1",
}
# Two branches of jl_log_pmf_general have no label because no table reaches them: L = 0 means K = M, so lo = K - m = n >= a, and
# K = 0 means a = 0 = lo: both leave at early_one.


def all_labels():
    out = {"early_one", "upper", "lower", "mean_exact", "lo_pos", "direct", "direct_fallback:upper", "direct_fallback:lower",
           "saddle", "break", "no_break", "p_zero", "p_denormal", "p_normal", "beyond_2^53", "lower_is_one"}
    out |= {"zero_cell:%s" % v for v in CELLS}
    out |= {"stirlerr:%s@%s" % (f, v) for f in STIRLERR_FORMS for v in STIRLERR_ARGS}
    out |= {"bd0:%s@%s" % (f, v) for f in ("series", "log") for v in CELLS}
    out |= {"batch16:%d" % k for k in range(K_DIRECT // BATCH + 1)}
    return out - set(UNREACHABLE)


def stirlerr_form(v):
    if v <= STIRLERR_LAST[0]:
        return "tab"
    for last, form in zip(STIRLERR_LAST[1:], ("s4", "s3", "s2")):
        if v <= last:
            return form
    return "s1"


def bd0_form(x, np_):
    x, np_ = float(x), float(np_)
    return "series" if abs(x - np_) < BD0_SERIES * (x + np_) else "log"


def pmf_point(a, n, c, m):
    """(x, upper): where the routine takes the point mass, or None (early return)."""
    K = a + c
    if a <= max(K - m, 0):
        return None
    return (a, True) if a * (n + m) >= n * K else (a - 1, False)


def exact_pmf_small(x, K, n, m):
    """P(X = x) as a Fraction by the K factors of jl_pmf_general_small (for K <= 64)."""
    M = n + m
    num = math.comb(K, x) * math.prod(n - i for i in range(x)) * math.prod(m - i for i in range(K - x))
    return Fraction(num, math.prod(M - i for i in range(K)))


def takes_direct(x, K, n, m):
    """K <= 64 and the product above 1e-280.  A designed table stays 1 % away from that border (the double product is good to
    about K 1e-16), so that its last bits cannot decide."""
    if K > K_DIRECT:
        return False
    p = exact_pmf_small(x, K, n, m)
    assert not Fraction(PMF_MIN) * 99 / 100 < p < Fraction(PMF_MIN) * 101 / 100, ("too close to 1e-280", x, K, n, m)
    return p > Fraction(PMF_MIN)


def saddle_args(a, n, c, m):
    """The nine arguments of jl_log_pmf_general, or None where it is not evaluated (early return, direct product)."""
    pt = pmf_point(a, n, c, m)
    if pt is None:
        return None
    K, x = a + c, pt[0]
    if takes_direct(x, K, n, m):
        return None
    M = n + m
    return dict(K=K, L=M - K, n=n, m=m, M=M, x=x, c=K - x, nx=n - x, mc=m - (K - x))


def means(d):
    """{cell: the mean its deviance is taken against}, in the doubles of jl_mean_with_rest."""
    K, L, n, m, M = (float(d[k]) for k in ("K", "L", "n", "m", "M"))
    return {"x": K * n / M, "c": K * m / M, "nx": L * n / M, "mc": L * m / M}


def bd0_calls(a, n, c, m):
    """{cell: (value, mean)} of the bd0 calls of jl_log_pmf_general (the cells that are not 0), or None (see saddle_args)."""
    d = saddle_args(a, n, c, m)
    if d is None:
        return None
    mu = means(d)
    return {k: (d[k], mu[k]) for k in CELLS if d[k] > 0}


def _tail_breaks(x0, K, n, L, lo, hi, upper):
    """The tail loop in the routine's own IEEE doubles: does `break` fire while the loop would go on?"""
    K, n, L = float(K), float(n), float(L)
    term = total = 1.0
    x = float(x0)
    if upper:
        while x < hi:
            term *= ((K - x) * (n - x)) / ((x + 1.0) * (L - n + x + 1.0))
            total += term
            x += 1.0
            if term < total * BREAK_EPS:
                return x < hi
        return False
    while x > lo:
        term *= (x * (L - n + x)) / ((K - x + 1.0) * (n - x + 1.0))
        total += term
        x -= 1.0
        if term < total * BREAK_EPS:
            return x > lo
    return False


def classify(a, n, c, m, log_p=None):
    """The labels of the table; `log_p` (the exact ln p, optional) adds p_zero / p_denormal / p_normal."""
    assert 0 <= a <= n <= U32 and 0 <= c <= m <= U32 and n >= 1 and m >= 1
    out = set()
    K, M = a + c, n + m
    L = M - K
    lo, hi = max(K - m, 0), min(K, n)
    if K > m:
        out.add("lo_pos")
    if max(K * n, K * m, L * n, L * m, a * M) > TWO_53:
        out.add("beyond_2^53")
    if a <= lo:
        out.add("early_one")
        if log_p is not None:
            out.add("p_normal")
        return out
    x, upper = pmf_point(a, n, c, m)
    out.add("upper" if upper else "lower")
    if a * M == n * K:
        out.add("mean_exact")
    direct = takes_direct(x, K, n, m)
    if K <= K_DIRECT:
        out.add("batch16:%d" % (K // BATCH))
        out.add("direct" if direct else "direct_fallback:%s" % ("upper" if upper else "lower"))
    else:
        out.add("saddle")
    if not direct:
        d = saddle_args(a, n, c, m)
        for name in STIRLERR_ARGS:
            out.add("stirlerr:%s@%s" % (stirlerr_form(d[name]), name))
        mu = means(d)
        for name in CELLS:
            out.add("zero_cell:%s" % name if d[name] == 0 else "bd0:%s@%s" % (bd0_form(d[name], mu[name]), name))
    out.add("break" if _tail_breaks(x, K, n, L, lo, hi, upper) else "no_break")
    if log_p is not None:
        if upper and not direct:
            out.add("p_zero" if log_p < LOGP_ZERO else "p_denormal" if log_p < LN_DBL_MIN else "p_normal")
        else:
            out.add("p_normal")     # a direct product above 1e-280, or a tail that holds the mean
    return out


# ---------------------------------------------------------------------------------------------------------------- the design
def _isqrt_up(v):
    r = math.isqrt(v)
    return r if r * r == v else r + 1


def sigma_up(K, n, m):
    """An integer at or above the standard deviation of X ~ Hypergeometric(n + m, K, n) (and at least 1)."""
    M = n + m
    return max(1, _isqrt_up(-(-K * n * m * (M - K) // (M * M * max(M - 1, 1)))))


def counts_of(K, n, m):
    """The designed counts a of one (K, n, m): lo, lo + 1, either side of the mean, 4 sigma above it, hi."""
    M = n + m
    lo, hi = max(K - m, 0), min(K, n)
    mean, s = K * n // M, sigma_up(K, n, m)
    return sorted({min(max(v, lo), hi) for v in (lo, lo + 1, mean - 1, mean, mean + 1, mean + 2, mean + 4 * s, hi)})


MARGINS = ((1, 1), (1, 7), (7, 2), (30, 30), (65, 65), (50, 5000), (5000, 50), (2907, 29070), (29070, 2907), (100, 10 ** 6),
           (10 ** 6, 100), (10 ** 5, 10 ** 7), (10 ** 7, 10 ** 5), (10 ** 7, 10 ** 7), (1, 10 ** 7), (10 ** 7, 1))


def totals_of(n, m):
    """The designed K of one pair of rows: 1, 2, both sides of 64, 1 % and a third of all reads, lo > 0 from one read, from
    half of the sample's and almost everything."""
    M = n + m
    return sorted({K for K in (1, 2, 64, 65, M // 100, M // 3, m + 1, m + max(1, n // 2), M - 1) if 1 <= K <= M - 1})


def family_margins():
    """Row ratios 1:1, 1:3.5, 1:10, 1:100, 1:1e4, 1:1e7 and their inverses at coverages from 1 to 1e7."""
    return [(a, n, K - a, m) for n, m in MARGINS for K in totals_of(n, m) for a in counts_of(K, n, m)]


EXTREME = ((1000, 10 ** 7), (10 ** 7, 1000), (40, 4 * 10 ** 9), (4 * 10 ** 9, 40))


def family_extreme():
    """K = 1 .. 66 at 1:1e4, 1e4:1, 1:1e8 and 1e8:1: every observed count the table allows (a = hi) and the first count above the
    early return (a = lo + 1).  At 1:1e8 the first is the direct product's fallback on the upper path from K = 33, at 1e8:1 the
    second is the fallback on the lower path; (64, 640000) and its inverse reach both at 1e4."""
    out = []
    for n, m in EXTREME + ((64, 640000), (640000, 64)):
        for K in range(1, 67) if (n, m) in EXTREME else (62, 63, 64):
            lo, hi = max(K - m, 0), min(K, n)
            for a in sorted({hi, min(lo + 1, hi)}):
                out.append((a, n, K - a, m))
    out += [(64, 64, 0, 700000), (63, 63, 0, 10 ** 6), (1, 700000, 63, 64), (1, 10 ** 6, 62, 63)]   # both fallbacks below 1e6 + 1 reads
    out.append((1000, 1000, 0, 10 ** 8))      # the one such table the suite held before (test_control_host.py)
    return out


def table_at(x, K, n, m):
    """The table whose point mass the routine takes at x of Hypergeometric(n + m, K, n)."""
    M = n + m
    t = (x, n, K - x, m) if x * M >= n * K else (x + 1, n, K - x - 1, m)
    assert pmf_point(*t) is not None and pmf_point(*t)[0] == x, (x, K, n, m)
    return t


def family_switch():
    """Every stirlerr argument ON each border it can reach and one above it, every bd0 cell on the two integers either side of
    9/11 and of 11/9 of its mean (whole means: K = L = 4000 against rows of 2000 and 6000 reads)."""
    out = []
    for v in [b + s for b in STIRLERR_LAST for s in (0, 1)]:
        out.append(table_at(v, v + 200, 1000, 3000))                       # x
        out.append(table_at(300, 300 + v, 1000, 3000))                     # c
        out.append(table_at(100, 150, 100 + v, 3000))                      # nx
        out.append(table_at(50, 150, 1000, 100 + v))                       # mc
        out.append(table_at(52, 100, 50 + v - v // 2, 50 + v // 2))        # L = v at K = 100
        out.append(table_at(min(v, 5), 100, v, 1000))                      # n
        out.append(table_at(100 - min(v, 3), 100, 1000, v))                # m
        if v >= 80:
            out.append(table_at(v // 4 + 3, v, 1000, 3000))                # K on the saddle path
            out.append(table_at(35, 66, v // 2, v - v // 2))               # M
        if v in (35, 36):
            out.append((v, v, 0, 4 * 10 ** 9))                             # K below 65: through the fallback
    out += [table_at(35, 66, 35, 35), table_at(36, 66, 37, 38)]            # M = 70 and 75 (65 .. 80 is all of s3 that M can take)
    out += [table_at(99, 100, 1000, 20), table_at(99, 100, 1000, 30)]      # m inside s4
    out += [(33, 33, 0, U32), (34, 34, 0, U32), (34, 35, 0, U32)]          # the smallest K the fallback can see, and the next
    # why the direct product hands over at 1e-280 and not at the end of the normal range: these masses are 9e-300 .. 2e-298, and
    # the product before its last factor C(64, 26) = 6e17 would be a denormal of seven digits or fewer
    out += [(38, 38, 26, 3170000000), (38, 38, 26, 3 * 10 ** 9), (38, 39, 26, 3600000000), (38, 38, 25, 3100000000)]
    K, n, m = 4000, 2000, 6000
    for v in (818, 819, 1222, 1223):                                      # means of 1000
        out.append(table_at(v, K, n, m))                                   # x
        out.append(table_at(n - v, K, n, m))                               # nx
    for v in (2454, 2455, 3666, 3667):                                     # means of 3000
        out.append(table_at(K - v, K, n, m))                               # c
        out.append(table_at(K - (m - v), K, n, m))                         # mc
    return out


def family_mean():
    """a M == n K exactly, and one count to either side: K <= 64 and above, lo > 0, every product beyond 2^53."""
    out = []
    for a, n, c, m in ((3, 7, 3, 7), (10, 1000, 30, 3000), (100, 1000, 300, 3000), (1000, 10 ** 7, 10, 10 ** 5), (60, 100, 30, 50),
                       (20, 40, 2 * 10 ** 9, 4 * 10 ** 9), (2 * 10 ** 6, 2 * 10 ** 9, 10 ** 6, 10 ** 9),
                       (2 ** 26 + 1, 2 ** 31 - 1, 2 ** 26 + 1, 2 ** 31 - 1)):
        assert a * m == n * c
        out += [(a - 1, n, c, m), (a, n, c, m), (a + 1, n, c, m)]
    return out


def approx_log_p(a, n, c, m):
    """ln P(X >= a) above the mean in doubles (lgamma and the ratio recurrence): only to FIND the tables of the underflow family."""
    K, M = a + c, n + m
    lg = math.lgamma
    l0 = (lg(K + 1) - lg(a + 1) - lg(c + 1) + lg(n + 1) - lg(n - a + 1) + lg(m + 1) - lg(m - c + 1)
          - (lg(M + 1) - lg(M - K + 1)))
    term = total = 1.0
    for x in range(a, min(K, n)):
        term *= ((K - x) * (n - x)) / ((x + 1.0) * (M - K - n + x + 1.0))
        total += term
        if term < total * 1e-17:
            break
    return l0 + math.log(total)


UNDERFLOW_RANGES = ((-700.0, -690.0), (-745.0, -708.0), (-760.0, -745.0), (-math.inf, -1e4))


def family_underflow():
    """Upper-tail tables whose ln p lies in (-700, -690) (the gate of the skipping form looks at l0 > -700), (-745, -708) (p is a
    denormal), (-760, -745) (p = 0 with a finite log_p) and below -10^4, found by walking a upwards at a fixed control count."""
    out = []
    for n, c, m in ((2907, 1, 29070), (10 ** 5, 30, 10 ** 7), (10 ** 7, 1000, 10 ** 7), (10 ** 6, 0, 10 ** 4)):
        for lo_, hi_ in UNDERFLOW_RANGES:
            want = 0.5 * (lo_ + hi_) if lo_ > -math.inf else 1.2 * hi_
            x0, x1 = c * n // m + 2, n           # ln p falls as a grows: the first a below `want`, then the nearer neighbour
            if approx_log_p(n, n, c, m) >= want:
                continue
            while x0 < x1:
                mid = (x0 + x1) // 2
                if approx_log_p(mid, n, c, m) < want:
                    x1 = mid
                else:
                    x0 = mid + 1
            a = min((x0 - 1, x0), key=lambda v: abs(approx_log_p(v, n, c, m) - want))
            if lo_ + 1.0 < approx_log_p(a, n, c, m) < hi_ - 1.0 or (lo_ == -math.inf and approx_log_p(a, n, c, m) < hi_ - 1.0):
                out.append((a, n, c, m))
    out.append((10 ** 7, 10 ** 7, 1, 10 ** 7))     # every read of the sample
    return out


BEYOND_ROWS = ((10 ** 8, 2 * 10 ** 9), (2 * 10 ** 9, 10 ** 8), (2 * 10 ** 9, 2 * 10 ** 9), (10 ** 9 + 7, 1500000011),
               (2 ** 31 - 1, 2 ** 31 - 1), (U32, U32))


def family_beyond():
    """Rows of 1e8 to 2e9 reads (and the largest the ABI takes): L n is above 2^53 in every one of them, K n and a M from
    K = 3e7.  Counts from the mean to 30 sigma above it, the ends of the support where the table is small enough to matter."""
    out = []
    for n, m in BEYOND_ROWS:
        M = n + m
        for K in (10, 100, 5000, 10 ** 6, 3 * 10 ** 7):
            mean, s = K * n // M, sigma_up(K, n, m)
            lo, hi = max(K - m, 0), min(K, n)
            cand = [lo + 1, mean - 1, mean, mean + 1, mean + 2 * s, mean + 6 * s, mean + 30 * s] + ([hi] if K <= 5000 else [])
            for a in sorted({min(max(v, lo), hi) for v in cand}):
                out.append((a, n, K - a, m))
    return out


def tables():
    """[(family, a, n, c, m)], each table once (under the first family that holds it)."""
    out, seen = [], set()
    for fam, rows in (("margins", family_margins()), ("extreme", family_extreme()), ("switch", family_switch()),
                      ("mean", family_mean()), ("underflow", family_underflow()), ("beyond", family_beyond())):
        for t in rows:
            a, n, c, m = t
            assert 0 <= a <= n <= U32 and 0 <= c <= m <= U32 and n >= 1 and m >= 1, t
            if t not in seen:
                seen.add(t)
                out.append((fam,) + t)
    return out


def load_fixture():
    """The fixture's tables as dicts: fam, a, n, c, m, p and log_p (the 25-digit strings), labels."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    for t in fx["tables"]:
        t["labels"] = classify(t["a"], t["n"], t["c"], t["m"], float(t["log_p"]))
    return fx
