"""The count domain of the Fisher routines (minorseq_amd/csrc/jl_fisher.h), as designed tables and a branch census (test
infrastructure, like call_edges.py; nothing of the product imports it).

`classify` restates WHICH piece of jl_fisher.h a table [[a, n - a], [c, n - c]] takes, as a set of labels; it computes no
p-value.  `tables` is the designed list behind tests/golden/fisher_domain.json (exact values: make_fisher_domain_golden.py):
no random draw decides whether a label is covered.  tests/test_fisher_domain_host.py proves with a census that every label is
reached, and tests/test_gpu_fisher_domain.py sends the same tables through the kernels.

Labels:
  early_one                                   a <= lo = max(0, K - n), K = a + c: p = 1 before anything is computed
  direct_upper direct_lower                   K <= 64: products; the tail above the mean (a > c) | 1 - the tail below it
  saddle_upper saddle_lower                   K > 64: the saddle-point point mass
  lo_pos                                      K > n: the support starts at lo > 0
  zero_arg:{x,c,nx,nc}                        the point mass is asked for at a corner of the table (jl_log_pmf_equal_rows' fallback)
  stirlerr:{tab,s4,s3,s2,s1}@{K,L,n,M,x,c,nx,nc}   which form of stirlerr each of its eight arguments takes (saddle path)
  bd0:{series,log}@{x,c,nx,nc}                which form of bd0 each of its four arguments takes (saddle path)
  batch16:{0..4}  binom_m:{<=16,>16}          jl_pmf_equal_rows_small: renormalisations, factors of the binomial coefficient
  break no_break                              saddle path: the tail loop left at `term < sum * 1e-17` before its own end, or not
  p_zero p_denormal p_normal                  from the exact ln p (given as `log_p`): below -745 the routine returns 0
  two:{a<c,a==c,a>c}                          tail = 1
In the names, the point mass is taken at x (= a on the upper path, a - 1 on the lower one) of the table
[[x, nx], [c, nc]] with x + c = K, x + nx = c + nc = n, L = 2n - K, M = 2n; `c` there is K - x, not the expected count."""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fisher_domain.json")

# the constants of jl_fisher.h this module mirrors (test_fisher_domain_host.py reads them back from the header)
K_DIRECT = 64                       # K <= 64: direct products
STIRLERR_LAST = (15, 35, 80, 500)   # the last argument of tab | s4 | s3 | s2; above 500: s1
BD0_SERIES = 0.1                    # |x - np| < 0.1 (x + np): the series
BREAK_EPS = 1e-17                   # term < sum * 1e-17: leave the tail loop
LOGP_ZERO = -745.0                  # ln p below it: p = 0
BATCH = 16                          # factors between two renormalisations
LN_DBL_MIN = -708.3964185322641     # ln 2^-1022: below it p is a denormal
K_MAX = 20000                       # the generator's bound on K (exact integers of K factors; a few minutes in all)
K_TWO_SIDED = 4000                  # the first two families enter at tail = 1 up to this K

STIRLERR_FORMS = ("tab", "s4", "s3", "s2", "s1")
STIRLERR_ARGS = ("K", "L", "n", "M", "x", "c", "nx", "nc")
BD0_ARGS = ("x", "c", "nx", "nc")
FAMILIES = ("lo_pos", "fraction", "switch", "direct", "underflow")

# Labels no valid table (a, c <= n) can take, with the reason; everything else in `all_labels` must be reached.
#   K > 64 on the saddle path, M = 2n >= K, n >= K / 2 > 32
UNREACHABLE = {"stirlerr:tab@K", "stirlerr:s4@K",                         # K >= 65
               "stirlerr:tab@M", "stirlerr:s4@M",                         # M >= 66
               "stirlerr:tab@n"}                                          # n >= 33


def all_labels():
    out = {"early_one", "direct_upper", "direct_lower", "saddle_upper", "saddle_lower", "lo_pos", "break", "no_break",
           "p_zero", "p_denormal", "p_normal", "binom_m:<=16", "binom_m:>16", "two:a<c", "two:a==c", "two:a>c"}
    out |= {"zero_arg:%s" % v for v in BD0_ARGS}
    out |= {"stirlerr:%s@%s" % (f, v) for f in STIRLERR_FORMS for v in STIRLERR_ARGS}
    out |= {"bd0:%s@%s" % (f, v) for f in ("series", "log") for v in BD0_ARGS}
    out |= {"batch16:%d" % k for k in range(K_DIRECT // BATCH + 1)}
    return out - UNREACHABLE


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


def pmf_point(a, c, n):
    """(x, upper): where the routine takes the point mass, or None (early return)."""
    K = a + c
    if a <= max(K - n, 0):
        return None
    return (a, True) if a > c else (a - 1, False)


def saddle_args(a, c, n):
    """The eight arguments of jl_log_pmf_equal_rows' main expression, or None where it is not evaluated (early return, direct
    products, the zero-argument fallback)."""
    K = a + c
    pt = pmf_point(a, c, n)
    if pt is None or K <= K_DIRECT:
        return None
    x = pt[0]
    d = dict(K=K, L=2 * n - K, n=n, M=2 * n, x=x, c=K - x, nx=n - x, nc=n - (K - x))
    return None if 0 in (d["x"], d["c"], d["nx"], d["nc"]) else d


def bd0_calls(a, c, n):
    """{argument: (value, np)} of the four bd0 calls of the main expression, or None (see saddle_args)."""
    d = saddle_args(a, c, n)
    if d is None:
        return None
    return {"x": (d["x"], d["K"] / 2), "c": (d["c"], d["K"] / 2), "nx": (d["nx"], d["L"] / 2), "nc": (d["nc"], d["L"] / 2)}


def _log_binom_half_labels(out, x, N, names):
    """log_binom_half(x, N): names = (N, x, N - x) as labels."""
    if N == 0 or x == 0 or x == N:
        return
    for v, name in zip((N, x, N - x), names):
        out.add("stirlerr:%s@%s" % (stirlerr_form(v), name))
    out.add("bd0:%s@%s" % (bd0_form(x, N / 2), names[1]))
    out.add("bd0:%s@%s" % (bd0_form(N - x, N / 2), names[2]))


def _tail_breaks(x0, K, n, lo, hi, upper):
    """The tail loop of the saddle path in the routine's own IEEE doubles: does `break` fire while the loop would go on?"""
    K, n = float(K), float(n)
    term = total = 1.0
    x = float(x0)
    if upper:
        while x < hi:
            term *= ((K - x) * (n - x)) / ((x + 1.0) * (n - K + x + 1.0))
            total += term
            x += 1.0
            if term < total * BREAK_EPS:
                return x < hi
        return False
    while x > lo:
        term *= (x * (n - K + x)) / ((K - x + 1.0) * (n - x + 1.0))
        total += term
        x -= 1.0
        if term < total * BREAK_EPS:
            return x > lo
    return False


def classify(a, c, n, tail=0, log_p=None):
    """The labels of the table at `tail`; `log_p` (the exact ln p, optional) adds p_zero / p_denormal / p_normal."""
    assert 0 <= a <= n and 0 <= c <= n and n >= 1
    out = set()
    if tail == 1:
        out.add("two:a<c" if a < c else "two:a==c" if a == c else "two:a>c")
        if a == c:
            if log_p is not None:
                out.add("p_normal")
            return out
        a, c = max(a, c), min(a, c)
        if log_p is not None and log_p < 0.0:
            log_p -= math.log(2.0)   # the one-sided value the routine doubles
    K = a + c
    lo, hi = max(K - n, 0), min(K, n)
    if K > n:
        out.add("lo_pos")
    if a <= lo:
        out.add("early_one")
        if log_p is not None:
            out.add("p_normal")
        return out
    x, upper = pmf_point(a, c, n)
    if K <= K_DIRECT:
        out.add("direct_upper" if upper else "direct_lower")
        out.add("batch16:%d" % (K // BATCH))
        out.add("binom_m:<=16" if min(x, K - x) <= 16 else "binom_m:>16")
        if log_p is not None:
            out.add("p_normal")    # the smallest direct-product mass is about 2^-64
        return out
    out.add("saddle_upper" if upper else "saddle_lower")
    cc, nx, nc, L, M = K - x, n - x, n - (K - x), 2 * n - K, 2 * n
    zero = [name for name, v in zip(BD0_ARGS, (x, cc, nx, nc)) if v == 0]
    if zero:
        out |= {"zero_arg:%s" % name for name in zero}
        _log_binom_half_labels(out, x, K, ("K", "x", "c"))
        _log_binom_half_labels(out, nx, L, ("L", "nx", "nc"))
        out.add("stirlerr:%s@M" % stirlerr_form(M))      # log_binom_half(n, M): bd0(n, n) is the series at its first term
        out.add("stirlerr:%s@n" % stirlerr_form(n))
    else:
        for name, v in zip(STIRLERR_ARGS, (K, L, n, M, x, cc, nx, nc)):
            out.add("stirlerr:%s@%s" % (stirlerr_form(v), name))
        for name, (v, np_) in bd0_calls(a, c, n).items():
            out.add("bd0:%s@%s" % (bd0_form(v, np_), name))
    out.add("break" if _tail_breaks(x, K, n, lo, hi, upper) else "no_break")
    if log_p is not None:
        if not upper:
            out.add("p_normal")    # at or below the mean: p >= 1/2
        else:
            out.add("p_zero" if log_p < LOGP_ZERO else "p_denormal" if log_p < LN_DBL_MIN else "p_normal")
    return out


# ---------------------------------------------------------------------------------------------------------------- the design
def _ceil_sqrt(v):
    r = math.isqrt(v)
    return r if r * r == v else r + 1


def family_lo_pos():
    """a + c > n.  For every n the excess lo = a + c - n in {1, 2, n/2, n - 1, n}; a from lo (the early return: a <= lo needs
    c >= n, so it is a == lo with c == n; a == lo - 1 would need c = n + 1) over lo + 1, lo + 2, both sides of a == c, to n."""
    out = []
    for n in (1, 2, 7, 40, 63, 64, 65, 100, 1000):
        for lo in sorted({1, 2, n // 2, n - 1, n}):
            if not 1 <= lo <= n:
                continue
            K = n + lo
            for a in sorted({lo, lo + 1, lo + 2, K // 2 - 1, K // 2, K // 2 + 1, (K + 1) // 2 + 1, n - 1, n}):
                if lo <= a <= n:
                    out.append((a, K - a, n))
        out.append((n, n, n))
    return out


FRACTIONS = ((2, 1000), (1, 100), (5, 100), (25, 100), (50, 100), (90, 100), (1, 1))


def fraction_count(n, num, den):
    return max(1, (n * num + den // 2) // den)


def family_fraction():
    """Expected fractions c / n from 0.2 % to 100 %, counts from 1 over the expected one and its 1 and 4 sigma to n."""
    out = []
    for n in (64, 65, 1000, 2907, 20000, 100000):
        for num, den in FRACTIONS:
            c = fraction_count(n, num, den)
            s = _ceil_sqrt(c)
            for a in sorted({min(max(v, 0), n) for v in (1, c // 2, c - 1, c, c + 1, c + s, c + 4 * s, 2 * c, n)}):
                if a + c <= K_MAX:
                    out.append((a, c, n))
    return out


def _table_at(x, cc, n):
    """The table whose point mass is taken at [[x, n - x], [cc, n - cc]]: on the upper path (x > cc) or the lower one."""
    if x > cc:
        return (x, cc, n)
    assert cc >= x + 2
    return (x + 1, cc - 1, n)


def family_switch():
    """Every stirlerr argument on each side of every border it can reach with K > 64, every bd0 argument just inside and just
    outside 9/11 and 11/9 of its mean."""
    out = []
    for v in [b + s for b in STIRLERR_LAST for s in (0, 1)]:
        out.append(_table_at(v, 200, 1000))                 # x
        out.append(_table_at(200, v, 1000))                 # c
        out.append(_table_at(200, 100, 200 + v))            # nx
        out.append(_table_at(100, 200, 200 + v))            # nc
        K = 600 - v                                         # L = v at n = 300
        out.append(_table_at(K // 2 + 3, K - K // 2 - 3, 300))
        if v >= 80:                                         # K
            out.append(_table_at(v // 2 + 5, v - v // 2 - 5, 1000))
        if v >= 35:                                         # n, and M = 2n on each side of 80 and 500 (M is even)
            for n in (v,) + ((v // 2, v // 2 + 1) if v in (80, 500) else ()):
                for K in (k + max(66, min(2 * n - 4, n + 40)) for k in (0, -1, 1)):
                    out.append(_table_at(K // 2 + 1, K - K // 2 - 1, n))
    # bd0: np = 1000; 818 | 819 and 1222 | 1223 are the integers either side of 9/11 and 11/9
    for v in (818, 819, 1222, 1223):
        out.append(_table_at(v, 2000 - v, 5000))            # x
        out.append(_table_at(2000 - v, v, 5000))            # c
        out.append(_table_at(5000 - v, 3000 + v, 5000))     # nx: K = 8000, L = 2000
        out.append(_table_at(3000 + v, 5000 - v, 5000))     # nc
    return out


def family_direct():
    """K <= 64 at every multiple of the 16 factors between renormalisations and either side of it, x at both ends and in the
    middle, n from K (every read in the table) to 10^7; K = 65, 66 for the other side."""
    out = []
    for K in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66):
        for n in (K, K + 1, 2907, 10 ** 7):
            for a in sorted({0, 1, K // 2, K - 1, K}):
                if 0 <= a <= min(K, n) and K - a <= n:
                    out.append((a, K - a, n))
    return out


def approx_log_p(a, c, n):
    """ln P(X >= a), a > c, in doubles (lgamma and the ratio recurrence): only to FIND the tables of the underflow family."""
    K = a + c
    lg = math.lgamma
    l0 = (lg(K + 1) - lg(a + 1) - lg(c + 1) + 2 * lg(n + 1) - lg(n - a + 1) - lg(n - c + 1)
          - (lg(2 * n + 1) - lg(2 * n - K + 1)))
    term = total = 1.0
    for x in range(a, min(K, n)):
        term *= ((K - x) * (n - x)) / ((x + 1.0) * (n - K + x + 1.0))
        total += term
        if term < total * 1e-17:
            break
    return l0 + math.log(total)


UNDERFLOW_RANGES = ((-700.0, -690.0), (-745.0, -708.0), (-760.0, -745.0), (-math.inf, -1e4))


def family_underflow():
    """Upper-tail tables whose ln p lies in (-700, -690) (the gate of the skipping form looks at l0 > -700), (-745, -708) (p is a
    denormal), (-760, -745) (p = 0 with a finite log_p) and below -10^4, found by walking a upwards; a = n = 10^7 against c = 1."""
    out = []
    for n in (2907, 100000):
        for c in (1, 30):
            top = min(n, K_MAX - c)
            for lo_, hi_ in UNDERFLOW_RANGES:
                want = 0.5 * (lo_ + hi_) if lo_ > -math.inf else 1.2 * hi_
                x0, x1 = c + 1, top            # ln p falls as a grows: the first a below `want`, then the nearer neighbour
                if approx_log_p(top, c, n) >= want:
                    continue
                while x0 < x1:
                    mid = (x0 + x1) // 2
                    if approx_log_p(mid, c, n) < want:
                        x1 = mid
                    else:
                        x0 = mid + 1
                a = min((x0 - 1, x0), key=lambda v: abs(approx_log_p(v, c, n) - want))
                if lo_ + 1.0 < approx_log_p(a, c, n) < hi_ - 1.0 or (lo_ == -math.inf and approx_log_p(a, c, n) < hi_ - 1.0):
                    out.append((a, c, n))
    out.append((10 ** 7, 1, 10 ** 7))          # K = 10^7 + 1: one term; its exact value comes from a closed form
    return out


def tables():
    """[(family, a, c, n, tail)], each (a, c, n, tail) once (under the first family that holds it)."""
    out, seen = [], set()

    def add(fam, rows, tail):
        for a, c, n in rows:
            if (a, c, n, tail) not in seen:
                seen.add((a, c, n, tail))
                out.append((fam, a, c, n, tail))

    fams = (("lo_pos", family_lo_pos()), ("fraction", family_fraction()), ("switch", family_switch()),
            ("direct", family_direct()), ("underflow", family_underflow()))
    for fam, rows in fams:
        add(fam, rows, 0)
    for fam, rows in fams[:2]:
        add(fam, [r for r in rows if r[0] + r[1] <= K_TWO_SIDED], 1)
    return out


def load_fixture():
    """The fixture's tables as dicts: fam, a, c, n, tail, p and log_p (the 17-digit strings), labels."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    for t in fx["tables"]:
        t["labels"] = classify(t["a"], t["c"], t["n"], t["tail"], float(t["log_p"]))
    return fx
