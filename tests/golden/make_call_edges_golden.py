#!/usr/bin/env python3
"""Generates tests/golden/call_edges.json: designed codon positions whose call decision lies at an edge (the Bonferroni-adjusted
p next to alpha, counts at the expected count, ties of the majority codon, percentages equal to a filter bound, DRM masks at
codon 0 and 63), decided in exact arithmetic.  Needs mpmath (for printing the 60-digit values only); the tests read the JSON.

How the numbers are made (docs/SPEC.md §4-7):
  * `expected` is SPEC §5 in IEEE double as written there (Python floats: products left to right, ceil / floor / nearest, clamp).
  * p is a rational: with both rows summing to n, P(X = x) = w(x) / D with the integers
        w(x) = C(K, x) * n!/(n-x)! * n!/(n-K+x)!,   D = (2n)!/(2n-K)!,   K = a + c,
    w walked by its integer ratio recurrence from ONE product (K factors each, however deep the coverage).  Upper tail: the sum
    over x >= a.  Two-sided: the sum over all x with w(x) <= w(a), the definition, not the symmetry the device uses.
  * alpha and n_tests are the exact rationals of their doubles; `p * n_tests < alpha` is decided on integers.
  * A codon whose exact p_adj / alpha is within 1e-6 of 1 does not enter (the gate's own margin in jl_fisher.h); the number of
    positions dropped for it is recorded and must be 0.
  * p_adj = min(1, p n_tests) and log_p = ln p are printed from the rationals at 60 digits, 17 significant digits kept.

Run time: about 1 s (everything is small-integer arithmetic; no binomial of the coverage is ever formed).
"""
import json
import math
import os
import sys
import time
from fractions import Fraction

import mpmath as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from call_edges import CALLED, ERROR_MODELS, FILTERED, NOT_SIGNIFICANT, n_substituted  # noqa: E402

mp.mp.dps = 60
DIGITS = 17
CUSTOM = (0.99, 0.03, 0.0)          # e = 30 at coverage 1000, 32 at 1075 for one substituted base
CLAMP_HI = (0.999, 1.0001, 0.0)     # three substituted bases: coverage * P_err > coverage, e clamped to the coverage
CLAMP_EQ = (0.999, 0.9999, 0.0)     # e = ceil(coverage * 0.9997..) = coverage without the clamp


def expected(cov, ref, j, err, rnd):
    match, sub = err[0], err[1]
    perr = 1.0
    for sh in (4, 2, 0):
        perr = perr * (match if ((ref >> sh) & 3) == ((j >> sh) & 3) else sub)
    x = float(cov) * perr
    r = math.floor(x) if rnd == 1 else (math.floor(x + 0.5) if rnd == 2 else math.ceil(x))
    return int(min(max(r, 0), cov))


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


class Dropped(Exception):
    pass


def decide(S, D, n_tests, alpha):
    """exact p_adj < alpha; raises Dropped inside the 1e-6 margin."""
    nt, al = Fraction(n_tests), Fraction(alpha)
    padj = min(Fraction(1), Fraction(S, D) * nt)
    if abs(padj / al - 1) < Fraction(1, 10 ** 6):
        raise Dropped
    return padj < al


def significant(h, e, cov, prm):
    S, D = p_exact(h, e, cov, prm["tail"])
    return decide(S, D, prm["n_tests"], prm["alpha"])


def err_of(prm):
    return ERROR_MODELS[prm["err"]] if isinstance(prm["err"], str) else tuple(prm["err"])


def params(alpha=0.01, n_tests=1000.0, err="sequel", expected_round=0, tail=0, min_perc=-1.0, max_perc=-1.0):
    return dict(alpha=alpha, n_tests=float(n_tests), err=err if isinstance(err, str) else list(err), expected_round=expected_round,
                tail=tail, min_perc=min_perc, max_perc=max_perc)


def codons_of_class(ref, s):
    return [j for j in range(64) if n_substituted(ref, j) == s]


def edge_up(cov, e, prm, start=1):
    """smallest count >= start that is significant, or None; counts above it stay significant (checked for the next one)."""
    for h in range(start, min(cov, e + 400) + 1):
        if significant(h, e, cov, prm):
            assert h == cov or significant(h + 1, e, cov, prm)
            return h
    return None


# ---------------------------------------------------------------------------------------------------------------- families
def family_a(out):
    """h* - 1 and h* for every combination of coverage, n_tests, alpha, error-model row and number of substituted bases."""
    REF = 27   # CGT
    for cov in (1, 2, 7, 64, 65, 1000, 2907, 17241, 17242, 17300, 100000):
        for n_tests in (1, 50, 1000, 1884):
            for alpha in (0.01, 0.05, 0.3):
                for err in ("sequel", "permissive"):
                    prm = params(alpha, n_tests, err)
                    items = []   # (class, count)
                    for s in (1, 2, 3):
                        e = expected(cov, REF, codons_of_class(REF, s)[0], ERROR_MODELS[err], 0)
                        hs = edge_up(cov, e, prm)
                        if cov == 2907 and err == "sequel" and alpha == 0.01 and s == 1 and 982 <= n_tests <= 1884:
                            assert hs == 21, hs   # SPEC §5 anchor
                        if hs is None:
                            items.append((s, cov))      # no count is called: the largest one there is
                        else:
                            if hs > 1:
                                items.append((s, hs - 1))
                            items.append((s, hs))
                    # as many of them to a position as its coverage holds (two codons per class and position)
                    while items:
                        hist, used, left, rest = {}, {1: 0, 2: 0, 3: 0}, cov, []
                        for s, h in items:
                            if h <= left and used[s] < 2:
                                hist[codons_of_class(REF, s)[used[s]]] = h
                                used[s] += 1
                                left -= h
                            else:
                                rest.append((s, h))
                        if left:
                            hist[REF] = left
                        out.append(dict(family="a", ref=REF, hist=hist, prm=prm))
                        items = rest


def family_a_rounding(out):
    """`expected` where it steps, at the three rounding modes: the coverages either side of ceil's 1 -> 2 and of nearest's 0 -> 1."""
    REF, err = 6, ERROR_MODELS["sequel"]
    j = codons_of_class(REF, 1)[0]
    c2 = next(c for c in range(17000, 17400) if expected(c, REF, j, err, 0) == 2)
    c1 = next(c for c in range(8500, 8800) if expected(c, REF, j, err, 2) == 1)
    assert expected(c2 - 1, REF, j, err, 0) == 1 and expected(c1 - 1, REF, j, err, 2) == 0 and expected(c2, REF, j, err, 1) == 1
    for rnd in (0, 1, 2):
        prm = params(0.01, 1000, "sequel", expected_round=rnd)
        for cov in (c1 - 1, c1, c2 - 1, c2):
            e = expected(cov, REF, j, err, rnd)
            hs = edge_up(cov, e, prm)
            a, b = codons_of_class(REF, 1)[:2]
            out.append(dict(family="a", ref=REF, hist={a: hs - 1, b: hs, REF: cov - 2 * hs + 1}, prm=prm))


def family_b(out):
    """K = a + c across 64 | 65 (direct products | saddle-point form) with the edge inside: alpha is the geometric mean of the
    exact p of the two counts."""
    REF = 57
    a, b = codons_of_class(REF, 1)[:2]
    for cov, e_want, k_stars in ((1000, 30, (64, 65, 66)), (1075, 32, (65, 66, 67))):
        assert expected(cov, REF, a, CUSTOM, 0) == e_want
        for ks in k_stars:
            hs = ks - e_want
            p1, p0 = (Fraction(*p_exact(h, e_want, cov, 0)) for h in (hs, hs - 1))
            alpha = float(mp.sqrt(mp.mpf(p1.numerator) / p1.denominator * mp.mpf(p0.numerator) / p0.denominator))
            prm = params(alpha, 1, CUSTOM)
            assert significant(hs, e_want, cov, prm) and not significant(hs - 1, e_want, cov, prm)
            out.append(dict(family="b", ref=REF, hist={a: hs - 1, b: hs, REF: cov - 2 * hs + 1}, prm=prm))


def family_c(out):
    """Counts at or below the expected one: behind the shortcut (n_tests / 2 >= alpha) and in front of it."""
    REF = 0
    js = codons_of_class(REF, 1)
    counts = (33, 30, 29, 27, 24, 20, 12, 3)   # e = 30 (31 against 30 is p = 1/2 exactly, by symmetry)
    hist = dict(zip(js, counts))
    hist[REF] = 1000 - sum(counts)
    for alpha, n_tests in ((0.01, 1000), (0.9, 2), (0.5, 1), (0.9, 1), (0.3, 0.5), (0.6, 1), (0.45, 0.75)):
        out.append(dict(family="c", ref=REF, hist=dict(hist), prm=params(alpha, n_tests, CUSTOM)))
    # e = 1 (sequel, ceil), one read of the codon
    for alpha, n_tests in ((0.01, 1000), (0.9, 1), (0.3, 0.5)):
        for cov in (64, 2907):
            out.append(dict(family="c", ref=REF, hist={js[0]: 1, js[1]: 2, REF: cov - 3}, prm=params(alpha, n_tests)))


def family_d(out):
    """tail = 1: the edge above the expected count, the edge below it, and a == c."""
    REF = 42
    js = codons_of_class(REF, 1)
    for alpha, n_tests in ((0.05, 1), (0.05, 50), (0.01, 1000)):
        prm = params(alpha, n_tests, CUSTOM, tail=1)
        cov, e = 1000, 30
        up = edge_up(cov, e, prm, start=e + 1)
        below = [h for h in range(1, e) if significant(h, e, cov, prm)]
        hist = {js[0]: up - 1, js[1]: up, js[2]: e}
        if below:
            lo = max(below)
            assert all(significant(h, e, cov, prm) for h in range(1, lo + 1))
            hist[js[3]], hist[js[4]] = lo, lo + 1
        else:
            hist[js[3]] = 1
        hist[REF] = cov - sum(hist.values())
        out.append(dict(family="d", ref=REF, hist=hist, prm=prm))
    for cov in (64, 65, 2907, 17300, 100000):   # e = 1 or 2: nothing lies below it
        for alpha, n_tests in ((0.01, 1000), (0.3, 1)):
            prm = params(alpha, n_tests, tail=1)
            e = expected(cov, REF, js[0], ERROR_MODELS["sequel"], 0)
            up = edge_up(cov, e, prm, start=e + 1)
            hist = {js[0]: up - 1, js[1]: up, js[2]: e}
            hist[REF] = cov - sum(hist.values())
            out.append(dict(family="d", ref=REF, hist=hist, prm=prm))
    # a == c is p = 1 whatever alpha <= 1 is
    hist = {js[0]: 30, js[1]: 29, js[2]: 31}
    hist[REF] = 1000 - 90
    out.append(dict(family="d", ref=REF, hist=hist, prm=params(0.9, 1, CUSTOM, tail=1)))
    out.append(dict(family="d", ref=REF, hist=dict(hist), prm=params(0.999, 1, CUSTOM, tail=1)))


def family_e(out):
    """Degenerate tables."""
    REF = 21
    j1, j3 = codons_of_class(REF, 1)[0], codons_of_class(REF, 3)[0]
    for tail in (0, 1):
        for alpha, n_tests in ((0.01, 1000), (0.3, 1)):
            prm = params(alpha, n_tests, tail=tail)
            for cov in (1, 2, 7, 64, 1000):
                out.append(dict(family="e", ref=REF, hist={j1: cov}, prm=prm))            # h == cov, reference codon unobserved
            out.append(dict(family="e", ref=REF, hist={j1: 6, j3: 1}, prm=prm))           # two codons, no reference codon
            out.append(dict(family="e", ref=REF, hist={}, extra=9, prm=prm))              # every read skipped
            for err in (CLAMP_HI, CLAMP_EQ):                                              # e == cov
                q = params(alpha, n_tests, err, tail=tail)
                out.append(dict(family="e", ref=REF, hist={j1: 3, j3: 4, REF: 3}, prm=q))
                out.append(dict(family="e", ref=REF, hist={j3: 10}, prm=q))
    for prm in (params(0.01, 1000), params(0.9, 1)):
        out.append(dict(family="e", ref=None, hist={}, extra=9, prm=prm))                 # ... and without a reference
        out.append(dict(family="e", ref=None, hist={}, extra=0, prm=prm))                 # no read at all


def family_f(out):
    """Majority ties (no reference): the lowest tied index is the reference codon, the other tied codons are tested against it."""
    prm = params(0.9, 1)
    for hist in ({0: 20, 63: 20}, {5: 20, 6: 20}, {62: 20, 63: 20}, {63: 7, 62: 7, 1: 3}, {9: 11, 33: 11, 58: 11, 2: 10},
                 {j: 3 for j in range(64)}, {j: 1 for j in range(64)}, {37: 1}, {63: 1}, {40: 2, 3: 1}, {3: 2, 40: 1}, {17: 1, 18: 1}):
        out.append(dict(family="f", ref=None, hist=hist, prm=prm))
    strict = params(0.01, 1000)
    for hist in ({0: 500, 63: 500}, {62: 40, 63: 40, 5: 39}, {j: 30 for j in range(64)}):
        out.append(dict(family="f", ref=None, hist=hist, prm=strict))


def family_g(out):
    """--min-perc / --max-perc are strict: a percentage equal to the bound is not kept (all percentages exact in binary)."""
    REF = 0
    js = codons_of_class(REF, 1) + codons_of_class(REF, 2)
    h64 = {js[0]: 1, js[1]: 2, js[2]: 3, REF: 58}                                                   # 1.5625 3.125 4.6875 %
    h200 = {js[0]: 23, js[1]: 24, js[2]: 25, js[3]: 26, js[4]: 27, REF: 75}                         # 11.5 12 12.5 13 13.5 %
    for lo, hi in ((1.5625, -1.0), (3.125, -1.0), (-1.0, 3.125), (-1.0, 4.6875), (1.5625, 4.6875), (0.0, -1.0), (-1.0, 100.0)):
        out.append(dict(family="g", ref=REF, hist=dict(h64), prm=params(0.9, 1, min_perc=lo, max_perc=hi)))
    for lo, hi in ((12.5, -1.0), (-1.0, 12.5), (11.5, 12.5), (12.5, 13.5), (12.0, 12.5), (11.5, 13.5)):
        out.append(dict(family="g", ref=REF, hist=dict(h200), prm=params(0.9, 1, min_perc=lo, max_perc=hi)))
    out.append(dict(family="g", ref=None, hist={5: 100, 9: 100}, prm=params(0.9, 1, min_perc=50.0)))   # majority tie, 50 % exactly
    out.append(dict(family="g", ref=21, hist={5: 64}, prm=params(0.01, 1, max_perc=100.0)))            # 100 % == max_perc


def family_h(out):
    """DRM masks: only codon 0, only codon 63, everything, nothing."""
    prm = params(0.01, 1000)
    hist = {0: 50, 63: 60, 22: 40, 21: 850}
    for drm in (1, 1 << 63, (1 << 64) - 1, 0, (1 << 63) | 1, 1 << 21, ((1 << 64) - 1) ^ (1 | 1 << 63)):
        out.append(dict(family="h", ref=21, hist=dict(hist), drm=drm, prm=prm))
    out.append(dict(family="h", ref=None, hist={0: 500, 63: 500}, drm=1 << 63, prm=prm))   # majority tie -> ref 0; codon 63 kept
    out.append(dict(family="h", ref=None, hist={0: 500, 63: 500}, drm=1, prm=prm))         # the reference codon's own bit: nothing


# ---------------------------------------------------------------------------------------------------------------- evaluation
def evaluate(spec):
    prm, hist = spec["prm"], {j: h for j, h in spec["hist"].items() if h > 0}
    cov = sum(hist.values())
    ref = spec["ref"]
    if ref is None:
        ref = min((j for j in hist if hist[j] == max(hist.values())), default=None)   # lowest index on ties (SPEC §4)
    codons = {}
    if ref is not None:
        nt = Fraction(prm["n_tests"])
        for j in sorted(hist):
            if j == ref:
                continue
            h = hist[j]
            e = expected(cov, ref, j, err_of(prm), prm["expected_round"])
            S, D = p_exact(h, e, cov, prm["tail"])
            if not decide(S, D, prm["n_tests"], prm["alpha"]):
                codons[j] = [e, NOT_SIGNIFICANT]
                continue
            perc = Fraction(100 * h, cov)
            keep = True
            if prm["min_perc"] >= 0.0 and not perc > Fraction(prm["min_perc"]):
                keep = False
            if prm["max_perc"] >= 0.0 and not perc < Fraction(prm["max_perc"]):
                keep = False
            if spec.get("drm") is not None and not (spec["drm"] >> j) & 1:
                keep = False
            p = mp.mpf(S) / mp.mpf(D)
            padj = min(mp.mpf(1), p * mp.mpf(nt.numerator) / mp.mpf(nt.denominator))
            codons[j] = [e, CALLED if keep else FILTERED, mp.nstr(padj, DIGITS), mp.nstr(mp.log(p), DIGITS)]
    case = dict(family=spec["family"], cov=cov, ref=spec["ref"])
    if spec["ref"] is None:
        case["ref_codon"] = ref   # the majority codon, null where the position has no read
    if spec.get("drm") is not None:
        case["drm"] = spec["drm"]
    if spec.get("extra"):
        case["extra"] = spec["extra"]
    case["hist"] = {str(j): h for j, h in sorted(hist.items())}
    case["codons"] = {str(j): v for j, v in codons.items()}
    return case


def main():
    t0 = time.time()
    specs = []
    for fam in (family_a, family_a_rounding, family_b, family_c, family_d, family_e, family_f, family_g, family_h):
        fam(specs)
    table, cases, dropped = [], [], 0
    for s in specs:
        try:
            case = evaluate(s)
        except Dropped:
            dropped += 1
            continue
        if s["prm"] not in table:
            table.append(s["prm"])
        case["params"] = table.index(s["prm"])
        cases.append(case)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "call_edges.json")
    with open(path, "w") as f:
        f.write('{"generator": "tests/golden/make_call_edges_golden.py", "dps": 60, "margin": 1e-06, "dropped": %d,\n' % dropped)
        f.write('"codon": "[expected, decision (0 not significant, 1 called, 2 significant but filtered), p_adj, log_p]",\n"params": [\n')
        f.write(",\n".join(json.dumps(p) for p in table))
        f.write('\n],\n"cases": [\n')
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    n_cod = sum(len(c["codons"]) for c in cases)
    print("%d cases (%d codons, %d parameter sets), %d dropped, %.1f s" % (len(cases), n_cod, len(table), dropped, time.time() - t0))


if __name__ == "__main__":
    main()
