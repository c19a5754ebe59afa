"""The codon calls of a sample against a control (docs/SPEC.md §21) in plain numpy and exact rational arithmetic (test
infrastructure, like deletion_mirror.py; nothing of the product imports it).

`positions` lays the evaluated positions of §3 out as the library's plan does, `hists` counts the codon histograms of a by-row
symbol matrix, `call_rows` states the rows and control coverages jl_control_call_fetch must return for two sets of histograms,
and `edge_tables` designs small tables either side of alpha / n_tests the way call_edges.py designs them for the error-model call.
Every decision is taken on Fractions; `call_rows` refuses a table whose adjusted p lies within MIN_GAP (relative) of alpha, so
no rounding of the device can flip a decision it states.

Symbols as everywhere: A C G T = 0..3, '-' = 4, N = 5, not covered = 6; codon index = 16 b0 + 4 b1 + b2."""
import functools
import math
from fractions import Fraction

import numpy as np

REF_MAJORITY, REF_SKIP = 0xFF, 0xFE
MIN_GAP = 1e-6


@functools.lru_cache(maxsize=None)
def exact_p(a, n, c, m):
    """P(X >= a), X ~ Hypergeometric(n + m, a + c, n): the table [[a, n - a], [c, m - c]]."""
    M, K = n + m, a + c
    lo, hi = max(0, K - m), min(K, n)
    if a <= lo:
        return Fraction(1)
    if 2 * a > lo + hi:   # the shorter sum
        s = sum(math.comb(K, x) * math.comb(M - K, n - x) for x in range(a, hi + 1))
        return Fraction(s, math.comb(M, n))
    s = sum(math.comb(K, x) * math.comb(M - K, n - x) for x in range(lo, a))
    return 1 - Fraction(s, math.comb(M, n))


def log_of(p):
    """ln of a Fraction in (0, 1] to the last bits of a double."""
    if p >= Fraction(1, 2):
        return math.log1p(-float(1 - p))
    f = float(p)
    if f > 1e-290:
        return math.log(f)
    return math.log(p.numerator) - math.log(p.denominator)


def positions(genes, n_cols, refseq=None, win_begin=0):
    """(pos_gene, pos_codon, pos_col, refcfg, default n_tests) of genes [(begin, end)] (1-based, end exclusive) over a window."""
    pg, pk, pc, cfg = [], [], [], []
    n_tests = 0
    for g, (b, e) in enumerate(genes):
        if b == 0 or e <= b:
            continue
        ncod = (e - b) // 3
        n_tests += ncod
        for k in range(ncod):
            r = b - 1 + 3 * k
            c = r - win_begin
            if c < 0 or c + 2 >= n_cols:
                continue
            v = REF_MAJORITY
            if refseq is not None:
                if r + 2 >= len(refseq) or max(refseq[r:r + 3]) > 3:
                    v = REF_SKIP
                else:
                    v = 16 * int(refseq[r]) + 4 * int(refseq[r + 1]) + int(refseq[r + 2])
            pg.append(g), pk.append(k + 1), pc.append(c), cfg.append(v)
    return pg, pk, pc, cfg, float(n_tests)


def hists(rows, pos_col):
    """int64[P][64]: the reads whose three cells at a position are all bases, by codon."""
    rows = np.asarray(rows)
    out = np.zeros((len(pos_col), 64), dtype=np.int64)
    for p, c in enumerate(pos_col):
        t = rows[:, c:c + 3].astype(np.int64)
        ok = (t < 4).all(axis=1)
        out[p] = np.bincount(16 * t[ok, 0] + 4 * t[ok, 1] + t[ok, 2], minlength=64)
    return out


def call_rows(hs, hc, pos_gene, pos_codon, pos_col, refcfg, alpha, n_tests, min_perc=-1.0, max_perc=-1.0, drm=None, stats=None):
    """([(gene, codon_pos, col, ref_codon, codon, count, coverage, expected, p_adj, log_p)], [control coverage]) in table order.
    `stats` (a dict) counts what happened on the way: skipped positions by cause, tables by kind."""
    stats = {} if stats is None else stats
    bump = lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)   # noqa: E731
    A, T = Fraction(alpha), Fraction(n_tests)
    rows, ccov = [], []
    for p in range(len(pos_col)):
        cov_s, cov_c = int(hs[p].sum()), int(hc[p].sum())
        if cov_s == 0 or cov_c == 0:
            bump("no_sample_coverage" if cov_s == 0 else "no_control_coverage")
            continue
        ref = refcfg[p]
        if ref == REF_SKIP:
            bump("config_codon_not_acgt")
            continue
        if ref == REF_MAJORITY:
            ref = int(np.argmax(hs[p]))   # the first of equal maxima: the lowest index
            if (hs[p] == hs[p][ref]).sum() > 1:
                bump("majority_tied")
        for j in range(64):
            a, c = int(hs[p][j]), int(hc[p][j])
            if j == ref or a == 0:
                continue
            pv = exact_p(a, cov_s, c, cov_c)
            adj = min(Fraction(1), pv * T)
            assert adj == 1 or abs(adj - A) >= Fraction(MIN_GAP) * A, ("a decision too close to alpha to be stated", a, cov_s, c, cov_c)
            called = adj < A
            bump("tables")
            if c == 0:
                bump("control_lacks_codon")
            if c * cov_s > a * cov_c:
                bump("control_carries_more")
                assert not called
            perc = 100.0 * a / cov_s
            if called and ((min_perc >= 0.0 and not perc > min_perc) or (max_perc >= 0.0 and not perc < max_perc)):
                bump("removed_by_perc")
                called = False
            if called and drm is not None and not (int(drm[p]) >> j) & 1:
                bump("removed_by_drm")
                called = False
            if called:
                rows.append((pos_gene[p], pos_codon[p], pos_col[p], ref, j, a, cov_s, c, float(adj), log_of(pv)))
                ccov.append(cov_c)
    return rows, ccov


def edge_tables(alpha, n_tests, shapes=((40, 40), (64, 23), (30, 200), (200, 64), (1000, 100))):
    """For every (cov_s, cov_c) and a few control counts c: (cov_s, cov_c, c, a*) with a* the smallest count that is called,
    where both a* - 1 and a* decide with a relative gap of at least MIN_GAP."""
    A, T = Fraction(alpha), Fraction(n_tests)
    out = []
    for n, m in shapes:
        for c in (0, 1, 2, 5):
            if c > m:
                continue
            a_star = next((a for a in range(1, n + 1) if min(Fraction(1), exact_p(a, n, c, m) * T) < A), None)
            if a_star is None or a_star < 2 or 2 * a_star - 1 > n:
                continue
            gaps = [abs(min(Fraction(1), exact_p(a, n, c, m) * T) - A) / A for a in (a_star - 1, a_star)]
            if min(gaps) >= Fraction(MIN_GAP):
                out.append((n, m, c, a_star))
    return out


def edge_window(tables, ref=0, lo=21, hi=42):
    """The tables of `edge_tables` as histograms, one position each: codon `lo` is seen a* - 1 times (not called), codon `hi` a*
    times (called), the control shows c of each, the config codon `ref` takes the rest.  Returns (hs, hc)."""
    hs = np.zeros((len(tables), 64), dtype=np.int64)
    hc = np.zeros((len(tables), 64), dtype=np.int64)
    for p, (n, m, c, a) in enumerate(tables):
        hs[p][lo], hs[p][hi], hs[p][ref] = a - 1, a, n - (2 * a - 1)
        hc[p][lo], hc[p][hi], hc[p][ref] = c, c, m - 2 * c
        assert hs[p][ref] >= 0 and hc[p][ref] >= 0
    return hs, hc


def rows_of_hists(h, seed=0):
    """uint8[max reads][3 P]: a by-row matrix whose histogram at position p (columns 3p..3p+2) is h[p]; reads a position
    does not need are not covered there (code 6).  Each position's reads are spread over the rows by a seeded permutation."""
    h = np.asarray(h)
    need = h.sum(axis=1)
    n_rows = max(int(need.max()), 1)
    rows = np.full((n_rows, 3 * len(h)), 6, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    for p in range(len(h)):
        codons = np.repeat(np.arange(64), h[p])
        blk = np.stack([(codons >> 4) & 3, (codons >> 2) & 3, codons & 3], axis=1).astype(np.uint8)
        rows[rng.permutation(n_rows)[: len(codons)], 3 * p: 3 * p + 3] = blk
    return rows
