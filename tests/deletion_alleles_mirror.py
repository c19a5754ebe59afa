"""The rule of docs/SPEC.md §25 in plain numpy over uint8[N][L] rows, as a per-read scan: every read's maximal runs of '-', the
bounded ones grouped by (start, length) with their reads and their flank coverage, the open ones counted per column.  It shares
nothing with the device code — no planes, no bit words, no table — so that what the tests compare the device with is the rule's
own text.  The test of one allele is exact: deletion_mirror's hypergeometric tail in integers and fractions.Fraction, the expected
count by the same IEEE double product and rounding as the library, every decision in exact arithmetic."""
from fractions import Fraction

import numpy as np

import deletion_mirror as dm

GAP, UNCOVERED = 4, 6
ALLELE = np.dtype([("col", "<u4"), ("len", "<u4"), ("count", "<u4"), ("flank", "<u4")])


def read_runs(row):
    """One read: its maximal runs of '-' as (s, len, bounded), ascending by s."""
    n_cols = len(row)
    out, gaps = [], np.flatnonzero(np.asarray(row) == GAP)
    i = 0
    while i < len(gaps):
        k = i
        while k + 1 < len(gaps) and gaps[k + 1] == gaps[k] + 1:
            k += 1
        s, length = int(gaps[i]), k - i + 1
        bounded = s >= 1 and s + length <= n_cols - 1 and row[s - 1] != UNCOVERED and row[s + length] != UNCOVERED
        out.append((s, length, bool(bounded)))
        i = k + 1
    return out


def alleles(rows):
    """rows uint8[N][L] -> dict(runs uint64[2] = (bounded, open), open uint32[L], alleles ALLELE rows ascending by (col, len))."""
    rows = np.asarray(rows)
    n_cols = rows.shape[1]
    runs, open_, table = np.zeros(2, dtype=np.uint64), np.zeros(n_cols, dtype=np.uint32), {}
    for row in rows:
        for s, length, bounded in read_runs(row):
            if bounded:
                runs[0] += 1
                table[(s, length)] = table.get((s, length), 0) + 1
            else:
                runs[1] += 1
                open_[s:s + length] += 1
    out = np.zeros(len(table), dtype=ALLELE)
    covered = rows != UNCOVERED
    for i, (s, length) in enumerate(sorted(table)):
        out[i] = (s, length, table[(s, length)], int((covered[:, s - 1] & covered[:, s + length]).sum()))
    return dict(runs=runs, open=open_, alleles=out)


def column_gaps(rows):
    """col[c]['-'] of §2: the reads whose cell at c is '-'."""
    return (np.asarray(rows) == GAP).sum(axis=0).astype(np.uint32)


def column_covered(rows):
    """The reads covering column c (code != 6)."""
    return (np.asarray(rows) != UNCOVERED).sum(axis=0).astype(np.uint32)


def check_identities(res, gaps, covered, del3):
    """The four consequences of §25: res of alleles() or of the device; gaps[c] = col[c]['-'] and covered[c] of §2, del3[c] of §16
    (None: fewer than three columns)."""
    al, open_ = res["alleles"], res["open"].astype(np.int64)
    n_cols = len(open_)
    assert int(al["count"].astype(np.int64).sum()) == int(res["runs"][0])
    inside, whole = np.zeros(n_cols, dtype=np.int64), np.zeros(n_cols, dtype=np.int64)
    for a in al:
        s, length, count, flank = (int(a[k]) for k in ("col", "len", "count", "flank"))
        assert 1 <= count <= flank <= min(int(covered[s - 1]), int(covered[s + length])), a
        inside[s:s + length] += count
        if length >= 3:
            whole[s:s + length - 2] += count      # the codon starts c with s <= c and c + 3 <= s + length
    assert (np.asarray(gaps).astype(np.int64) == open_ + inside).all()
    if del3 is not None:
        d = np.asarray(del3).astype(np.int64)
        assert (d >= whole[:n_cols - 2]).all()
        quiet = open_[:n_cols - 2] == 0
        assert (d[quiet] == whole[:n_cols - 2][quiet]).all()


def test(count, flank, rate, n_tests, alpha=0.01, round_mode=0, two_sided=False, min_perc=-1.0, max_perc=-1.0):
    """One allele: dict(count, coverage, expected, called, p (Fraction, unadjusted), p_adj (Fraction))."""
    count, cov = int(count), int(flank)
    out = dict(count=count, coverage=cov, expected=0, called=False, p=Fraction(1), p_adj=Fraction(1))
    if cov == 0:
        return out
    e = dm.expected(cov, rate, round_mode)
    p = dm.tail(count, e, cov, two_sided)
    p_adj = min(Fraction(1), p * Fraction(n_tests))
    called = count > 0 and p_adj < Fraction(alpha)
    if min_perc >= 0 and not Fraction(100 * count, cov) > Fraction(min_perc):
        called = False
    if max_perc >= 0 and not Fraction(100 * count, cov) < Fraction(max_perc):
        called = False
    out.update(expected=e, called=called, p=p, p_adj=p_adj)
    return out


test.__test__ = False   # (not a pytest test, whatever its name)


def smallest_called(coverage, rate, n_tests, alpha=0.01, round_mode=0, two_sided=False):
    """The smallest count above the expected one that the exact test calls at this flank coverage."""
    for d in range(dm.expected(coverage, rate, round_mode) + 1, coverage + 1):
        if test(d, coverage, rate, n_tests, alpha, round_mode, two_sided)["called"]:
            return d
    raise AssertionError("no count is called")


def gene_overlaps(begin_abs, length, genes):
    """genes: (name, begin, end) in 1-based reference coordinates, end exclusive, codon k of a gene at begin + 3 (k - 1).  The genes
    the extent [begin_abs, begin_abs + length) overlaps: dict(name, first_position, last_position, codon_aligned) — the first and
    last amino-acid positions touched, clipped to the gene; codon_aligned: the allele removes whole codons of that gene's frame
    (its part inside the gene begins and ends on a codon boundary)."""
    out = []
    for name, b, e in genes:
        lo, hi = max(begin_abs, b), min(begin_abs + length, e)
        if lo >= hi:
            continue
        out.append(dict(name=name, first_position=(lo - b) // 3 + 1, last_position=(hi - 1 - b) // 3 + 1,
                        codon_aligned=(lo - b) % 3 == 0 and (hi - b) % 3 == 0))
    return out
