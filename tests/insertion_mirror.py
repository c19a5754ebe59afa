"""The rule of docs/SPEC.md §17 as plain Python loops over record arrays, op by op and base by base, like
records_expand.expand_reference — whose matrix defines which reads span a junction.  It shares nothing with the device code: no
bit planes, no table, no waves.  Per junction c (between window columns c - 1 and c) the reads spanning it and, of those with an
insertion there, the in-frame readable ones, the frame-shifting ones and the unreadable ones; and the distinct (col, len, seq)
among the first kind with their read counts.  The test of one allele is exact (deletion_mirror's hypergeometric tail in Python
integers), the expected count by the same IEEE double product and rounding as the library.

`records()` builds the arrays the library takes from reads written out by hand: test infrastructure for the two test files."""
from collections import Counter
from fractions import Fraction

import numpy as np

import deletion_mirror as dm
import records_expand

SPAN, INFRAME, FRAMESHIFT, UNREAD = 0, 1, 2, 3
MAX_LEN = 30
OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
_NIB = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "R": 5, "=": 0}      # BAM's 4-bit codes (R = A or G: an ambiguity code)
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}


def records(reads, with_qual=False):
    """reads: (pos, [(op letter, len), ...], bases[, quals]) each -> dict(pos, cigar, cig_off, seq4, seq_off[, qual, qual_off]).
    bases: a string over A C G T N R =, one per query base the cigar consumes (I S = X); quals: a list as long (default 40)."""
    pos, cigar, cig_off, seq4, seq_off, qual, qual_off = [], [], [0], [], [0], [], [0]
    for rd in reads:
        p, ops, bases = rd[0], rd[1], rd[2]
        assert sum(ln for op, ln in ops if op in "IS=XM") == len(bases), rd
        pos.append(p)
        cigar += [(ln << 4) | OPS[op] for op, ln in ops]
        cig_off.append(len(cigar))
        nib = [_NIB[b] for b in bases] + [0]
        seq4 += [(nib[i] << 4) | nib[i + 1] for i in range(0, len(bases), 2)]
        seq_off.append(len(seq4))
        q = list(rd[3]) if len(rd) > 3 and rd[3] is not None else [40] * len(bases)
        assert len(q) == len(bases)
        qual += q
        qual_off.append(len(qual))
    rec = dict(pos=np.array(pos, dtype=np.int32), cigar=np.array(cigar, dtype=np.uint32), cig_off=np.array(cig_off, dtype=np.uint64),
               seq4=np.array(seq4, dtype=np.uint8), seq_off=np.array(seq_off, dtype=np.uint64))
    if with_qual:
        rec.update(qual=np.array(qual, dtype=np.uint8), qual_off=np.array(qual_off, dtype=np.uint64))
    return rec


def _readable(rec, r, q, min_qv, qmask):
    """Base q of read r -> its code 0..3, or None when it is not exactly A C G T or the filter in force takes it."""
    byte = int(rec["seq4"][int(rec["seq_off"][r]) + (q >> 1)])
    code = _CODE.get(byte & 15 if q & 1 else byte >> 4)
    if code is None or not min_qv:
        return code
    if qmask is not None:                                   # a bit per base, laid out by the bases' bytes (include/juliet_hip.h)
        i = 2 * (int(rec["seq_off"][r]) - int(rec["seq_off"][0])) + q
        return None if (int(qmask[i >> 3]) >> (i & 7)) & 1 else code
    if rec.get("qual") is not None:
        qv = int(rec["qual"][int(rec["qual_off"][r]) + q])
        return None if qv != 0xFF and qv < min(min_qv, 127) else code
    return code


def walk(rec, n_cols, win_begin=0, min_qv=0, qmask=None):
    """-> (jcnt uint32[n_cols][4], [(col, len, seq, count), ...] ascending).  The filter: `qmask` (with min_qv != 0) or rec's qualities."""
    m = records_expand.expand_reference(rec, n_cols, win_begin, 0)       # (covered or not does not depend on the filter)
    jcnt = np.zeros((n_cols, 4), dtype=np.uint32)
    for c in range(1, n_cols):
        jcnt[c, SPAN] = int(((m[:, c - 1] != 6) & (m[:, c] != 6)).sum())
    alleles = Counter()
    for r in range(len(rec["pos"])):
        c, q = int(rec["pos"][r]) - win_begin, 0
        ins = []                                                         # query offsets of the inserted bases gathered so far
        for w in rec["cigar"][int(rec["cig_off"][r]):int(rec["cig_off"][r + 1])]:
            op, ln = int(w) & 15, int(w) >> 4
            if op == 0:
                raise ValueError("cigar M")
            if ln == 0:
                continue
            if op == 1:
                ins += range(q, q + ln)
                q += ln
            elif op == 4:
                q += ln
            elif op in (2, 3, 7, 8):
                if ins and 1 <= c < n_cols and m[r, c - 1] != 6 and m[r, c] != 6:
                    length = len(ins)
                    codes = [_readable(rec, r, i, min_qv, qmask) for i in ins]
                    if length % 3:
                        jcnt[c, FRAMESHIFT] += 1
                    elif length > MAX_LEN or None in codes:
                        jcnt[c, UNREAD] += 1
                    else:
                        jcnt[c, INFRAME] += 1
                        alleles[(c, length, sum(b << (2 * j) for j, b in enumerate(codes)))] += 1
                ins = []
                c += ln
                if op in (7, 8):
                    q += ln
    return jcnt, [(c, l, s, n) for (c, l, s), n in sorted(alleles.items())]


def test(count, jcnt, rate, n_tests, alpha=0.01, round_mode=0, two_sided=False, min_perc=-1.0, max_perc=-1.0):
    """One allele: dict(count, coverage, expected, frameshift, unread, called, p (Fraction, unadjusted), p_adj (Fraction))."""
    span, fs, un = int(jcnt[SPAN]), int(jcnt[FRAMESHIFT]), int(jcnt[UNREAD])
    cov = span - fs - un
    assert 0 <= count <= cov
    out = dict(count=count, coverage=cov, expected=0, frameshift=fs, unread=un, called=False, p=Fraction(1), p_adj=Fraction(1))
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
    """The smallest count above the expected one that the exact test calls at a junction of `coverage` reads, none out of frame."""
    for d in range(dm.expected(coverage, rate, round_mode) + 1, coverage + 1):
        if test(d, (coverage, d, 0, 0), rate, n_tests, alpha, round_mode, two_sided)["called"]:
            return d
    raise AssertionError("no count is called")


def seq_of(word, length):
    """The inserted bases of a table row as letters."""
    return "".join("ACGT"[(int(word) >> (2 * j)) & 3] for j in range(length))
