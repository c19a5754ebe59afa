"""The per-read counters and the read rule of docs/SPEC.md §20 restated in plain numpy over a [n_reads][n_cols] code array: five
comparisons and a sum along the columns — deliberately not bit-sliced, nothing of the kernel's shape in it.  The expectations of
tests/test_readstats_host.py and tests/test_gpu_readstats.py."""
import numpy as np

BASES, GAPS, MASKED, COMPARED, MISMATCHES = range(5)
RULES = ("min_bases", "mismatches", "mismatch_perc", "gap_perc", "n_perc")


def stats(rows, compare=None):
    """rows[n_reads, n_cols] codes 0..6; compare[n_cols] codes, 4 and above = not compared, None = no column is.  uint32 [5, n_reads]."""
    rows = np.asarray(rows, dtype=np.uint8)
    cmp_row = np.full(rows.shape[1], 4, dtype=np.uint8) if compare is None else np.asarray(compare, dtype=np.uint8)
    assert cmp_row.shape == (rows.shape[1],)
    base = rows < 4
    compared = base & (cmp_row < 4)[None, :]
    out = [base, rows == 4, rows == 5, compared, compared & (rows != cmp_row[None, :])]
    return np.stack([m.sum(axis=1) for m in out]).astype(np.uint32)


def column_counts(rows):
    """The plain pileup of the rows: [n_cols, 6] reads with A C G T - N."""
    rows = np.asarray(rows, dtype=np.uint8)
    return np.stack([(rows == k).sum(axis=0) for k in range(6)], axis=1).astype(np.uint32)


def consensus(rows):
    """Majority of A C G T - per column, lowest code on ties; 5 where nobody votes (jl_consensus_fetch)."""
    cnt = column_counts(rows)[:, :5]
    out = np.argmax(cnt, axis=1).astype(np.uint8)
    out[cnt.max(axis=1) == 0] = 5
    return out


def read_filter(st, min_bases=0, max_mismatches=0xFFFFFFFF, max_mismatch_perc=-1.0, max_gap_perc=-1.0, max_masked_perc=-1.0):
    """(idx, failed[5]): the kept reads ascending, and the reads failing each of RULES.  The products in float64, left to right."""
    st = np.asarray(st, dtype=np.uint32)
    b, g, m, c, x = (st[k].astype(np.float64) for k in range(5))
    never = np.zeros(st.shape[1], dtype=bool)
    fail = [
        ~(st[BASES] >= min_bases),
        ~(st[MISMATCHES] <= max_mismatches),
        never if max_mismatch_perc < 0 else ~(100.0 * x <= max_mismatch_perc * c),
        never if max_gap_perc < 0 else ~(100.0 * g <= max_gap_perc * (b + g)),
        never if max_masked_perc < 0 else ~(100.0 * m <= max_masked_perc * (b + g + m)),
    ]
    keep = ~np.logical_or.reduce(fail)
    return np.flatnonzero(keep).astype(np.uint32), np.array([f.sum() for f in fail], dtype=np.uint64)
