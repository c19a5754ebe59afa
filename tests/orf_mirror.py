"""The per-read reading-frame counters, their flags and the keep rule of docs/SPEC.md §27 restated without a device, by row: for every
span and every read a plain loop over the span's codons of the [n_reads][n_cols] code array, written from the SPEC's sentences —
nothing of the kernel's masks, planes or shape in it.  The expectations of tests/test_orf_host.py, tests/test_gpu_orf.py and
tests/test_gpu_orf_cli.py."""
import numpy as np

COVERED, GAP_CELLS, CODONS_READ, STOPS = range(4)
NO_STOP = 0xFFFFFFFF
PARTIAL, STOP, FRAMESHIFT, DELETION = 1, 2, 4, 8
A, C, G, T = range(4)
GAP, N, UNCOVERED = 4, 5, 6
STOP_CODONS = {(T, A, A), (T, A, G), (T, G, A)}


def counters(rows, spans, ref):
    """rows[n_reads, n_cols] codes 0..6; spans: (col, n_codons) pairs; ref[n_cols] codes.
    (counts uint32 [4, n_spans, n_reads], first_stop uint32 [n_spans, n_reads])."""
    rows = np.asarray(rows, dtype=np.uint8)
    ref = [int(x) for x in np.asarray(ref, dtype=np.uint8)]
    n_reads, n_cols = rows.shape
    assert len(ref) == n_cols and 1 <= len(spans) <= 64
    counts = np.zeros((4, len(spans), n_reads), dtype=np.uint32)
    first = np.full((len(spans), n_reads), NO_STOP, dtype=np.uint32)
    for g, (col, n_codons) in enumerate(spans):
        col, n_codons = int(col), int(n_codons)
        assert n_codons >= 1 and col + 3 * n_codons <= n_cols
        ref_is_stop = [tuple(ref[col + 3 * k:col + 3 * k + 3]) in STOP_CODONS for k in range(n_codons)]   # (a code >= 4: in no such triple)
        for i in range(n_reads):
            cells = rows[i, col:col + 3 * n_codons].tolist()
            counts[COVERED, g, i] = sum(1 for x in cells if x != UNCOVERED)
            counts[GAP_CELLS, g, i] = sum(1 for x in cells if x == GAP)
            for k in range(n_codons):
                codon = tuple(cells[3 * k:3 * k + 3])
                if max(codon) >= 4:
                    continue
                counts[CODONS_READ, g, i] += 1
                if codon in STOP_CODONS and not ref_is_stop[k]:
                    counts[STOPS, g, i] += 1
                    if first[g, i] == NO_STOP:
                        first[g, i] = k
    return counts, first


def classify(counts, first, spans, max_gap_cells=0, tail_codons=0):
    """flags uint8 [n_spans, n_reads]."""
    flags = np.zeros(first.shape, dtype=np.uint8)
    for g, (_, n) in enumerate(spans):
        n = int(n)
        body = n - min(int(tail_codons), n)
        for i in range(first.shape[1]):
            f = 0
            if counts[COVERED, g, i] < 3 * n:
                f |= PARTIAL
            if first[g, i] != NO_STOP and first[g, i] < body:
                f |= STOP
            if counts[GAP_CELLS, g, i] % 3 != 0:
                f |= FRAMESHIFT
            if max_gap_cells > 0 and counts[GAP_CELLS, g, i] >= max_gap_cells:
                f |= DELETION
            flags[g, i] = f
    return flags


def keep(flags, mask=STOP | FRAMESHIFT):
    """(idx, n_flagged): the reads none of whose spans' flags meets the mask, ascending."""
    assert mask and not mask & ~(STOP | FRAMESHIFT | DELETION)
    bad = np.array([any(int(flags[g, i]) & mask for g in range(flags.shape[0])) for i in range(flags.shape[1])], dtype=bool)
    return np.flatnonzero(~bad).astype(np.uint32), int(bad.sum())


def letters(f):
    """The report's flags column: the letters P S F D, or -."""
    return "".join(ch for bit, ch in ((PARTIAL, "P"), (STOP, "S"), (FRAMESHIFT, "F"), (DELETION, "D")) if f & bit) or "-"
