"""The rule of docs/SPEC.md §22 in plain loops over uint8[N][L] rows: which haplotype of `pattern` a read is nearest to at the
variant positions where it can be read, within a budget of differing codon positions.  It shares nothing with the device code —
no planes, no bit slices, no saturation — so that what the tests compare the device with is the rule's own text.  (Only the
comparison of one read's codons with all pattern rows is a numpy expression, as in rescue_mirror.py.)"""
import numpy as np

UNINFORMATIVE, NONE, AMBIGUOUS = 0xFFFB, 0xFFFC, 0xFFFD
MAX_DISTANCE = 7


def distances(row, pos_cols, pattern):
    """One read: (k = its informative positions, d[H] = the informative positions at which its codon differs from each row)."""
    informative, codons = [], []
    for p, c in enumerate(pos_cols):
        s0, s1, s2 = int(row[c]), int(row[c + 1]), int(row[c + 2])
        if s0 < 4 and s1 < 4 and s2 < 4:
            informative.append(p)
            codons.append(16 * s0 + 4 * s1 + s2)
    differs = pattern[:, informative] != np.array(codons, dtype=np.int64)[None, :]      # [H][k]
    return len(informative), differs.sum(axis=1)


def nearest(rows, pos_cols, pattern, min_positions=1, max_distance=1):
    """rows uint8[N][L] (codes of SPEC §1), pos_cols[Vp] codon starts, pattern[H][Vp] codon indices, max_distance = D.
    Returns (nearest uint16[N], dist uint8[N], hap_reads uint32[H][D + 1], tally uint64[4] = assigned, ambiguous, none,
    uninformative)."""
    assert 0 <= max_distance <= MAX_DISTANCE
    rows = np.asarray(rows)
    pattern = np.asarray(pattern, dtype=np.int64).reshape(len(pattern), len(pos_cols))
    n_hap = len(pattern)
    out = np.zeros(len(rows), dtype=np.uint16)
    dist = np.zeros(len(rows), dtype=np.uint8)
    hap_reads = np.zeros((n_hap, max_distance + 1), dtype=np.uint32)
    tally = np.zeros(4, dtype=np.uint64)
    for i, row in enumerate(rows):
        k, d = distances(row, pos_cols, pattern)
        dmin = int(d.min())
        at_min = [h for h in range(n_hap) if d[h] == dmin]
        if k < min_positions:
            out[i], dist[i] = UNINFORMATIVE, 0xFF
            tally[3] += 1
        elif dmin > max_distance:
            out[i], dist[i] = NONE, max_distance + 1
            tally[2] += 1
        elif len(at_min) == 1:
            out[i], dist[i] = at_min[0], dmin
            hap_reads[at_min[0], dmin] += 1
            tally[0] += 1
        else:
            out[i], dist[i] = AMBIGUOUS, dmin
            tally[1] += 1
    return out, dist, hap_reads, tally


def true_distance(rows, pos_cols, pattern):
    """dmin of every read whatever the budget (int64[N]; -1 where the read is informative nowhere): what the tests use to show
    that their cases hold distances a four-bit counter would wrap."""
    pattern = np.asarray(pattern, dtype=np.int64).reshape(len(pattern), len(pos_cols))
    out = np.full(len(rows), -1, dtype=np.int64)
    for i, row in enumerate(np.asarray(rows)):
        k, d = distances(row, pos_cols, pattern)
        if k:
            out[i] = int(d.min())
    return out
