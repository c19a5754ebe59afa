"""The rule of docs/SPEC.md §14 in plain loops over uint8[N][L] rows: which haplotype of `pattern` a read agrees with at the
variant positions where it can be read.  It shares nothing with the device code — no planes, no bit tricks — so that what the
tests compare the device with is the rule's own text.  (Only the comparison of one read's codons with all pattern rows is a
numpy expression: 702 haplotypes x 130 positions a read would take minutes otherwise.)"""
import numpy as np

UNINFORMATIVE, NONE, AMBIGUOUS = 0xFFFB, 0xFFFC, 0xFFFD


def rescue(rows, pos_cols, pattern, min_positions=1):
    """rows uint8[N][L] (codes of SPEC §1), pos_cols[Vp] codon starts, pattern[H][Vp] codon indices.
    Returns (rescue uint16[N], hap_reads uint32[H], tally uint64[4] = assigned, ambiguous, none, uninformative)."""
    rows = np.asarray(rows)
    pattern = np.asarray(pattern, dtype=np.int64).reshape(len(pattern), len(pos_cols))
    n_hap = len(pattern)
    out = np.zeros(len(rows), dtype=np.uint16)
    hap_reads = np.zeros(n_hap, dtype=np.uint32)
    tally = np.zeros(4, dtype=np.uint64)
    for i, row in enumerate(rows):
        informative, codons = [], []           # the positions where the read can be read, and its codons there
        for p, c in enumerate(pos_cols):
            s0, s1, s2 = int(row[c]), int(row[c + 1]), int(row[c + 2])
            if s0 < 4 and s1 < 4 and s2 < 4:
                informative.append(p)
                codons.append(16 * s0 + 4 * s1 + s2)
        agrees = (pattern[:, informative] == np.array(codons, dtype=np.int64)[None, :]).all(axis=1)   # [H]; all True without any
        agreeing = [h for h in range(n_hap) if agrees[h]]
        if len(informative) < min_positions:
            out[i] = UNINFORMATIVE
            tally[3] += 1
        elif len(agreeing) == 0:
            out[i] = NONE
            tally[2] += 1
        elif len(agreeing) == 1:
            out[i] = agreeing[0]
            hap_reads[agreeing[0]] += 1
            tally[0] += 1
        else:
            out[i] = AMBIGUOUS
            tally[1] += 1
    return out, hap_reads, tally
