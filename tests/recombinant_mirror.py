"""The rule of docs/SPEC.md §23 in plain loops over uint8[N][L] rows: which reads are one haplotype of `pattern` from the first
variant position up to a breakpoint and another from there to the last, and the haplotype-level rule over the pattern rows
themselves.  It shares nothing with the device code — no planes, no bit slices, no reversed copies — so that what the tests compare
the device with is the rule's own text."""
import numpy as np

UNINFORMATIVE, NONE, AMBIGUOUS, WHOLE = 0xFFFB, 0xFFFC, 0xFFFD, 0xFFFA


def agreement(row, pos_cols, pattern):
    """One read: (k = its informative positions, agree bool[H][Vp] = the position is open for the read or its codon equals the
    row's).  Only the comparison of the read's codons with all pattern rows is a numpy expression, as in rescue_mirror.py."""
    vp = len(pos_cols)
    is_open = np.ones(vp, dtype=bool)
    codons = np.zeros(vp, dtype=np.int64)
    for p, c in enumerate(pos_cols):
        s0, s1, s2 = int(row[c]), int(row[c + 1]), int(row[c + 2])
        if s0 < 4 and s1 < 4 and s2 < 4:
            is_open[p] = False
            codons[p] = 16 * s0 + 4 * s1 + s2
    return int((~is_open).sum()), (pattern == codons[None, :]) | is_open[None, :]


def pre_suf(agree):
    """Per row of agree[H][Vp]: pre = the smallest p with !agree (Vp when none); suf = Vp - 1 - the largest p with !agree (Vp when
    none) = the smallest p with !agree counted from the last position."""
    vp = agree.shape[1]
    bad = ~agree
    some = bad.any(axis=1)
    return np.where(some, bad.argmax(axis=1), vp), np.where(some, bad[:, ::-1].argmax(axis=1), vp)


def recombinants(rows, pos_cols, pattern, min_positions=1):
    """rows uint8[N][L] (codes of SPEC §1), pos_cols[Vp] codon starts, pattern[H][Vp] codon indices.  Returns dict(left, right,
    prefix, suffix uint16[N]; parent_reads uint32[H][2]; tally uint64[5] = recombinant, ambiguous_parent, whole, none,
    uninformative)."""
    rows = np.asarray(rows)
    pattern = np.asarray(pattern, dtype=np.int64).reshape(len(pattern), len(pos_cols))
    n_hap, vp = pattern.shape
    out = {key: np.zeros(len(rows), dtype=np.uint16) for key in ("left", "right", "prefix", "suffix")}
    parent_reads = np.zeros((n_hap, 2), dtype=np.uint32)
    tally = np.zeros(5, dtype=np.uint64)
    for i, row in enumerate(rows):
        k, agree = agreement(row, pos_cols, pattern)
        pre, suf = pre_suf(agree)
        big_p, big_s = int(pre.max()), int(suf.max())
        at_p, at_s = np.flatnonzero(pre == big_p), np.flatnonzero(suf == big_s)
        out["prefix"][i], out["suffix"][i] = big_p, big_s
        if k < min_positions:
            left = right = UNINFORMATIVE
            tally[4] += 1
        elif big_p == vp:
            left = right = WHOLE
            tally[2] += 1
        elif big_p + big_s < vp:
            left = right = NONE
            tally[3] += 1
        else:
            left = at_p[0] if len(at_p) == 1 else AMBIGUOUS
            right = at_s[0] if len(at_s) == 1 else AMBIGUOUS
            if left != AMBIGUOUS and right != AMBIGUOUS:
                parent_reads[left, 0] += 1
                parent_reads[right, 1] += 1
                tally[0] += 1
            else:
                tally[1] += 1
        out["left"][i], out["right"][i] = left, right
    out["parent_reads"], out["tally"] = parent_reads, tally
    return out


def haplotype_recombinants(pattern, hap_count, min_parent_ratio=2.0):
    """The haplotype level: for row h the candidate parents are the a != h with hap_count[a] >= min_parent_ratio * hap_count[h] (in
    double); pre / suf = the common prefix / suffix length of the two rows; flagged iff candidates exist and max pre + max suf >=
    Vp; left / right = the lowest index attaining each maximum.  A list of dict(flagged, left, right, prefix, suffix), all 0 / False
    without a candidate."""
    pattern = [[int(x) for x in row] for row in pattern]
    vp = len(pattern[0])
    out = []
    for h, row in enumerate(pattern):
        best = dict(flagged=False, left=0, right=0, prefix=0, suffix=0)
        seen = False
        for a, other in enumerate(pattern):
            if a == h or not float(hap_count[a]) >= float(min_parent_ratio) * float(hap_count[h]):
                continue
            pre = 0
            while pre < vp and row[pre] == other[pre]:
                pre += 1
            suf = 0
            while suf < vp and row[vp - 1 - suf] == other[vp - 1 - suf]:
                suf += 1
            if not seen or pre > best["prefix"]:
                best["prefix"], best["left"] = pre, a
            if not seen or suf > best["suffix"]:
                best["suffix"], best["right"] = suf, a
            seen = True
        best["flagged"] = seen and best["prefix"] + best["suffix"] >= vp
        out.append(best)
    return out
