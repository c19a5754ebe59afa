"""docs/SPEC.md §19 in plain Python: the per-read insertion events of a record build (insertion_mirror.walk's loop, emitting a row
per read and junction instead of counting), the site matrix with insertion sites on the expanded uint8[N][L] rows (§18's rules from
sites_mirror plus §19's table), and the front end's sites, alleles, phasing table and report leaves.  It shares nothing with the
C++ or the device code: no planes, no bit words, no atomics."""
import numpy as np

import insertion_mirror as im
import records_expand
import sites_mirror as sm

INSERTION = 2                                   # jl_site.kind
INS_NONE, INS_OTHER, INS_MAX_ALLELES = 0, 63, 62
GAP, HETERODUPLEX, OUT = 4, 5, 6
EVENT = np.dtype([("read", "<u4"), ("col", "<u4"), ("len", "<u4"), ("kind", "<u4"), ("seq", "<u8")])   # jl_insertion_event


def events(rec, n_cols, win_begin=0, min_qv=0, qmask=None):
    """-> [(read, col, len, kind, seq)] ascending by (read, col): one per read and junction that §17 counts in inframe (kind 1: len
    and seq the allele's key), frameshift (2) or unread (3), len and seq 0 for the last two."""
    m = records_expand.expand_reference(rec, n_cols, win_begin, 0)
    out = []
    for r in range(len(rec["pos"])):
        c, q = int(rec["pos"][r]) - win_begin, 0
        ins = []
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
                    codes = [im._readable(rec, r, i, min_qv, qmask) for i in ins]
                    if length % 3:
                        out.append((r, c, 0, im.FRAMESHIFT, 0))
                    elif length > im.MAX_LEN or None in codes:
                        out.append((r, c, 0, im.UNREAD, 0))
                    else:
                        out.append((r, c, length, im.INFRAME, sum(b << (2 * j) for j, b in enumerate(codes))))
                ins = []
                c += ln
                if op in (7, 8):
                    q += ln
    assert out == sorted(out) and len(set((r, c) for r, c, _, _, _ in out)) == len(out)      # one event a read and junction
    return out


def event_rows(evs):
    out = np.zeros(len(evs), dtype=EVENT)
    for i, e in enumerate(evs):
        out[i] = e
    return out


def aggregate(evs, n_cols):
    """The events counted: (jcnt[:, 1:] of §17, its allele table)."""
    cnt = np.zeros((n_cols, 3), dtype=np.uint32)
    alleles = {}
    for _, c, ln, kind, seq in evs:
        cnt[c, kind - 1] += 1
        if kind == im.INFRAME:
            alleles[(c, ln, seq)] = alleles.get((c, ln, seq), 0) + 1
    return cnt, [(c, l, s, n) for (c, l, s), n in sorted(alleles.items())]


def codes_of(sites, alleles):
    """{(col, len, seq): code} — 1 + the allele's rank among the alleles of its site — with every rule of §19 on the two tables."""
    ins_cols = [col for col, kind, _ in sites if kind == INSERTION]
    keys = [(int(a[0]), int(a[1]), int(a[2])) for a in alleles]
    assert keys == sorted(set(keys)) and len(keys) <= sm.SITES_MAX
    out = {}
    for col in ins_cols:
        mine = [k for k in keys if k[0] == col]
        assert 1 <= len(mine) <= INS_MAX_ALLELES
        for rank, k in enumerate(mine):
            assert k[1] in range(3, 31, 3) and k[2] >> (2 * k[1]) == 0
            out[k] = 1 + rank
    assert len(out) == len(keys)                                    # every allele's column is an insertion site
    return out


def site_matrix(m, evs, sites, alleles):
    """m uint8[N][L] (the expanded matrix, its QV filter applied), the events of the same records, sites [(col, kind, fill)]
    ascending by (col, kind), alleles [(col, len, seq[, count])] ascending -> uint8[N][3 S]."""
    m = np.asarray(m, dtype=np.uint8)
    assert [(s[0], s[1]) for s in sites] == sorted(set((s[0], s[1]) for s in sites))
    code = codes_of(sites, alleles)
    by_col = {}
    for e in evs:
        by_col.setdefault(e[1], []).append(e)
    out = np.empty((m.shape[0], 3 * len(sites)), dtype=np.uint8)
    for k, (col, kind, fill) in enumerate(sites):
        if kind != INSERTION:
            out[:, 3 * k:3 * k + 3] = sm.recode(m, [(col, kind, fill)])
            continue
        assert 1 <= col < m.shape[1] and fill == sm.NO_FILL
        cells = np.empty((m.shape[0], 3), dtype=np.uint8)
        spans = (m[:, col - 1] != OUT) & (m[:, col] != OUT)
        cells[~spans] = OUT
        cells[spans] = sm.bases(INS_NONE)
        for r, _, ln, ekind, seq in by_col.get(col, []):
            assert spans[r]
            if ekind == im.FRAMESHIFT:
                cells[r] = GAP
            elif ekind == im.UNREAD:
                cells[r] = HETERODUPLEX
            else:
                cells[r] = sm.bases(code.get((col, ln, seq), INS_OTHER))
        out[:, 3 * k:3 * k + 3] = cells
    return out


def classes(matrix, sites, alleles):
    """Per insertion site k: dict(none, listed [per code], other, gap, n, out) read counts of the six classes of §19's table."""
    out = {}
    for k, (col, kind, _) in enumerate(sites):
        if kind != INSERTION:
            continue
        cells = matrix[:, 3 * k:3 * k + 3]
        is_codon = (cells < 4).all(axis=1)
        codon = 16 * cells[:, 0].astype(np.int64) + 4 * cells[:, 1] + cells[:, 2]
        n_all = sum(1 for a in alleles if a[0] == col)
        out[k] = dict(none=int((is_codon & (codon == INS_NONE)).sum()),
                      listed=[int((is_codon & (codon == c)).sum()) for c in range(1, n_all + 1)],
                      other=int((is_codon & (codon == INS_OTHER)).sum()),
                      gap=int((cells == GAP).all(axis=1).sum()), n=int((cells == HETERODUPLEX).all(axis=1).sum()),
                      out=int((cells == OUT).all(axis=1).sum()))
        assert out[k]["none"] + sum(out[k]["listed"]) + out[k]["other"] + out[k]["gap"] + out[k]["n"] + out[k]["out"] == len(cells)
    return out


# ---------------------------------------------------------------------------------------------- the front end
def build_sites(variants, deletion_cols, called_alleles, phase_deletions=True):
    """The filtered variant rows, the codon starts of the called deletions (phased or not) and the called insertion alleles
    [(col, len, seq)] of all genes -> (sites [(col, kind, fill)] ascending by (col, kind), alleles ascending and distinct)."""
    sites = sm.build_sites(variants, deletion_cols if phase_deletions else [])
    alleles = sorted(set((int(a[0]), int(a[1]), int(a[2])) for a in called_alleles))
    sites += [(c, INSERTION, sm.NO_FILL) for c in sorted(set(a[0] for a in alleles))]
    return sorted(sites, key=lambda s: (s[0], s[1])), alleles


def build_table(variants, sites, alleles):
    """§18's table, and per insertion site one pseudo-row per allele {col = 3 k, codon = its code, ref_codon = INS_NONE}, ascending
    by code, in the place of its site."""
    variants = np.asarray(variants)
    code = codes_of(sites, alleles)
    rows = []
    for k, (col, kind, _) in enumerate(sites):
        if kind == sm.CODON:
            for v in variants[variants["col"] == col]:
                row = v.copy()
                row["col"] = 3 * k
                rows.append(row)
        else:
            for c in ([sm.DELETED] if kind == sm.DELETION else sorted(code[a] for a in alleles if a[0] == col)):
                row = np.zeros((), dtype=variants.dtype)
                row["col"], row["codon"], row["ref_codon"] = 3 * k, c, sm.PRESENT if kind == sm.DELETION else INS_NONE
                rows.append(row)
    out = np.zeros(len(rows), dtype=variants.dtype)
    for i, row in enumerate(rows):
        out[i] = row
    return out


def report(phase, sites, alleles):
    """The new leaves of the front end from a phasing result on the site matrix: per haplotype `insertions` (a flag per allele, by
    site then code), and per allele its haplotype_hit."""
    code = codes_of(sites, alleles)
    site_of = {col: k for k, (col, kind, _) in enumerate(sites) if kind == INSERTION}
    haps = [[bool(pat[site_of[a[0]]] == code[a]) for a in alleles] for pat in phase["hap_pattern"]]
    return dict(insertions=haps, hit={a: [bool(pat[site_of[a[0]]] == code[a]) for pat in phase["hap_pattern"]] for a in alleles})
