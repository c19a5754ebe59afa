"""docs/SPEC.md §18 in plain numpy over uint8[N][L] rows: the site matrix (jl_sites_assemble), and the construction of the sites and
of the phasing table from a variant table and the called deletions.  It shares nothing with the C++ or the device code — no planes,
no bit words — so that what the tests compare either with is the rule's own text."""
import numpy as np

CODON, DELETION = 0, 1                       # jl_site.kind
NO_FILL, PRESENT, DELETED = 0xFF, 0, 1       # jl_site.fill; the two letters of a deletion site (codons AAA, AAC)
SITES_MAX = 4096
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
VARIANT = np.dtype([("gene", "<u4"), ("codon_pos", "<u4"), ("col", "<u4"), ("ref_codon", "u1"), ("codon", "u1"), ("flags", "<u2"),
                    ("count", "<u4"), ("coverage", "<u4"), ("expected", "<u4"), ("pad_", "<u4"), ("p_value", "<f8"), ("log_p", "<f8")])   # jl_variant


def bases(codon):
    """The three base codes of a codon index 16 s0 + 4 s1 + s2 (SPEC §1)."""
    return (codon >> 4) & 3, (codon >> 2) & 3, codon & 3


def classes(rows, col):
    """(codon, del3) of SPEC §16 at codon start `col`: boolean per read."""
    three = np.asarray(rows)[:, col:col + 3]
    return (three < 4).all(axis=1), (three == 4).all(axis=1)


def recode(rows, sites):
    """rows uint8[N][L], sites [(col, kind, fill)] -> uint8[N][3 S]: site k at columns 3k..3k+2."""
    rows = np.asarray(rows, dtype=np.uint8)
    out = np.empty((rows.shape[0], 3 * len(sites)), dtype=np.uint8)
    for k, (col, kind, fill) in enumerate(sites):
        assert col + 2 < rows.shape[1] and kind in (CODON, DELETION)
        cells = rows[:, col:col + 3].copy()
        codon, del3 = classes(rows, col)
        if kind == DELETION:
            assert fill == NO_FILL
            cells[codon] = bases(PRESENT)
            cells[del3] = bases(DELETED)
        elif fill != NO_FILL:
            assert 0 <= fill <= 63
            cells[del3] = bases(fill)
        out[:, 3 * k:3 * k + 3] = cells
    return out


def build_sites(variants, deletion_cols):
    """The filtered variant rows (fields col, ref_codon) and the codon-start columns of the called deletions of all genes ->
    [(col, kind, fill)] ascending by (col, kind): a variant position is a CODON site, filled with its ref_codon iff a deletion is
    called there too; every called deletion is a DELETION site."""
    dels = sorted(set(int(c) for c in deletion_cols))
    ref = {}
    for v in variants:
        ref.setdefault(int(v["col"]), int(v["ref_codon"]))
    sites = [(c, CODON, r if c in dels else NO_FILL) for c, r in ref.items()] + [(c, DELETION, NO_FILL) for c in dels]
    return sorted(sites, key=lambda s: (s[0], s[1]))


def build_table(variants, sites):
    """The phasing table on the site matrix: the codon rows with col = 3 k of their CODON site, and per DELETION site one pseudo-row
    {col = 3 k, codon = DELETED, ref_codon = PRESENT}, ascending by column (the codon rows of one site keep their order)."""
    variants = np.asarray(variants)
    out = np.zeros(len(variants) + sum(1 for s in sites if s[1] == DELETION), dtype=variants.dtype)
    n = 0
    for k, (col, kind, _) in enumerate(sites):
        if kind == CODON:
            for v in variants[variants["col"] == col]:
                out[n] = v
                out[n]["col"] = 3 * k
                n += 1
        else:
            out[n]["col"], out[n]["codon"], out[n]["ref_codon"] = 3 * k, DELETED, PRESENT
            n += 1
    assert n == len(out)
    return out


def report(phase, sites, table, win_begin=0):
    """What the front end prints of a phasing result on the site matrix (phase: oracle_lib.Oracle.phase's dict or
    capi.Juliet.phase_fetch's): the codon sites' absolute positions, per haplotype the codons ("---" where the companion deletion
    site at the same column is DELETED) and the deletions, and the hit rows of the codon rows and of the deletion sites."""
    assert [int(c) for c in phase["pos_cols"]] == [3 * k for k in range(len(sites))]
    codon_k = [k for k, s in enumerate(sites) if s[1] == CODON]
    del_k = [k for k, s in enumerate(sites) if s[1] == DELETION]
    companion = {k: next((d for d in del_k if sites[d][0] == sites[k][0]), None) for k in codon_k}
    haps = []
    for pat in phase["hap_pattern"]:
        codons = ["---" if companion[k] is not None and pat[companion[k]] == DELETED else CODONS[pat[k]] for k in codon_k]
        haps.append(dict(codons=codons, deletions=[bool(pat[d] == DELETED) for d in del_k]))
    h = len(phase["hap_pattern"])
    hit = np.asarray(phase["hit"])[:len(table), :h].astype(bool)
    is_del = np.array([sites[int(c) // 3][1] == DELETION for c in table["col"]], dtype=bool)
    return dict(variant_positions_abs=[win_begin + sites[k][0] + 1 for k in codon_k],
                deletion_positions_abs=[win_begin + sites[k][0] + 1 for k in del_k],
                haplotypes=haps, codon_hit=hit[~is_del].tolist(),
                deletion_hit={sites[k][0]: [bool(p[k] == DELETED) for p in phase["hap_pattern"]] for k in del_k})


# ---------------------------------------------------------------------------------------------- two designed, noise-free samples
def variant_rows(entries):
    """[(col, ref_codon, codon)] -> rows of a variant table, ascending."""
    out = np.zeros(len(entries), dtype=VARIANT)
    for k, (col, ref, codon) in enumerate(sorted(entries)):
        out[k]["col"], out[k]["ref_codon"], out[k]["codon"], out[k]["codon_pos"] = col, ref, codon, col // 3 + 1
    return out


def cod(cells):
    return 16 * int(cells[0]) + 4 * int(cells[1]) + int(cells[2])


def other_codon(ref, k):
    return (ref + 21 * k + 5) % 64 if (ref + 21 * k + 5) % 64 != ref else (ref + 1) % 64


def scenario_a():
    """30 columns.  100 wild-type reads, 40 with a codon variant at column 6, 30 with codon 6 (column 15) deleted and nothing else,
    20 with that deletion and a second codon variant at column 21.  No noise."""
    rng = np.random.default_rng(41)
    ref = rng.integers(0, 4, size=30, dtype=np.uint8)
    v1, v2 = other_codon(cod(ref[6:9]), 1), other_codon(cod(ref[21:24]), 2)
    rows = np.repeat(ref[None, :], 190, axis=0)
    rows[100:140, 6:9] = bases(v1)
    rows[140:190, 15:18] = 4
    rows[170:190, 21:24] = bases(v2)
    rows = rows[np.random.default_rng(5).permutation(190)]
    return rows, ref, variant_rows([(6, cod(ref[6:9]), v1), (21, cod(ref[21:24]), v2)]), [15], (v1, v2)


def scenario_b():
    """30 columns.  100 wild-type reads, 40 with a codon variant at column 9, 25 with the codon at column 9 deleted."""
    rng = np.random.default_rng(43)
    ref = rng.integers(0, 4, size=30, dtype=np.uint8)
    v = other_codon(cod(ref[9:12]), 3)
    rows = np.repeat(ref[None, :], 165, axis=0)
    rows[100:140, 9:12] = bases(v)
    rows[140:165, 9:12] = 4
    rows = rows[np.random.default_rng(6).permutation(165)]
    return rows, ref, variant_rows([(9, cod(ref[9:12]), v)]), [9], (v,)
