"""Restatement of docs/SPEC.md §24 for the tests: the counting rule of jl_class_codons_async in numpy, sharing no code with the
library."""
import numpy as np

def class_codons(rows, labels, n_classes, cols):
    """rows uint8[n][l] codes 0..6, labels uint16[n], cols codon starts -> (hist uint32[K][P][64], class_reads uint32[K]).
    A read of class k whose three codes at col .. col + 2 are all < 4 adds one to hist[k][p][16 a + 4 b + c]; labels at or above
    n_classes belong to no class."""
    rows = np.asarray(rows, dtype=np.uint8)
    labels = np.asarray(labels)
    cols = [int(c) for c in cols]
    hist = np.zeros((n_classes, len(cols), 64), dtype=np.uint32)
    reads = np.array([(labels == k).sum() for k in range(n_classes)], dtype=np.uint32)
    inside = labels < n_classes
    for p, c in enumerate(cols):
        trip = rows[:, c:c + 3].astype(np.int64)
        ok = inside & (trip < 4).all(axis=1)
        codon = trip[ok, 0] * 16 + trip[ok, 1] * 4 + trip[ok, 2]
        np.add.at(hist[:, p, :], (labels[ok].astype(np.int64), codon), 1)
    return hist, reads



# ---------------------------------------------------------------------------------------------- the front-end rule of §24
CODON_AA = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVVXYXYSSSSXCWCLFLF"   # index = 16 * first + 4 * second + third over A C G T; stop = X


def codon_string(idx):
    return "ACGT"[idx >> 4] + "ACGT"[(idx >> 2) & 3] + "ACGT"[idx & 3]


def drm_matches(entry, position, amino_acid):
    """One entry of a DRM's positions — "103", "M103", "M103L", "103LKA", "103*": an optional reference letter, the 1-based codon
    position, the mutant amino acids; none, or a '*' among them, is a wildcard."""
    body = entry[1:] if entry[:1].isalpha() else entry
    digits = ""
    while body and body[0].isdigit():
        digits, body = digits + body[0], body[1:]
    muts = body.upper()
    return int(digits) == position and (muts == "" or "*" in muts or amino_acid in muts)


def drms_of(gene_drms, position, amino_acid):
    """Names of the gene's DRMs (dict(name, positions=[...]), in the config's order) with an entry that matches."""
    return [d["name"] for d in gene_drms if any(drm_matches(s, position, amino_acid) for s in d["positions"])]


def front_end(hist, cols, positions, hap_reads, hap_frequency, variant_rows=()):
    """hist[H][P][64] at the ascending distinct columns `cols` (H = 0: no reported haplotype).  positions: the evaluated
    positions of every gene, dict(gene_index, gene, position, col, ref (codon index, or None: no reference codon there), drms
    (the gene's DRM list)).  hap_reads / hap_frequency: the haplotypes' `reads` and `frequency` leaves.  variant_rows:
    dict(col, codon) per variant_codons[] entry.  Returns dict(mutations[H], drugs[H], drug_profile, haplotype_count[rows],
    haplotype_coverage[rows])."""
    hist = np.asarray(hist)
    n_hap = hist.shape[0] if hist.ndim == 3 else 0
    at = {int(c): i for i, c in enumerate(cols)}
    mutations, drugs = [], []
    for h in range(n_hap):
        mine = []
        for q in sorted(positions, key=lambda q: (q["gene_index"], q["position"])):
            if q["ref"] is None:
                continue
            row = hist[h, at[q["col"]]]
            cov = int(row.sum())
            if cov == 0:
                continue
            best = int(np.argmax(row))             # the first maximum: the lowest index on ties
            if best == q["ref"]:
                continue
            aa = CODON_AA[best]
            mine.append(dict(gene=q["gene"], position=q["position"], ref_codon=codon_string(q["ref"]), ref_amino_acid=CODON_AA[q["ref"]],
                             codon=codon_string(best), amino_acid=aa, count=int(row[best]), coverage=cov, frequency=int(row[best]) / cov,
                             drms=drms_of(q["drms"], q["position"], aa)))
        mutations.append(mine)
        drugs.append(sorted({d for m in mine for d in m["drms"]}))
    profile = []
    for drug in sorted({d for ds in drugs for d in ds}):
        has = [drug in ds for ds in drugs]
        freq = 0.0
        for f, x in zip(hap_frequency, has):
            if x:
                freq += f
        profile.append(dict(drug=drug, haplotypes=has, reads=sum(r for r, x in zip(hap_reads, has) if x), frequency=freq))
    count = [[int(hist[h, at[v["col"]], v["codon"]]) for h in range(n_hap)] for v in variant_rows]
    coverage = [[int(hist[h, at[v["col"]]].sum()) for h in range(n_hap)] for v in variant_rows]
    return dict(mutations=mutations, drugs=drugs, drug_profile=profile, haplotype_count=count, haplotype_coverage=coverage)
