"""The host-only half of the per-class codon tables (docs/SPEC.md §24): the numpy mirror of the counting rule against the
oracle's codon histogram, and what the header and the Python binding declare.  No GPU: the library only has to load."""
import os
import re

import numpy as np
import pytest

import class_codons_mirror as mirror
import oracle_lib
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def ragged_rows(n, l, seed):
    """Seeded codes 0..5, bases four times as likely as '-' and N, with ragged code-6 ends."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5], dtype=np.uint8), size=(n, l))
    lo, hi = rng.integers(0, l // 3 + 1, size=n), l - rng.integers(0, l // 3 + 1, size=n)
    ci = np.arange(l)[None, :]
    rows[(ci < lo[:, None]) | (ci >= hi[:, None])] = 6
    return rows


WINDOWS = [(1, 3, 1), (40, 9, 2), (257, 64, 3), (1000, 130, 4)]


@pytest.mark.parametrize("n,l,seed", WINDOWS)
def test_one_class_is_the_oracles_codon_histogram(oracle, n, l, seed):
    rows = ragged_rows(n, l, seed)
    cols = np.arange(l - 2, dtype=np.uint32)            # every start, the three frames together
    hist, reads = mirror.class_codons(rows, np.zeros(n, dtype=np.uint16), 1, cols)
    exp, cov = oracle.codon_hist(rows, cols)
    assert hist.dtype == np.uint32 and hist.shape == (1, l - 2, 64)
    assert (hist[0] == exp).all() and (hist[0].sum(axis=1) == cov).all() and reads.tolist() == [n]


@pytest.mark.parametrize("n,l,seed", WINDOWS)
@pytest.mark.parametrize("k", [1, 5, 17])
def test_classes_sum_to_the_labelled_reads(oracle, n, l, seed, k):
    rows = ragged_rows(n, l, seed + 10)
    rng = np.random.default_rng(seed + k)
    pool = np.array(list(range(k)) + [k, 0xFFFE, 0xFFFF], dtype=np.uint16)
    lab = pool[rng.integers(0, len(pool), size=n)]
    cols = np.arange(0, l - 2, 2, dtype=np.uint32)
    hist, reads = mirror.class_codons(rows, lab, k, cols)
    exp, cov = oracle.codon_hist(rows[lab < k], cols) if (lab < k).any() else (np.zeros((len(cols), 64), np.uint32), None)
    assert (hist.sum(axis=0) == exp).all()
    assert (reads == np.bincount(lab[lab < k], minlength=k)).all()
    for c in range(k):                                  # ... and every class alone is the oracle over its own reads
        if (lab == c).any():
            assert (hist[c] == oracle.codon_hist(rows[lab == c], cols)[0]).all()
        else:
            assert not hist[c].any()


def test_header_and_binding_declare_the_call():
    text = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    assert re.search(r"int\s+jl_class_codons_async\(jl_ctx \*ctx, const uint16_t \*label, uint32_t n_classes,\s*const uint32_t \*col, uint32_t n_pos\);", text)
    assert re.search(r"int\s+jl_class_codons_fetch\(jl_ctx \*ctx, uint32_t \*hist[^,]*,\s*uint32_t \*class_reads[^)]*\);", text)
    m = re.search(r"JL_CLASS_CODONS_CELLS\s*=\s*1\s*<<\s*20", text)
    assert m, "JL_CLASS_CODONS_CELLS = 2^20 is not in the header"
    lib = capi.load_library()
    for name in ("jl_class_codons_async", "jl_class_codons_fetch"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "class_codons") and hasattr(capi.Juliet, "class_codons_fetch")


# ---------------------------------------------------------------------------------------------- the front-end rule on hand-made tables
AAA, AAC, ACG, ATG, GTG, TAA = 0, 1, 6, 14, 46, 48


def table(n_hap, n_entries, cells):
    hist = np.zeros((n_hap, n_entries, 64), dtype=np.uint32)
    for (h, e, codon), n in cells.items():
        hist[h, e, codon] = n
    return hist


def pos(gene_index, gene, position, col, ref, drms=()):
    return dict(gene_index=gene_index, gene=gene, position=position, col=col, ref=ref, drms=list(drms))


def test_front_end_a_tie_goes_to_the_lowest_index():
    hist = table(1, 1, {(0, 0, ATG): 5, (0, 0, AAC): 5, (0, 0, GTG): 4})
    out = mirror.front_end(hist, [10], [pos(0, "g", 4, 10, ATG)], [14], [1.0])
    (m,) = out["mutations"][0]
    assert (m["codon"], m["amino_acid"], m["count"], m["coverage"], m["frequency"]) == ("AAC", "N", 5, 14, 5 / 14)
    assert (m["ref_codon"], m["ref_amino_acid"], m["gene"], m["position"], m["drms"]) == ("ATG", "M", "g", 4, [])
    # ... and to the reference when the reference is the lower of the two: no mutation
    out = mirror.front_end(hist, [10], [pos(0, "g", 4, 10, AAC)], [14], [1.0])
    assert out["mutations"] == [[]] and out["drugs"] == [[]] and out["drug_profile"] == []


def test_front_end_zero_coverage_in_one_haplotype():
    hist = table(2, 1, {(0, 0, GTG): 7})
    out = mirror.front_end(hist, [3], [pos(0, "g", 2, 3, ATG)], [7, 9], [0.4375, 0.5625], [dict(col=3, codon=GTG)])
    assert [len(m) for m in out["mutations"]] == [1, 0]
    assert out["haplotype_count"] == [[7, 0]] and out["haplotype_coverage"] == [[7, 0]]


def test_front_end_a_wildcard_drm_and_the_profile():
    drms = [dict(name="zeta", positions=["M184*"]), dict(name="alpha", positions=["184V", "K65R"]), dict(name="none", positions=["M184I"])]
    hist = table(3, 2, {(0, 0, GTG): 9, (0, 0, ATG): 1, (1, 0, TAA): 4, (2, 0, ATG): 6, (0, 1, AAA): 10, (1, 1, AAA): 4, (2, 1, AAA): 6})
    positions = [pos(0, "rt", 184, 30, ATG, drms), pos(0, "rt", 65, 0, AAA, drms)]
    # written with position 184 first; entry 0 of the table is column 0 (position 65), entry 1 column 30 (position 184)
    hist = hist[:, ::-1]
    out = mirror.front_end(hist, [0, 30], positions, [10, 4, 6], [0.5, 0.2, 0.3])
    assert [[(m["position"], m["amino_acid"], m["drms"]) for m in ms] for ms in out["mutations"]] == \
        [[(184, "V", ["zeta", "alpha"])], [(184, "X", ["zeta"])], []]            # the wildcard takes a stop codon too
    assert out["drugs"] == [["alpha", "zeta"], ["zeta"], []]
    assert out["drug_profile"] == [dict(drug="alpha", haplotypes=[True, False, False], reads=10, frequency=0.5),
                                   dict(drug="zeta", haplotypes=[True, True, False], reads=14, frequency=0.0 + 0.5 + 0.2)]


def test_front_end_two_genes_share_a_column():
    """Positions of two genes on one column are one entry of the table; each gene reports it under its own name, position,
    reference and DRMs, in (gene index, position) order."""
    hist = table(1, 2, {(0, 0, GTG): 8, (0, 1, ACG): 8})
    a = [dict(name="da", positions=["7V"])]
    b = [dict(name="db", positions=["3V"])]
    positions = [pos(1, "second", 3, 12, ATG, b), pos(0, "first", 7, 12, AAA, a), pos(0, "first", 8, 15, ACG, a)]
    out = mirror.front_end(hist, [12, 15], positions, [8], [1.0])
    assert [(m["gene"], m["position"], m["ref_codon"], m["drms"]) for m in out["mutations"][0]] == [("first", 7, "AAA", ["da"]), ("second", 3, "ATG", ["db"])]
    assert out["drugs"] == [["da", "db"]]


def test_front_end_without_drms_and_without_haplotypes():
    hist = table(1, 1, {(0, 0, GTG): 3})
    out = mirror.front_end(hist, [0], [pos(0, "g", 1, 0, ATG)], [3], [1.0])
    assert out["mutations"][0][0]["drms"] == [] and out["drugs"] == [[]] and out["drug_profile"] == []
    out = mirror.front_end(np.zeros((0, 1, 64), dtype=np.uint32), [0], [pos(0, "g", 1, 0, ATG)], [], [], [dict(col=0, codon=GTG)])
    assert out == dict(mutations=[], drugs=[], drug_profile=[], haplotype_count=[[]], haplotype_coverage=[[]])
    out = mirror.front_end(table(1, 1, {(0, 0, GTG): 3}), [0], [pos(0, "g", 1, 0, None)], [3], [1.0])     # no reference codon there
    assert out["mutations"] == [[]]
