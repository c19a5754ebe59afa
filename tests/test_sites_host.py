"""The host-only half of phasing over deletion sites (docs/SPEC.md §18): the binding of jl_sites_assemble, the mirror of the site
matrix on seeded rows against the counts of §16's mirror, and two designed, noise-free samples run through the oracle's phasing
over the mirror's rows — with exact, designed counts.  No GPU: the library only has to load."""
import os
import re

import numpy as np
import pytest

import deletion_mirror as dm
import oracle_lib
import sites_mirror as sm
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 4


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def test_header_library_and_binding_have_the_call():
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    assert re.search(r"\bint jl_sites_assemble\(jl_ctx \*pc, jl_ctx \*src, const jl_site \*sites, uint32_t n_sites\);", header)
    for word in ("JL_SITE_CODON = 0", "JL_SITE_DELETION = 1", "JL_SITE_NO_FILL = 0xFF", "JL_SITE_PRESENT = 0", "JL_SITE_DELETED = 1",
                 "JL_SITES_MAX = 4096"):
        assert word in header, word
    lib = capi.load_library()
    assert "jl_sites_assemble" in capi.EXPORTS and hasattr(lib, "jl_sites_assemble")
    assert hasattr(capi.Juliet, "sites_assemble")
    assert capi.SITE.itemsize == 8 and capi.SITE.fields["kind"][1] == 4 and capi.SITE.fields["fill"][1] == 5
    assert (capi.SITE_CODON, capi.SITE_DELETION, capi.SITE_NO_FILL, capi.SITE_PRESENT, capi.SITE_DELETED, capi.SITES_MAX) == \
        (sm.CODON, sm.DELETION, sm.NO_FILL, sm.PRESENT, sm.DELETED, sm.SITES_MAX)


def make_case(n, n_cols, seed, n_hap=4):
    """tests/test_gpu_deletions.py's: copies of a few haplotype rows with seeded damage by kind of read (a clean codon deletion in
    any frame, one-, two- and six-base deletions, N cells, ragged ends, uncovered reads)."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    rows = haps[rng.integers(0, n_hap, size=n)].copy()
    kind = rng.integers(0, 10, size=n)
    ci = np.arange(n_cols)[None, :]
    for k, length in ((0, 3), (1, 1), (2, 2), (3, 6)):
        start = rng.integers(0, n_cols - length + 1, size=n)[:, None]
        rows[(kind == k)[:, None] & (ci >= start) & (ci < start + length)] = GAP
    rows[(kind == 4)[:, None] & (rng.random(size=rows.shape) < 2.0 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    rows[(kind == 5)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 6] = 6
    return rows


def codon_index(cells):
    return 16 * cells[:, 0].astype(np.int64) + 4 * cells[:, 1] + cells[:, 2]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mirror_against_the_deletion_counts(seed):
    n, n_cols = 3000, 12
    rows = make_case(n, n_cols, seed)
    cnt = dm.counts(rows)
    cols = list(range(n_cols - 2))
    out = sm.recode(rows, [(c, sm.DELETION, sm.NO_FILL) for c in cols])
    assert cnt[:, dm.DEL3].all() and cnt[:, dm.PARTIAL].all()
    for k, c in enumerate(cols):
        cells, src = out[:, 3 * k:3 * k + 3], rows[:, c:c + 3]
        whole = (cells < 4).all(axis=1)
        present, deleted = whole & (codon_index(cells) == sm.PRESENT), whole & (codon_index(cells) == sm.DELETED)
        assert present.sum() == cnt[c, dm.CODON] and deleted.sum() == cnt[c, dm.DEL3]
        other = ~(present | deleted)
        assert other.any() and (cells[other] == src[other]).all() and not (cells[other] < 4).all(axis=1).any()
    # a filled codon site differs from the source on the del3 reads only, which carry the fill; an unfilled one not at all
    for fill in (0, 27, 63):
        out = sm.recode(rows, [(c, sm.CODON, fill) for c in cols])
        for k, c in enumerate(cols):
            cells, src = out[:, 3 * k:3 * k + 3], rows[:, c:c + 3]
            del3 = (src == GAP).all(axis=1)
            assert (cells[~del3] == src[~del3]).all() and (codon_index(cells[del3]) == fill).all() and del3.sum() == cnt[c, dm.DEL3]
    assert (sm.recode(rows, [(c, sm.CODON, sm.NO_FILL) for c in cols]) == np.concatenate([rows[:, c:c + 3] for c in cols], axis=1)).all()


cod, scenario_a, scenario_b = sm.cod, sm.scenario_a, sm.scenario_b


def test_scenario_a_a_deletion_alone_is_a_haplotype(oracle):
    rows, ref, var, dels, (v1, v2) = scenario_a()
    plain = oracle.phase(rows, var)
    assert plain["summary"]["n_haplotypes"] == 3 and plain["hap_count"].tolist() == [130, 40, 20]     # the deletion-only reads: wild type
    assert plain["summary"]["damaged_reads"] == 0
    sites = sm.build_sites(var, dels)
    assert sites == [(6, sm.CODON, sm.NO_FILL), (15, sm.DELETION, sm.NO_FILL), (21, sm.CODON, sm.NO_FILL)]
    table = sm.build_table(var, sites)
    assert table["col"].tolist() == [0, 3, 6] and table["codon"].tolist() == [v1, sm.DELETED, v2] and table["ref_codon"][1] == sm.PRESENT
    ph = oracle.phase(sm.recode(rows, sites), table)
    assert ph["summary"]["n_haplotypes"] == 4 and ph["hap_count"].tolist() == [100, 40, 30, 20]
    assert ph["summary"]["reported_reads"] == 190 and ph["summary"]["damaged_reads"] == 0
    rep = sm.report(ph, sites, table)
    r1, r2 = sm.CODONS[cod(ref[6:9])], sm.CODONS[cod(ref[21:24])]
    assert rep["variant_positions_abs"] == [7, 22] and rep["deletion_positions_abs"] == [16]
    assert [h["codons"] for h in rep["haplotypes"]] == [[r1, r2], [sm.CODONS[v1], r2], [r1, r2], [r1, sm.CODONS[v2]]]
    assert [h["deletions"] for h in rep["haplotypes"]] == [[False], [False], [True], [True]]
    assert rep["deletion_hit"] == {15: [False, False, True, True]}
    assert rep["codon_hit"] == [[False, True, False, False], [False, False, False, True]]
    # the ids: every read of the two deleted populations is in its own haplotype
    deleted = (rows[:, 15:18] == GAP).all(axis=1)
    assert set(ph["read_hap"][deleted].tolist()) == {2, 3} and not set(ph["read_hap"][~deleted].tolist()) & {2, 3}


def test_scenario_b_carriers_at_a_variant_position_stop_being_damage(oracle):
    rows, ref, var, dels, (v,) = scenario_b()
    plain = oracle.phase(rows, var)
    assert plain["summary"]["damaged_reads"] == 25 and plain["summary"]["marginal_gap"] == 25
    assert plain["hap_count"].tolist() == [100, 40]
    r = cod(ref[9:12])
    sites = sm.build_sites(var, dels)
    assert sites == [(9, sm.CODON, r), (9, sm.DELETION, sm.NO_FILL)]
    table = sm.build_table(var, sites)
    assert table["col"].tolist() == [0, 3] and table["codon"].tolist() == [v, sm.DELETED]
    ph = oracle.phase(sm.recode(rows, sites), table)
    assert ph["hap_count"].tolist() == [100, 40, 25]
    assert ph["summary"]["damaged_reads"] == plain["summary"]["damaged_reads"] - 25 == 0 and ph["summary"]["marginal_gap"] == 0
    assert ph["summary"]["reported_reads"] == 165
    rep = sm.report(ph, sites, table)
    assert rep["variant_positions_abs"] == [10] and rep["deletion_positions_abs"] == [10]
    assert [h["codons"] for h in rep["haplotypes"]] == [[sm.CODONS[r]], [sm.CODONS[v]], ["---"]]
    assert [h["deletions"] for h in rep["haplotypes"]] == [[False], [False], [True]]
    assert rep["codon_hit"] == [[False, True, False]] and rep["deletion_hit"] == {9: [False, False, True]}
