"""The host-only half of phasing over insertion sites (docs/SPEC.md §19): tests/insertion_sites_mirror.py against §17's mirror —
the events, counted, are its counters and its table; the insertion sites of the mirror's site matrix, counted by class, are its
counters again — the layout of jl_insertion_event, the constants, and a designed sample whose populations differ by an inserted
codon only, phased by the oracle over the mirror's rows.  No GPU: the library only has to load.

`site_reads` and `site_case` make the reads and tables the device tests use too (tests/test_gpu_insertion_sites.py)."""
import os
import re

import numpy as np
import pytest

import insertion_mirror as im
import insertion_sites_mirror as ism
import oracle_lib
import records_expand
import sites_mirror as sm
from minorseq_amd import capi
from test_gpu_insertions import WB, make_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = sm.NO_FILL


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


# ---------------------------------------------------------------------------------------------- reads with designed insertions
L = 24
J_FIRST, J_MIXED, J_MANY, J_LAST = 1, 9, 15, L - 1          # the first and the last junction; a column with all three kinds of site
DEL_MIXED, DEL_ALONE = 9, 18                                # haplotype 1 has the codon at 9 deleted, haplotype 2 the one at 18


def word6(i):
    return "".join("ACGT"[(i >> (2 * (5 - j))) & 3] for j in range(6))


def key(col, text):
    return (col, len(text), sum("ACGT".index(b) << (2 * j) for j, b in enumerate(text)))


POOLS = {J_FIRST: ["GGG"], J_MIXED: ["ACG", "CCGTTA", "TTT"], J_MANY: [word6(7 * i + 3) for i in range(70)], J_LAST: ["AAA", "AAAAAA"]}
LISTED = {J_FIRST: 1, J_MIXED: 2, J_MANY: 62, J_LAST: 2}      # how many of a junction's pool, in the table's order, are listed


def listed_alleles(junctions=None):
    """[(col, len, seq)] ascending: per junction the first LISTED[j] keys of its pool."""
    out = []
    for j in sorted(POOLS if junctions is None else junctions):
        out += sorted(key(j, t) for t in POOLS[j])[:LISTED[j]]
    return out


def build_read(hap, s, e, dels, inserts):
    """The read over columns [s, e) of haplotype row `hap`: '=' runs of its bases, a 'D' of three per codon start in `dels`, the
    text of inserts[c] as an 'I' in front of column c (s < c < e)."""
    ops, bases = [], []

    def add(op, ln, text=""):
        if ops and ops[-1][0] == op and op != "I":
            ops[-1] = (op, ops[-1][1] + ln)
        else:
            ops.append((op, ln))
        bases.append(text)

    for c in range(s, e):
        if c in inserts and c > s:
            add("I", len(inserts[c]), inserts[c])
        if any(d <= c < d + 3 for d in dels):
            add("D", 1)
        else:
            add("=", 1, "ACGT"[hap[c]])
    return (s, ops, "".join(bases))


def site_reads(n, seed):
    """n reads over L columns, copies of three haplotype rows.  Haplotype h carries the allele POOLS[J_MIXED][h] at junction 9; at
    the other junctions a read carries a pool allele now and then; one junction in ten of a read is damaged instead: a two-base
    insertion, one with an N, an in-frame one from no pool.  Some reads begin after column 0 or end before column L.  The first
    six reads are anchors at J_MANY: a listed allele, a pool allele that is not listed, a frameshift, an unreadable one, none, and
    a read that begins beyond it."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 4, size=(3, L))
    many = sorted(POOLS[J_MANY], key=lambda t: key(J_MANY, t))
    anchors = [many[0], many[-1], "AC", "ANG", None, None]
    reads = []
    for i in range(n):
        h = int(rng.integers(0, 3))
        dels = [DEL_MIXED] if h == 1 else [DEL_ALONE] if h == 2 else []
        inserts = {J_MIXED: POOLS[J_MIXED][h]}
        if rng.random() < 0.5:
            inserts[J_MANY] = POOLS[J_MANY][int(rng.integers(0, 70))]
        if rng.random() < 0.3:
            inserts[J_FIRST] = "GGG"
        if rng.random() < 0.3:
            inserts[J_LAST] = POOLS[J_LAST][int(rng.integers(0, 2))]
        for j in (J_FIRST, J_MIXED, J_MANY, J_LAST):
            if rng.random() < 0.1:
                inserts[j] = ("AC", "ANG", "CAT", "C" * 33)[int(rng.integers(0, 4))]
        s = int(rng.integers(1, 9)) if rng.random() < 0.15 else 0
        e = (16, 17, 18, 21, 22, 23)[int(rng.integers(0, 6))] if rng.random() < 0.15 else L
        if i < len(anchors):
            s, e = (16, L) if i == 5 else (0, L)
            inserts.pop(J_MANY, None)
            if anchors[i]:
                inserts[J_MANY] = anchors[i]
        reads.append(build_read(haps[h], s, e, dels, inserts))
    return reads


def all_sites():
    """Insertion sites at the first and the last junction, one with 62 listed alleles, and at column 9 a codon site (filled), a
    deletion site and an insertion site together; a codon site and a deletion site elsewhere."""
    return [(J_FIRST, ism.INSERTION, NF), (3, sm.CODON, NF), (DEL_MIXED, sm.CODON, 27), (DEL_MIXED, sm.DELETION, NF), (J_MIXED, ism.INSERTION, NF),
            (J_MANY, ism.INSERTION, NF), (DEL_ALONE, sm.DELETION, NF), (J_LAST, ism.INSERTION, NF)]


def site_case(n, seed):
    """-> (rec, rows uint8[n][L], events, sites, alleles): nothing passes vacuously — all six classes of §19's table occur."""
    rec = im.records(site_reads(n, seed), with_qual=True)
    rows = records_expand.expand_reference(rec, L, 0, 0)
    evs = ism.events(rec, L)
    sites, alleles = all_sites(), listed_alleles()
    return rec, rows, evs, sites, alleles


def holds_all_classes(matrix, sites, alleles):
    cl = ism.classes(matrix, sites, alleles).values()
    return all(any(c[k] for c in cl) for k in ("none", "other", "gap", "n", "out")) and any(sum(c["listed"]) for c in cl)


# ---------------------------------------------------------------------------------------------- the events against §17's mirror
@pytest.mark.parametrize("n,n_cols", [(1, 130), (33, 64), (65, 129), (257, 3), (513, 64)])
def test_events_aggregate_to_the_counters_and_the_table(n, n_cols):
    rec = im.records(make_reads(n, n_cols, 1000 * n + n_cols), with_qual=True)
    for min_qv, qmask in ((0, None), (20, None), (20, capi.qmask_from_quals(rec["seq_off"], rec["qual"], rec["qual_off"], 20))):
        jcnt, alleles = im.walk(rec, n_cols, WB, min_qv, qmask)
        evs = ism.events(rec, n_cols, WB, min_qv, qmask)
        cnt, table = ism.aggregate(evs, n_cols)
        assert (cnt == jcnt[:, 1:]).all() and table == alleles
        assert jcnt[:, 1:].any(axis=0).all() and len(alleles) >= 2
        assert all((ln, seq) == (0, 0) for _, _, ln, kind, seq in evs if kind != im.INFRAME)


@pytest.mark.parametrize("n", [31, 129, 1025])
def test_site_matrix_classes_are_the_counters(n):
    rec, rows, evs, sites, alleles = site_case(n, n)
    jcnt, table = im.walk(rec, L)
    cnt, agg = ism.aggregate(evs, L)
    assert (cnt == jcnt[:, 1:]).all() and agg == table
    m = ism.site_matrix(rows, evs, sites, alleles)
    assert m.shape == (n, 3 * len(sites)) and not (m == 7).any() and holds_all_classes(m, sites, alleles)
    count = {(c, l, s): k for c, l, s, k in table}
    for k, cl in ism.classes(m, sites, alleles).items():
        col = sites[k][0]
        mine = [a for a in alleles if a[0] == col]
        assert cl["listed"] == [count.get(a, 0) for a in mine]
        assert (cl["gap"], cl["n"]) == (jcnt[col, im.FRAMESHIFT], jcnt[col, im.UNREAD])
        assert cl["none"] + sum(cl["listed"]) + cl["other"] == int(jcnt[col, im.SPAN]) - int(jcnt[col, im.FRAMESHIFT]) - int(jcnt[col, im.UNREAD])
        assert cl["other"] == int(jcnt[col, im.INFRAME]) - sum(cl["listed"])
        assert cl["out"] == n - int(jcnt[col, im.SPAN])
    # the codon and the deletion sites are §18's, untouched by the events
    plain = [(i, s) for i, s in enumerate(sites) if s[1] != ism.INSERTION]
    assert (m[:, [3 * i + j for i, _ in plain for j in range(3)]] == sm.recode(rows, [s for _, s in plain])).all()
    # ... and with no insertion site the matrix is §18's
    assert (ism.site_matrix(rows, evs, [s for _, s in plain], []) == sm.recode(rows, [s for _, s in plain])).all()


def test_layout_and_constants():
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    assert re.search(r"typedef struct \{\s*uint32_t read, col, len, kind;\s*uint64_t seq;\s*\} jl_insertion_event;", header)
    e = capi.INSERTION_EVENT
    assert e.itemsize == 24 and [e.fields[k][1] for k in ("read", "col", "len", "kind", "seq")] == [0, 4, 8, 12, 16]
    assert e == ism.EVENT
    for word in ("JL_SITE_INSERTION = 2", "JL_SITE_INS_NONE = 0", "JL_SITE_INS_OTHER = 63", "JL_SITE_INS_MAX_ALLELES = 62"):
        assert word in header, word
    assert (capi.SITE_INSERTION, capi.SITE_INS_NONE, capi.SITE_INS_OTHER, capi.SITE_INS_MAX_ALLELES) == \
        (ism.INSERTION, ism.INS_NONE, ism.INS_OTHER, ism.INS_MAX_ALLELES) == (2, 0, 63, 62)
    assert re.search(r"\bint jl_sites_assemble_alleles\(jl_ctx \*pc, jl_ctx \*src, const jl_site \*sites, uint32_t n_sites, "
                     r"const jl_insertion_allele \*alleles,\s*uint32_t n_alleles\);", header)
    lib = capi.load_library()
    for name in ("jl_msa_track_insertion_reads", "jl_insertion_reads_fetch", "jl_sites_assemble_alleles"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    for name in ("track_insertion_reads", "insertion_reads", "sites_assemble_alleles"):
        assert hasattr(capi.Juliet, name)


def test_a_population_that_differs_by_an_inserted_codon_is_a_haplotype(oracle):
    """100 wild-type reads, 40 with a codon variant at column 6, 30 with GAT inserted in front of column 12 and nothing else, 5
    with a two-base insertion there.  Plain phasing over the variant position sees two haplotypes, 130 and 40 reads, and 5 more in
    the first; with the insertion site the carriers are a third haplotype and the frame-shifted reads are GAP-damaged."""
    rng = np.random.default_rng(19)
    ref = rng.integers(0, 4, size=L)
    var = ref.copy()
    v = sm.other_codon(sm.cod(ref[6:9]), 1)
    var[6:9] = sm.bases(v)
    reads = [build_read(ref, 0, L, [], {})] * 100 + [build_read(var, 0, L, [], {})] * 40 + [build_read(ref, 0, L, [], {12: "GAT"})] * 30 + \
        [build_read(ref, 0, L, [], {12: "GA"})] * 5
    rec = im.records([reads[i] for i in np.random.default_rng(3).permutation(len(reads))], with_qual=True)
    rows = records_expand.expand_reference(rec, L, 0, 0)
    variants = sm.variant_rows([(6, sm.cod(ref[6:9]), v)])
    plain = oracle.phase(rows, variants)
    assert plain["hap_count"].tolist() == [135, 40] and plain["summary"]["damaged_reads"] == 0
    sites, alleles = ism.build_sites(variants, [], [key(12, "GAT")], phase_deletions=False)
    assert sites == [(6, sm.CODON, NF), (12, ism.INSERTION, NF)] and alleles == [key(12, "GAT")]
    table = ism.build_table(variants, sites, alleles)
    assert [(int(r["col"]), int(r["codon"]), int(r["ref_codon"])) for r in table] == [(0, v, sm.cod(ref[6:9])), (3, 1, ism.INS_NONE)]
    ph = oracle.phase(ism.site_matrix(rows, ism.events(rec, L), sites, alleles), table)
    assert ph["hap_count"].tolist() == [100, 40, 30]
    assert ph["summary"]["damaged_reads"] == 5 and ph["summary"]["marginal_gap"] == 5
    rep = ism.report(ph, sites, alleles)
    assert rep["insertions"] == [[False], [False], [True]] and rep["hit"][key(12, "GAT")] == [False, False, True]
