"""The matrices, the stage parameters and the expected results of tests/test_gpu_stage_sequences.py, and the conditions that keep
those tests from passing vacuously (tests/test_stage_sequences_host.py checks them without a GPU).  Everything here is numpy and
the mirrors: nothing of the library is loaded.  Test infrastructure; nothing of the product imports it.

The eight stage calls of one context — class_pileup, class_codons, phase_rescue, phase_nearest, phase_recombinants,
variant_linkage, codon_deletions, read_stats — each with a LARGE and a SMALL parameter setting, so that the per-call tables of a
context shrink and grow from call to call:

    classes               17 (two passes of 16)          2
    haplotype patterns    65 x 22 positions              2 x 1
    linkage               P = 17, V = 33                 P = V = 1
    max_distance          3                              0
    compare (read stats)  the consensus                  None

An expected value is always a mirror applied to the rows (the numpy rule of test_gpu_class.expected for the class pileup)."""
import numpy as np

import class_codons_mirror
import deletion_mirror
import linkage_mirror
import nearest_mirror
import readstats_mirror
import recombinant_mirror
import rescue_mirror
import test_gpu_class

STAGES = ("class_pileup", "class_codons", "phase_rescue", "phase_nearest", "phase_recombinants", "variant_linkage",
          "codon_deletions", "read_stats")
LARGE, SMALL = "large", "small"
LARGE_COLS = 66                      # the fewest columns that hold the large setting's 22 codon starts
N_PLANTED = 5

# name: (reads, columns, seed).  A: three 512-read tiles, the last of one read; two 64-column groups, the second of two columns.
# A2: A's shape from another seed.  B: larger both ways.  C: smaller; its second word holds one valid bit.
SHAPES = {"A": (1025, 66, 101), "A2": (1025, 66, 202), "B": (2049, 130, 303), "C": (33, 9, 404)}


def codon_starts(l):
    """The codon starts the planted haplotypes differ at and the stages look at: 22 of them from 66 columns on, every third
    column below."""
    if l >= LARGE_COLS:
        return (np.arange(22) * ((l - 3) // 21)).astype(np.uint32)
    return np.arange(0, l - 2, 3).astype(np.uint32)


def codons_of(seq, starts):
    """codon indices of base codes seq[..., l] at the starts"""
    seq = np.asarray(seq).astype(np.int64)
    return np.stack([16 * seq[..., c] + 4 * seq[..., c + 1] + seq[..., c + 2] for c in (int(s) for s in starts)], axis=-1)


def mixture(n, l, seed):
    """(rows uint8[n][l], haps uint8[N_PLANTED][l]): reads of five planted haplotypes — whole, recombined at a breakpoint, or
    random — with substitutions, whole-codon and single-base deletions, masked bases, a few reads of a handful of columns, and
    ragged code-6 ends as test_gpu_class.code_rows has them."""
    rng = np.random.default_rng(seed)
    starts = codon_starts(l)
    vp = len(starts)
    haps = np.tile(rng.integers(0, 4, l).astype(np.uint8), (N_PLANTED, 1))
    for h in range(1, N_PLANTED):
        # every minor haplotype differs from the major one in each third of the window, and at a middle position of its own
        third = max(1, vp // 3)
        where = {int(rng.integers(0, third)), min(vp - 1, vp // 2 - 2 + h) if vp > 4 else (h % vp), int(rng.integers(vp - third, vp))}
        if h == 1:
            where.add(vp // 2)
        for p in where:
            c = int(starts[p]) + int(rng.integers(0, 3))
            haps[h, c] = (haps[h, c] + h) % 4 if h < 4 else (haps[h, c] + 1 + int(rng.integers(0, 3))) % 4
    which = rng.choice(N_PLANTED, size=n, p=[0.4, 0.2, 0.15, 0.15, 0.1])
    rows = haps[which].copy()
    ci = np.arange(l)[None, :]
    recombined = rng.random(n) < 0.10
    other, cut = rng.integers(0, N_PLANTED, n), rng.integers(1, l, n)
    swap = recombined[:, None] & (ci >= cut[:, None])
    rows[swap] = haps[other][swap]
    hit = rng.random((n, l)) < 0.004
    rows[hit] = (rows[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    noise = rng.random(n) < 0.04
    rows[noise] = rng.integers(0, 4, (int(noise.sum()), l))
    for c in starts[::4]:
        rows[rng.random(n) < 0.05, int(c):int(c) + 3] = 4
    rows[rng.random((n, l)) < 0.004] = 4
    rows[rng.random((n, l)) < 0.004] = 5
    lo, hi = rng.integers(0, l // 3 + 1, size=n), l - rng.integers(0, l // 3 + 1, size=n)
    short = rng.random(n) < 0.04
    hi[short] = lo[short] + rng.integers(0, 5, int(short.sum()))
    rows[(ci < lo[:, None]) | (ci >= hi[:, None])] = 6
    return rows.astype(np.uint8), haps


def top_codons(rows, col):
    """the two commonest codons among the reads that can be read at codon start `col` (the second made up when there is one)"""
    three = rows[:, col:col + 3].astype(np.int64)
    ok = (three < 4).all(axis=1)
    hist = np.bincount((16 * three[ok, 0] + 4 * three[ok, 1] + three[ok, 2]), minlength=64)
    order = np.argsort(-hist, kind="stable")
    first = int(order[0])
    return first, (int(order[1]) if hist[order[1]] else (first + 1) % 64)


def base_patterns(rows, starts, haps=None):
    """codons[N_PLANTED][Vp] the pattern rows start from: the planted haplotypes', or — for a matrix that has none — the consensus
    and four reads laid over it where they can be read"""
    if haps is not None:
        return codons_of(haps, starts)
    cons = readstats_mirror.consensus(rows).astype(np.int64)
    cons[cons > 3] = 0
    out = [cons]
    for i in np.linspace(0, len(rows) - 1, N_PLANTED - 1).astype(int):
        seq = np.where(rows[i] < 4, rows[i], cons)
        out.append(seq)
    return codons_of(np.stack(out), starts)


def parameters(rows, setting, seed, haps=None):
    """The arguments of all eight stages for `rows` in one setting, from `seed` and the rows alone."""
    n, l = rows.shape
    rng = np.random.default_rng([seed, 0 if setting == LARGE else 1])
    starts = codon_starts(l)
    mid = len(starts) // 2
    if setting == LARGE:
        assert l >= LARGE_COLS, "the large setting needs 22 codon starts"
        k = 17
        label = rng.integers(0, k, size=n).astype(np.uint16)
        label[label == 9] = 0xFFFF                                   # an empty class in the first pass
        label[rng.random(n) < 0.05] = 0xFFFE
        pos = starts
        base = base_patterns(rows, starts, haps)
        pattern = [row for row in base]
        while len(pattern) < 65:                                     # two chunks of 64 haplotypes
            row = base[int(rng.integers(0, len(base)))].copy()
            for p in rng.choice(np.arange(mid - 4, mid + 4), size=int(rng.integers(1, 4)), replace=False):
                row[p] = (row[p] + int(rng.integers(1, 64))) % 64
            pattern.append(row)
        pattern = np.stack(pattern).astype(np.uint8)
        min_positions, max_distance = 8, 3
        link_pos = starts[2:19]                                      # P = 17
        var_pos = np.repeat(np.arange(17), 2)[:33].astype(np.uint32)  # V = 33: more than one 16 x 16 block of the product
        var_codon = np.array([top_codons(rows, int(c))[j] for c in link_pos for j in (0, 1)][:33], dtype=np.uint8)
        compare = readstats_mirror.consensus(rows)
    else:
        k = 2
        label = np.array([0, 1, 0xFFFF, 2], dtype=np.uint16)[rng.integers(0, 4, size=n)]
        pos = starts[mid:mid + 1]
        pattern = np.array(top_codons(rows, int(pos[0])), dtype=np.uint8).reshape(2, 1)
        min_positions, max_distance = 1, 0
        link_pos, var_pos = pos, np.zeros(1, dtype=np.uint32)
        var_codon = pattern[1].copy()
        compare = None
    return dict(setting=setting, n_classes=k, label=label, pos_cols=pos.astype(np.uint32), pattern=pattern, min_positions=min_positions,
                max_distance=max_distance, link_pos=link_pos.astype(np.uint32), var_pos=var_pos, var_codon=var_codon, compare=compare)


def expected(rows, prm, stages=STAGES):
    """{stage: {array name: array}} by the mirrors, the arrays in the order the fetches return them."""
    out = {}
    for stage in stages:
        if stage == "class_pileup":
            counts, reads = test_gpu_class.expected(rows, prm["label"], prm["n_classes"])
            out[stage] = dict(counts=counts, class_reads=reads)
        elif stage == "class_codons":
            hist, reads = class_codons_mirror.class_codons(rows, prm["label"], prm["n_classes"], prm["pos_cols"])
            out[stage] = dict(hist=hist, class_reads=reads)
        elif stage == "phase_rescue":
            ids, hap_reads, tally = rescue_mirror.rescue(rows, prm["pos_cols"], prm["pattern"], prm["min_positions"])
            out[stage] = dict(rescue=ids, hap_reads=hap_reads, tally=tally)
        elif stage == "phase_nearest":
            ids, dist, hap_reads, tally = nearest_mirror.nearest(rows, prm["pos_cols"], prm["pattern"], prm["min_positions"], prm["max_distance"])
            out[stage] = dict(nearest=ids, dist=dist, hap_reads=hap_reads, tally=tally)
        elif stage == "phase_recombinants":
            r = recombinant_mirror.recombinants(rows, prm["pos_cols"], prm["pattern"], prm["min_positions"])
            out[stage] = {key: r[key] for key in ("left", "right", "prefix", "suffix", "parent_reads", "tally")}
        elif stage == "variant_linkage":
            r = linkage_mirror.linkage(rows, prm["link_pos"], prm["var_pos"], prm["var_codon"])
            out[stage] = {key: r[key] for key in ("both", "carry", "joint")}
        elif stage == "codon_deletions":
            out[stage] = dict(cnt=deletion_mirror.counts(rows))
        elif stage == "read_stats":
            out[stage] = dict(stats=readstats_mirror.stats(rows, prm["compare"]))
        else:
            raise ValueError(stage)
    return out


class Case:
    """A matrix with its parameters and expected results per setting, made once."""

    def __init__(self, name, rows, seed, haps=None, settings=None):
        self.name, self.rows, self.seed, self.haps = name, np.ascontiguousarray(rows, dtype=np.uint8), seed, haps
        if settings is None:
            settings = (LARGE, SMALL) if rows.shape[1] >= LARGE_COLS else (SMALL,)
        self.prm = {s: parameters(self.rows, s, seed, haps) for s in settings}
        self.exp = {s: expected(self.rows, self.prm[s]) for s in settings}

    @property
    def settings(self):
        return tuple(self.prm)


_cases = {}


def case(name):
    """The seeded matrices A, A2 (the issue's A'), B and C."""
    if name not in _cases:
        n, l, seed = SHAPES[name]
        rows, haps = mixture(n, l, seed)
        _cases[name] = Case(name, rows, seed, haps)
    return _cases[name]


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def check_not_vacuous():
    """What must hold of the expected values for the device tests to mean something; from the mirrors alone."""
    cases = {name: case(name) for name in SHAPES}
    for name, (n, l, _) in SHAPES.items():
        assert cases[name].rows.shape == (n, l)
    assert cases["A"].settings == cases["A2"].settings == cases["B"].settings == (LARGE, SMALL) and cases["C"].settings == (SMALL,)
    # a stale result is not a fresh one: per stage and setting the expected outputs of the matrices differ pairwise, and for A
    # against A' (same shapes, so no buffer moves and no size tells them apart) in at least one cell of EVERY output array
    names = list(SHAPES)
    for setting in (LARGE, SMALL):
        have = [x for x in names if setting in cases[x].settings]
        for stage in STAGES:
            for i, x in enumerate(have):
                for y in have[i + 1:]:
                    ex, ey = cases[x].exp[setting][stage], cases[y].exp[setting][stage]
                    assert any(not same(ex[key], ey[key]) for key in ex), (setting, stage, x, y)
            ea, eb = cases["A"].exp[setting][stage], cases["A2"].exp[setting][stage]
            for key in ea:
                if (setting, stage, key) == (SMALL, "phase_recombinants", "parent_reads"):
                    assert not ea[key].any() and not eb[key].any()      # (one position has no breakpoint: the table is zero by the rule)
                    continue
                assert ea[key].shape == eb[key].shape and (ea[key] != eb[key]).any(), (setting, stage, key)
    # ... and the two settings of one matrix differ too (a result left over from the other setting shows)
    for x in ("A", "A2", "B"):
        for stage in STAGES:
            if stage == "codon_deletions":       # (it has no parameters)
                continue
            el, es = cases[x].exp[LARGE][stage], cases[x].exp[SMALL][stage]
            assert any(not same(el[key], es[key]) for key in el), (x, stage)
    a = cases["A"].exp[LARGE]
    for stage in ("phase_rescue", "phase_nearest"):          # assigned, ambiguous, none, uninformative
        assert (a[stage]["tally"] > 0).all(), (stage, a[stage]["tally"])
        assert int(a[stage]["tally"].sum()) == SHAPES["A"][0]
    assert (a["phase_recombinants"]["tally"] > 0).all(), a["phase_recombinants"]["tally"]     # recombinant, ambiguous_parent, whole, none, uninformative
    assert (a["phase_nearest"]["dist"][a["phase_nearest"]["nearest"] < 65] > 0).any()       # some read is assigned at a distance
    prm = cases["A"].prm[LARGE]
    assert prm["pattern"].shape == (65, 22) and len(prm["link_pos"]) == 17 and len(prm["var_pos"]) == 33
    t = a["variant_linkage"]
    full = [(v, w) for v in range(33) for w in range(v + 1, 33) if prm["var_pos"][v] != prm["var_pos"][w]
            and min(linkage_mirror.pair_table(t, prm["var_pos"], v, w)[1:]) > 0]
    assert full, "no pair of variants with all four cells of its table non-zero"
    cnt = a["codon_deletions"]["cnt"]
    assert cnt[:, deletion_mirror.DEL3].any() and cnt[:, deletion_mirror.PARTIAL].any()
    reads = a["class_pileup"]["class_reads"]
    assert (reads > 0).sum() >= 2 and (reads == 0).any()
    for setting in (LARGE, SMALL):                           # the read stats compare something in one setting and nothing in the other
        st = cases["A"].exp[setting]["read_stats"]["stats"]
        assert st[readstats_mirror.MISMATCHES].any() == (setting == LARGE)
    # C: 33 reads, one valid bit in the second word; what it is small in is also what its results show
    c = cases["C"].exp[SMALL]
    assert c["read_stats"]["stats"].shape == (5, 33) and c["codon_deletions"]["cnt"].shape == (7, 4)
    assert (cases["C"].rows[32] != 6).any()                  # the read in the second word covers something
    return cases
