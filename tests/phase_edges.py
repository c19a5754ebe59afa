"""Designed windows for the phasing kernels (test infrastructure, like pileup_edges.py and call_edges.py; nothing of the product
imports it).

Phasing (minorseq_amd/csrc/kernels_phase.hip, phase_plan.h) has its edges where the position count changes the pipeline (10 / 11
and 20 / 21 positions, the third key word at 30 / 31), where a workgroup's 2048 reads or its 1024-slot LDS table end, where the
plan leaves its LDS bitset (131072 / 131073 columns), where a group has exactly min_reads reads, where the per-read ids change
their width and where the selection's capacities end.  This module builds small row matrices with host variant tables that sit
on those edges and states what phasing must give for them in plain numpy, from docs/SPEC.md §8 (no code shared with oracle/).

Symbols as everywhere: A C G T = 0..3, '-' = 4, N = 5, not covered = 6; codon index = 16 b0 + 4 b1 + b2."""
import numpy as np

from minorseq_amd import capi

VARIANT = capi.VARIANT
GENE = capi.GENE
SUMMARY_FIELDS = ("reported_reads", "insufficient_reads", "damaged_reads", "marginal_gap", "marginal_heteroduplex", "marginal_partial",
                  "n_positions", "n_haplotypes")
HAP_INSUFFICIENT, HAP_DAMAGED = 0xFFFE, 0xFFFF
ERR_OVERFLOW = -5                   # include/juliet_hip.h: JL_ERR_OVERFLOW

# ------------------------------------------------------------------------------------------------ the constants, mirrored
# (tests/test_phase_edges_host.py compares each with the line it mirrors)
POS_PER_WORD = 10                   # jl_internal.h: #define JL_POS_PER_WORD 10u
FORM_ONE_WORD_MAX = 10              # capi.hip phase_form_for: vp <= JL_POS_PER_WORD keeps the form
FORM_TWO_WORD_MAX = 20              # capi.hip phase_form_for: vp <= 2u * JL_POS_PER_WORD takes the two-word launch
PLAN_LDS_COLS = 4096 * 32           # phase_plan.h: #define JL_PLAN_LDS_WORDS 4096u, one bit a column
LDS_SLOTS = 1024                    # kernels_phase.hip: constexpr uint32_t kLdsSlots = 1024
BLOCK_READS = 256 * 8               # kernels_phase.hip jl_phase_grid_blocks: 256 lanes a workgroup, a lane = a byte of a plane = 8 reads
CAND_CAP = 4096                     # jl_internal.h: #define JL_CAND_CAP 4096u
MAX_HAPLOTYPES = 702                # juliet_hip.h: JL_MAX_HAPLOTYPES = 702
PACK_MAX_HAP = 128                  # jl_internal.h: #define JL_PACK_MAX_HAP 128u (kSelCand: what the selection out of LDS ranks)
ID4_MAX_H = 14                      # jl_internal.h: #define JL_ID4_MAX_H 14u
ID8_MAX_H = 254                     # jl_internal.h: #define JL_ID8_MAX_H 254u
INLINE_IDS_MAX_BLOCKS = 128         # jl_internal.h: #define JL_INLINE_IDS_MAX_BLOCKS 128u
LINE_READS = 1024                   # capi.hip jl_plane_stride: a plane grows by 128 bytes = 1024 reads
FORM_MULTI, FORM_ONE, FORM_TWO = 0, 1, 2   # jl_internal.h: enum class jl_phase_form
PACK_MAX_VAR = 128                  # jl_internal.h: #define JL_PACK_MAX_VAR 128u   (table rows the selection out of LDS takes)
SEL_HIT_BYTES = 8192                # jl_internal.h: #define JL_SEL_HIT_BYTES 8192u (rows x haplotypes it holds)


def form_for(vp, start=FORM_ONE):
    """The pipeline a context that phased in `start` takes for vp positions (capi.hip phase_form_for: it only grows)."""
    if vp <= FORM_ONE_WORD_MAX:
        return start
    if vp <= FORM_TWO_WORD_MAX and start == FORM_ONE:
        return FORM_TWO
    return FORM_MULTI


def form_of_run(vp, n_rows, n_candidates, start=FORM_ONE):
    """... and for a whole result: the two-word launch has only the selection out of LDS, so more than 128 candidates or table rows,
    or more than 8192 cells of hit, hand the context to the multi-word pipeline (kernels_phase.hip: phase_select_lds returns false)."""
    form = form_for(vp, start)
    if form == FORM_TWO and (n_candidates > PACK_MAX_HAP or n_rows > PACK_MAX_VAR or n_rows * n_candidates > SEL_HIT_BYTES):
        return FORM_MULTI
    return form


def key_words(vp):
    return -(-vp // POS_PER_WORD)


def id_bits(h, vp):
    """Width of the per-read ids of a run with h haplotypes (nothing phased: 4)."""
    return 4 if vp == 0 or h <= ID4_MAX_H else (8 if h <= ID8_MAX_H else 16)


def grid_blocks(n_reads):
    """Workgroups of a window's phasing launch: one per 2048 reads of the padded planes and the one that compacts the rows."""
    pad = -(-n_reads // LINE_READS) * LINE_READS
    return -(-pad // BLOCK_READS) + 1


INLINE_MAX_READS = (INLINE_IDS_MAX_BLOCKS - 1) * BLOCK_READS   # the deepest window whose launch writes its ids itself


# ------------------------------------------------------------------------------------------------ the expected result
def phase(rows, table, min_reads, wrong=None):
    """SPEC §8 on a row matrix uint8[n][l], a variant table (col and codon are read) and min_reads.  Returns the fields of
    oracle_lib.Oracle.phase (summary, pos_cols, hap_count, hap_pattern, hit, read_hap, cooc) and, for the tests of the cases,
    `patterns` int16[n][Vp] (-1 in damaged reads), `group_counts` (pattern order) and `n_candidates`.

    wrong: one of the wrong kernels the cases must be able to tell from the right one (tests/test_phase_edges_host.py) —
    'gt' (min_reads compared with >), 'last_col' (c + 2 <= n_cols), 'drop10th' (the 10th position of a word not in the key),
    'no_word1' (positions 10..19 not in the key), 'ties_reversed' (equal counts ordered by pattern descending)."""
    rows = np.asarray(rows, dtype=np.uint8)
    n, l = rows.shape
    nv = len(table)
    vcol = table["col"].astype(np.int64)
    vcodon = table["codon"].astype(np.int64)
    inside = vcol + 2 <= l if wrong == "last_col" else vcol + 2 < l
    pos = np.unique(vcol[inside])
    vp = len(pos)
    summary = dict.fromkeys(SUMMARY_FIELDS, 0)
    summary["n_positions"] = vp
    if vp == 0:
        return dict(summary=summary, pos_cols=pos.astype(np.uint32), hap_count=np.zeros(0, np.uint32), hap_pattern=np.zeros((0, 0), np.uint8),
                    hit=np.zeros((nv, 0), np.uint8), read_hap=np.full(n, HAP_DAMAGED, np.uint16), cooc=np.zeros((nv, nv), np.uint32),
                    patterns=np.zeros((n, 0), np.int16), group_counts=np.zeros(0, np.int64), n_candidates=0)
    padded = np.concatenate([rows, np.full((n, 3), 6, np.uint8)], axis=1)       # (only 'last_col' reads beyond the window)
    codes = np.stack([padded[:, pos + k] for k in range(3)], axis=2).astype(np.int64)   # [n][vp][3]
    gap, het, par = ((codes == s).any(axis=(1, 2)) for s in (4, 5, 6))
    damaged = gap | het | par
    clean = np.flatnonzero(~damaged)
    pat = 16 * (codes[:, :, 0] & 3) + 4 * (codes[:, :, 1] & 3) + (codes[:, :, 2] & 3)
    summary.update(damaged_reads=int(damaged.sum()), marginal_gap=int(gap.sum()), marginal_heteroduplex=int(het.sum()),
                   marginal_partial=int(par.sum()))
    in_key = np.ones(vp, dtype=bool)
    if wrong == "drop10th":
        in_key[POS_PER_WORD - 1::POS_PER_WORD] = False
    if wrong == "no_word1":
        in_key[POS_PER_WORD:2 * POS_PER_WORD] = False
    read_hap = np.full(n, HAP_DAMAGED, np.uint16)
    read_hap[clean] = HAP_INSUFFICIENT
    if len(clean):
        key = pat[clean][:, in_key]
        uniq, first, inverse, counts = np.unique(key, axis=0, return_index=True, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        group_pat = pat[clean][first]                          # the pattern of a group (of its first read, where the key is wrong)
    else:
        inverse, counts, group_pat = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, vp), np.int64)
    # count descending, then pattern ascending: the groups are in ascending pattern order already
    order = np.argsort(-counts, kind="stable")
    if wrong == "ties_reversed":
        order = np.argsort(-counts[::-1], kind="stable")
        order = len(counts) - 1 - order
    cand = counts[order] > min_reads if wrong == "gt" else counts[order] >= min_reads
    ranked = order[cand][:MAX_HAPLOTYPES]
    h = len(ranked)
    hap_of_group = np.full(len(counts), HAP_INSUFFICIENT, np.int64)
    hap_of_group[ranked] = np.arange(h)
    read_hap[clean] = hap_of_group[inverse].astype(np.uint16)
    hap_count = counts[ranked].astype(np.uint32)
    hap_pattern = group_pat[ranked].astype(np.uint8).reshape(h, vp)
    summary.update(reported_reads=int(hap_count.sum()), insufficient_reads=int(len(clean) - hap_count.sum()), n_haplotypes=h)
    hit = np.zeros((nv, h), np.uint8)
    for v in range(nv):
        if inside[v]:
            hit[v] = hap_pattern[:, np.searchsorted(pos, vcol[v])] == vcodon[v]
    cooc = ((hit.astype(np.int64) * hap_count.astype(np.int64)) @ hit.T.astype(np.int64)).astype(np.uint32)
    patterns = np.full((n, vp), -1, np.int16)
    patterns[clean] = pat[clean]
    return dict(summary=summary, pos_cols=pos.astype(np.uint32), hap_count=hap_count, hap_pattern=hap_pattern, hit=hit, read_hap=read_hap,
                cooc=cooc, patterns=patterns, group_counts=counts, n_candidates=int(cand.sum()))


def distinct_patterns_per_block(patterns):
    """Distinct patterns among the clean reads of every 2048-read block."""
    out = []
    for b in range(0, len(patterns), BLOCK_READS):
        p = patterns[b:b + BLOCK_READS]
        p = p[(p >= 0).all(axis=1)] if p.shape[1] else p[:0]
        out.append(len(np.unique(p, axis=0)))
    return out


# ------------------------------------------------------------------------------------------------ building blocks
def background(l):
    """The reference every designed matrix starts from: CGT repeated (codon 27 in frame, GTC = 45 and TCG = 54 out of frame)."""
    return np.array([1, 2, 3], dtype=np.uint8)[np.arange(l) % 3]


def ref_codon(c):
    b = background(c + 3)
    return 16 * int(b[c]) + 4 * int(b[c + 1]) + int(b[c + 2])


def variant_codon(p, c):
    """The variant codon of position p at column c: AAA at the first position of a key word, TTT at its last, else any other."""
    if p % POS_PER_WORD == 0:
        return 0
    if p % POS_PER_WORD == POS_PER_WORD - 1:
        return 63
    x = (7 * p + 3) % 64
    return x if x not in (ref_codon(c), 0, 63) else (x + 1) % 62 + 1


def put_codon(rows, sel, c, codon):
    codon = np.asarray(codon)
    rows[sel, c], rows[sel, c + 1], rows[sel, c + 2] = codon >> 4, (codon >> 2) & 3, codon & 3


def rows_of_groups(l, cols, groups, seed):
    """groups: [(pattern: a codon per position of cols, reads)] over non-overlapping columns -> rows in a seeded order."""
    pats = np.repeat(np.array([g[0] for g in groups], dtype=np.int64).reshape(len(groups), len(cols)), [g[1] for g in groups], axis=0)
    rows = np.tile(background(l), (len(pats), 1))
    for p, c in enumerate(cols):
        put_codon(rows, slice(None), c, pats[:, p])
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def table_of(pairs):
    """A host variant table from (col, codon) pairs, in the order of SPEC §6 for one gene in frame."""
    pairs = sorted(set((int(c), int(k)) for c, k in pairs))
    t = np.zeros(len(pairs), dtype=VARIANT)
    for i, (c, k) in enumerate(pairs):
        t[i]["col"], t[i]["codon"], t[i]["codon_pos"], t[i]["ref_codon"] = c, k, c // 3 + 1, ref_codon(c)
    return t


def observed_variants(rows, cols):
    """(col, codon) of every codon at the columns `cols` that some read carries whole and that is not the background's."""
    pairs = set()
    for c in cols:
        ok = (rows[:, c:c + 3] < 4).all(axis=1)
        codons = 16 * rows[ok, c].astype(np.int64) + 4 * rows[ok, c + 1] + rows[ok, c + 2]
        pairs |= {(c, int(k)) for k in np.unique(codons) if k != ref_codon(c)}
    return pairs


def damage(rows, cols, positions, first):
    """From read `first` on, one read for each of '-', N and not covered in each of the three columns of each position named."""
    i = first
    for p in positions:
        for k in range(3):
            for sym in (4, 5, 6):
                rows[i] = background(rows.shape[1])
                rows[i, cols[p] + k] = sym
                i += 1
    return i


# The cases that cannot go through the whole path (jl.run, group runs), and why.  Every other case does: with `called()`, the table
# the call stage gives for its matrix — which is the host table itself unless that holds rows no read carries or rows outside
# the window (those stay with the stage run: they must never hit).
NO_WHOLE_PATH = {
    "reads-1": "a window of one read: the call stage calls nothing, there is no position to phase",
    "vp11-overlap": "the overlapping codon starts out of frame: a gene in that frame would call every codon of it that a variant touches",
    "wide-131072": "the codon that ends in column 131071 starts out of frame; its rows sit on the plan kernel's two paths, which only a host table takes",
    "wide-131073": "the codon that ends in column 131071 starts out of frame; its rows sit on the plan kernel's two paths, which only a host table takes",
}
NO_GROUP = {"cand-4097": "the expected outcome is the overflow status, asserted on the stage API and the whole-path run"}


class Case:
    """name, the edge it sits on, build() -> (rows, host table), min_reads.  capacity: None, or the documented status of
    jl_phase_fetch the case expects.  called(): what the call stage gives for the matrix with one gene in frame over the window,
    the background as reference, alpha 0.9 and n_tests 1 — every codon an in-frame column carries that is not the background's."""

    def __init__(self, name, edge, build, min_reads=2, capacity=None, want=None):
        self.name, self.edge, self._build, self.min_reads, self.capacity = name, edge, build, min_reads, capacity
        self.want = want or {}
        self._built = None

    @property
    def whole_path(self):
        return self.name not in NO_WHOLE_PATH

    def called(self):
        rows = self.build()[0]
        return table_of(observed_variants(rows, range(0, rows.shape[1] - 2, 3)))

    def expected_run(self):
        return phase(self.build()[0], self.called(), self.min_reads)

    def build(self):
        if self._built is None:
            rows, table = self._build()
            self._built = (np.ascontiguousarray(rows, dtype=np.uint8), table)
        return self._built

    def drop(self):
        self._built = None

    def expected(self):
        rows, table = self.build()
        return phase(rows, table, self.min_reads)

    def genes(self):
        return np.array([(1, self.build()[0].shape[1] + 1)], dtype=GENE)

    def refseq(self):
        return background(self.build()[0].shape[1])


CASES = {}


def case(name, edge, **kw):
    def reg(build):
        assert name not in CASES
        CASES[name] = Case(name, edge, build, **kw)
        return build
    return reg


# ------------------------------------------------------------------------------------------------ position count
INTERESTING = (0, 9, 10, 19, 20, 29, 30)


def by_positions(vp, cols, l, others, seed, extra_pairs=(), same_col=None):
    """A window with a variant at each of vp positions: the reference group, one group per position that carries that position's
    variant alone (3..6 reads: many equal counts), groups that differ from another only in the first or last position of a key
    word, and a damaged read for every code and codon column at the first and last position of every word.  others: a read with
    a third codon that is no variant, at the first and the last position (insufficient at min_reads 2)."""
    if vp == 0:
        return np.tile(background(l), (100, 1)), table_of([])
    ref = [ref_codon(c) for c in cols]
    var = [variant_codon(p, c) for p, c in enumerate(cols)]
    groups = [(tuple(ref), 40)]
    for p in range(vp):
        g = list(ref)
        g[p] = var[p]
        groups.append((tuple(g), 3 + p % 4))
    marks = [p for p in INTERESTING if p < vp] + [vp - 1]
    if vp > 1:
        g = list(ref)
        for p in marks:
            g[p] = var[p]
        groups.append((tuple(g), 5))                     # every word edge at once
        for p in sorted(set(marks)):                     # ... and the same but for ONE word edge
            h = list(g)
            h[p] = ref[p]
            groups.append((tuple(h), 5))
    pairs = [(c, k) for c, k in zip(cols, var)]
    if same_col is not None:                             # two variants at one column: different codons
        g = list(ref)
        g[same_col] = 21 if var[same_col] != 21 else 22
        groups.append((tuple(g), 6))
        pairs.append((cols[same_col], g[same_col]))
    if others:
        for p in {0, vp - 1}:
            g = list(ref)
            g[p] = 38 if var[p] != 38 else 39            # GCG: neither the reference nor a variant
            groups.append((tuple(g), 1))
    seen = {}
    for g, k in groups:
        seen[g] = seen.get(g, 0) + k
    rows = rows_of_groups(l, cols, list(seen.items()), seed)
    dmg = sorted({p for p in (0, 9, 10, 19, 20, 29, 30, vp - 1) if p < vp})
    rows = np.concatenate([rows, np.tile(background(l), (9 * len(dmg), 1))])
    damage(rows, cols, dmg, len(rows) - 9 * len(dmg))
    return rows, table_of(pairs + list(extra_pairs))


for _vp in (0, 1, 10, 11, 20, 21, 30, 31, 41):
    def _b(vp=_vp):
        return by_positions(vp, [6 * i for i in range(vp)], 6 * max(vp, 1) + 4, False, 100 + vp, same_col=4 if vp == 10 else None)
    case("vp%d" % _vp, "%d positions, in frame from column 0%s" % (_vp, "; two variants at one column" if _vp == 10 else
         "; more than the four key words a whole-path run keeps" if _vp == 41 else ""), want=dict(vp=_vp))(_b)


@case("vp11-overlap", "11 positions, two of them overlapping codons at columns c and c + 1; a third codon that is no variant", want=dict(vp=11))
def _vp11_overlap():
    cols = [6 * i for i in range(10)]
    rows, table = by_positions(10, cols, 70, True, 211)
    # the overlapping codon at column 25 (24 is a position): reads that differ from the reference in column 27 alone change the
    # codon at 25 and not the one at 24
    sel = np.arange(0, len(rows), 5)
    sel = sel[(rows[sel, 24:28] < 4).all(axis=1)]
    rows[sel, 27] = 0
    codon25 = 16 * 2 + 4 * 3 + 0
    return rows, table_of([(r["col"], r["codon"]) for r in table] + [(25, codon25)])


@case("vp20-last", "20 positions, the last on the last valid codon (col = n_cols - 3); a row at col = n_cols - 2 that the plan ignores; "
      "a third codon that is no variant", want=dict(vp=20, ignored_rows=2))
def _vp20_last():
    l = 6 * 19 + 3
    cols = [6 * i for i in range(20)]
    assert cols[-1] == l - 3
    return by_positions(20, cols, l, True, 220, extra_pairs=[(l - 2, 9), (l - 1, 9)])


@case("vp21-last", "21 positions on the multi-word pipeline, the last on the last valid codon; a row at col = n_cols - 2", want=dict(vp=21, ignored_rows=1))
def _vp21_last():
    l = 6 * 20 + 3
    cols = [6 * i for i in range(20)] + [l - 3]
    return by_positions(21, cols, l, True, 221, extra_pairs=[(l - 2, 9)])


# ------------------------------------------------------------------------------------------------ read counts
READ_COUNTS = (1, 63, 64, 65, BLOCK_READS - 1, BLOCK_READS, BLOCK_READS + 1, 2 * BLOCK_READS + 1, INLINE_MAX_READS, INLINE_MAX_READS + 1)
READS_COLS, READS_L = (0, 6, 12), 16


def by_reads(n):
    """n reads over three positions: read i takes the pattern i % 16 names (both variants of position 0, the variants of 1 and 2
    and their combinations), every 97th read is damaged, the last read carries all three variants."""
    i = np.arange(n)
    rows = np.tile(background(READS_L), (n, 1))
    v = [variant_codon(p, c) for p, c in enumerate(READS_COLS)]
    put_codon(rows, i % 16 >= 10, 0, v[0])
    put_codon(rows, i % 16 == 9, 0, 21)
    put_codon(rows, i % 4 == 3, 6, v[1])
    put_codon(rows, i % 16 >= 14, 12, v[2])
    rows[(i % 97 == 5), 7] = 4
    rows[(i % 97 == 50), 13] = 6
    put_codon(rows, i == n - 1, 0, v[0]), put_codon(rows, i == n - 1, 6, v[1]), put_codon(rows, i == n - 1, 12, v[2])
    return rows, table_of(observed_variants(rows, READS_COLS))


for _n in READ_COUNTS:
    def _b(n=_n):
        return by_reads(n)
    _blocks = grid_blocks(_n)
    case("reads-%d" % _n, "%d reads: %d workgroup(s) of the fused launch, ids %s" % (_n, _blocks, "inline" if _blocks <= INLINE_IDS_MAX_BLOCKS else
         "by the separate launch"), min_reads=1 if _n == 1 else 2, want=dict(blocks=_blocks))(_b)


# ------------------------------------------------------------------------------------------------ the grouping table
BASE_CODON = 21    # CCC: what the positions that do not vary carry in every read, so that the call stage makes positions of them
def by_distinct(vp, vary, distinct, tail, seed_variants=20):
    """Block 0 (2048 reads) holds exactly `distinct` patterns: its first `distinct` reads one each (they differ in the two positions
    `vary`, base 64; every other position carries CCC in every read), the rest go round the first three; `tail` more reads in a
    second block repeat patterns of the first one each, so that at min_reads 2 about half of the small groups are reported —
    a read that took the way round a full table must come out with its group's id."""
    cols = [3 * i for i in range(vp)]
    l = 3 * vp + 2
    n = BLOCK_READS + tail
    i = np.arange(n)
    d = np.where(i < distinct, i, i % 3)
    d = np.where(i >= BLOCK_READS, (i * 7) % distinct, d)
    rows = np.tile(background(l), (n, 1))
    for c in cols:
        put_codon(rows, slice(None), c, BASE_CODON)
    put_codon(rows, slice(None), cols[vary[0]], d // 64)
    put_codon(rows, slice(None), cols[vary[1]], d % 64)
    pairs = [(cols[vary[0]], k) for k in range(seed_variants // 2)] + [(cols[vary[1]], k) for k in range(seed_variants // 2)]
    pairs += [(c, BASE_CODON) for c in cols] + [(c, variant_codon(p, c)) for p, c in enumerate(cols)]
    return rows, table_of(p for p in pairs if p[1] != ref_codon(p[0]))


# the first clean read's pattern is kept apart from the table (the block's dominant key): 1 + 1024 patterns fill it, the 1026th spills
for _d in (LDS_SLOTS, LDS_SLOTS + 1, LDS_SLOTS + 2):
    def _b(d=_d):
        return by_distinct(2, (0, 1), d, 600)
    case("lds-%d" % _d, "%d distinct patterns in one block of the one-word launch (its table holds %d besides the dominant pattern)" % (_d, LDS_SLOTS),
         want=dict(vp=2, distinct0=_d))(_b)
for _name, _vary, _what in (("w1", (18, 19), "agree in word 0, differ only in word 1"), ("w0", (8, 9), "agree in word 1, differ only in word 0")):
    def _b(vary=_vary):
        return by_distinct(20, vary, LDS_SLOTS + 2, 120)   # (no more candidates than the two-word launch selects itself: 123)
    case("lds-1026-" + _name, "1026 distinct patterns in one block of the two-word launch that " + _what,
         want=dict(vp=20, distinct0=LDS_SLOTS + 2, vary=_vary))(_b)


@case("w1-last", "20 positions, 40 patterns that differ only in the last position of the second key word", want=dict(vp=20, vary=(19, 19)))
def _w1_last():
    cols = [3 * i for i in range(20)]
    groups = [(tuple([BASE_CODON] * 19 + [k]), 2 + k % 5) for k in range(40)]
    rows = rows_of_groups(62, cols, groups, 77)
    return rows, table_of([(c, variant_codon(p, c)) for p, c in enumerate(cols)] + [(c, BASE_CODON) for c in cols] + [(cols[19], k) for k in (0, 1, 2, 39)])


# ------------------------------------------------------------------------------------------------ selection
for _m in (1, 2, 10):
    def _b(m=_m):
        cols = [0, 3]
        groups = [((27, 27), 30), ((5, 27), m), ((27, 5), m + 1)] + ([((5, 5), m - 1)] if m > 1 else [])
        return rows_of_groups(8, cols, groups, 300 + m), table_of([(0, 5), (3, 5)])
    case("minreads-%d" % _m, "a group of exactly min_reads = %d reads beside one of %d" % (_m, _m - 1), min_reads=_m,
         want=dict(vp=2, at_threshold=_m))(_b)


@case("ties", "six groups of 5 reads and two of 7 over 20 positions: equal counts go by pattern, decided in word 0 and in word 1",
      want=dict(vp=20, ties=True))
def _ties():
    cols = [3 * i for i in range(20)]
    def g(**at):
        p = [BASE_CODON] * 20
        for k, v in at.items():
            p[int(k[1:])] = v
        return tuple(p)
    groups = [(g(), 5), (g(p0=0), 5), (g(p9=63), 5), (g(p10=0), 5), (g(p19=63), 5), (g(p19=26), 5), (g(p0=63, p19=0), 7), (g(p0=63, p19=63), 7)]
    rows = rows_of_groups(62, cols, groups, 55)
    return rows, table_of([(c, variant_codon(p, c)) for p, c in enumerate(cols)] + [(c, BASE_CODON) for c in cols] + [(0, 63), (57, 0), (57, 26)])


def by_haplotypes(h, vp, count_of, singles, seed):
    """h qualifying groups (group k has count_of(k) >= 2 reads) and `singles` groups of one read, min_reads 2."""
    cols = [3 * i for i in range(vp)]

    def pattern(k):   # base 64 over the positions, never the all-reference pattern twice
        return tuple((k >> (6 * (vp - 1 - p))) & 63 for p in range(vp))
    groups = [(pattern(k), count_of(k)) for k in range(h)] + [(pattern(h + k), 1) for k in range(singles)]
    rows = rows_of_groups(3 * vp + 1, cols, groups, seed)
    return rows, table_of([(c, k) for c in cols for k in (0, 1, 2, 63) if k != ref_codon(c)] + [(cols[-1], 40)])


for _h, _why in ((ID4_MAX_H, "the most haplotypes 4-bit ids hold"), (ID4_MAX_H + 1, "one more than 4-bit ids hold"),
                 (PACK_MAX_HAP, "the most candidates the selection out of LDS ranks"), (PACK_MAX_HAP + 1, "one candidate more than the selection out of LDS ranks"),
                 (ID8_MAX_H, "the most haplotypes 8-bit ids hold"), (ID8_MAX_H + 1, "one more than 8-bit ids hold"),
                 (MAX_HAPLOTYPES, "the most haplotypes that have names")):
    def _b(h=_h):
        return by_haplotypes(h, 2, lambda k: 2 + k % 3, 5, 400 + h)
    case("haps-%d" % _h, "%d qualifying groups: %s" % (_h, _why), want=dict(vp=2, haplotypes=_h, candidates=_h))(_b)


# the two-word launch has no general selection behind it: a result beyond the selection out of LDS hands the context to the multi-word pipeline
for _h, _form in ((PACK_MAX_HAP, FORM_TWO), (PACK_MAX_HAP + 1, FORM_MULTI)):
    def _b(h=_h):
        return by_haplotypes(h, 11, lambda k: 2 + k % 3, 5, 900 + h)
    case("haps2w-%d" % _h, "%d qualifying groups over 11 positions: the two-word launch %s" % (_h, "selects them itself" if _form == FORM_TWO else
         "hands the run to the multi-word pipeline"), want=dict(vp=11, haplotypes=_h, candidates=_h, form=_form))(_b)


@case("haps-703", "703 qualifying groups: one more than have names; the 703rd in the documented order joins the insufficient reads",
      want=dict(vp=2, haplotypes=MAX_HAPLOTYPES, candidates=MAX_HAPLOTYPES + 1))
def _haps_703():
    return by_haplotypes(MAX_HAPLOTYPES + 1, 2, lambda k: 2 + k % 3, 5, 1103)


def _cand(n_cand):
    # 702 groups of 3 reads are the haplotypes whatever becomes of the groups of 2
    return by_haplotypes(n_cand, 3, lambda k: 3 if k % 5 == 0 and k < 5 * MAX_HAPLOTYPES else 2, 7, 5000 + n_cand)


@case("cand-4096", "4096 candidates: all the selector ranks", want=dict(vp=3, haplotypes=MAX_HAPLOTYPES, candidates=CAND_CAP))
def _cand_4096():
    return _cand(CAND_CAP)


@case("cand-4097", "4097 candidates: one more than the selector ranks; jl_phase_fetch returns JL_ERR_OVERFLOW", capacity=ERR_OVERFLOW,
      want=dict(vp=3, haplotypes=MAX_HAPLOTYPES, candidates=CAND_CAP + 1))
def _cand_4097():
    return _cand(CAND_CAP + 1)


# ------------------------------------------------------------------------------------------------ the plan's two paths
def by_width(l):
    """64 reads over l columns; rows at the first codon, at a codon across the 65536-column seam, at the codon that ends in column
    131071, at the last valid codon and at col = n_cols - 2."""
    cols = sorted({0, 65535, PLAN_LDS_COLS - 3, l - 3})
    n = 64
    rows = np.tile(background(l), (n, 1))
    i = np.arange(n)
    for p, c in enumerate(cols):
        rows[i % (p + 2) == 0, c + 1] = 0             # overlapping codons (131069, 131070) each see the other's change
    rows[5, 0], rows[6, 65536], rows[7, l - 1] = 4, 5, 6
    return rows, table_of(list(observed_variants(rows, cols)) + [(l - 2, 9)])


for _l in (PLAN_LDS_COLS, PLAN_LDS_COLS + 1):
    def _b(l=_l):
        return by_width(l)
    case("wide-%d" % _l, "%d columns: the plan %s" % (_l, "marks its columns in LDS" if _l <= PLAN_LDS_COLS else "takes the path through HBM"),
         want=dict(vp=3 if _l == PLAN_LDS_COLS else 4, ignored_rows=1, cols=_l))(_b)

WIDE = [n for n in CASES if n.startswith("wide-")]


# ------------------------------------------------------------------------------------------------ the windows beside a case in a group run
def plain(l, n=1500):
    """A window without variants: every read is the background."""
    return np.tile(background(l), (n, 1))


def companion(l, n):
    """A different window of the same width whose table is what the call stage gives for it: two variants at column 0, one at
    column 3, every 97th read damaged."""
    i = np.arange(n)
    rows = np.tile(background(l), (n, 1))
    put_codon(rows, i % 4 == 1, 0, 0)
    put_codon(rows, i % 16 == 2, 0, 21)
    put_codon(rows, i % 8 >= 6, 3, 63)
    rows[i % 97 == 11, 4] = 4
    return rows, table_of(observed_variants(rows, (0, 3)))


COMPANION_READS = 3000                      # with it a small case's launch writes its ids itself ...
COMPANION_DEEP = INLINE_MAX_READS + 1       # ... and with this one no launch of the group does

# "the form only grows": one context phases these in order; a fresh one starts with the last but one
GROWTH = ("vp10", "vp11", "vp21", "vp10")
GROWTH_FORMS = (FORM_ONE, FORM_TWO, FORM_MULTI, FORM_MULTI)
GROWTH_FRESH = "vp21"

# what one child process of tests/test_gpu_phase_edges.py runs (a part uploads a handful of small windows)
PARTS = {
    "positions": [n for n in CASES if n.startswith("vp")],
    "reads": [n for n in CASES if n.startswith("reads-")],
    "table": [n for n in CASES if n.startswith(("lds-", "w1-"))],
    "selection": [n for n in CASES if n.startswith(("minreads-", "ties", "haps"))],
    "capacity": [n for n in CASES if n.startswith("cand-")],
    "wide": WIDE,
}
assert sorted(n for p in PARTS.values() for n in p) == sorted(CASES)
