"""Designed cases for cross-window phasing with the reads sharded (test infrastructure, like phase_edges.py; nothing of the product
imports it and it shares no code with oracle/).

The route (kernels_xwin.hip, capi_xwin.hip, capi_merge.hip, xwin_schedule.h, the exporting phase run and jl_phase_regroup) has its
edges where a slice's last byte, 16-byte piece and 16 KiB x-block end, where the pack launch is cut into chunks of positions and of
destinations, where the merge changes its comparison (8 / 9 positions), where a group reaches min_reads only as a sum over slices,
where the ids change their width on the MERGED haplotype count, and where the session's blocks and tables end.  This module states
in plain numpy what the pack launch must write (pack_expected), what one slice exports (slice_groups) and what merge + selection
give (sharded); the expected result of every route is phase_edges.phase on the whole matrix.

Symbols as everywhere: A C G T = 0..3, '-' = 4, N = 5, not covered = 6."""
import numpy as np

import phase_edges as pe
from minorseq_amd import sharding

# ------------------------------------------------------------------------------------------------ the constants, mirrored
# (tests/test_xwin_edges_host.py compares each with the line it mirrors)
POS_MAX = 48                        # jl_internal.h: #define JL_XW_POS_MAX 48u    (owned positions per pack launch)
DST_MAX = 8                         # jl_internal.h: #define JL_XW_DST_MAX 8u     (destination ranks per pack launch)
TAB_MAX = 1024                      # jl_internal.h: #define JL_XW_TAB_MAX 1024u  (exported groups whose haplotypes travel by value)
GCAP0 = 1024                        # capi_xwin.hip: #define JL_XW_GCAP0 1024u    (groups a rank's export block holds before it grows)
XROWS0 = 256                        # capi_xwin.hip: #define JL_XW_XROWS0 256u    (variant rows a rank's table block holds before it grows)
PACK_PIECES = 4                     # kernels_xwin.hip: constexpr uint32_t kPackPieces = 4
XBLOCK_BYTES = PACK_PIECES * 256 * 16   # kernels_xwin.hip: off = ((blockIdx.x * kPackPieces + k) * 256 + threadIdx.x) * 16 -> 16384 a block
XBLOCK_READS = 8 * XBLOCK_BYTES     # 131072 reads of a plane row per x-block
PIECE_READS = 8 * 16                # a 16-byte piece = 128 reads
SLICE_ALIGN = 256                   # xwin_schedule.h: slice_begin[s] & 255u (a slice starts on a multiple of 256 reads)
LINE_READS = 1024                   # xwin_schedule.h xwin_stride: (n_reads + 1023) / 1024 * 128 bytes
MERGE_WORD_MAX = 8                  # capi_merge.hip jl_merge_groups: const bool by_word = vp <= 8u
ERR_ARG = -1                        # include/juliet_hip.h: JL_ERR_ARG
UNWRITTEN = 7                       # what the mirrors of wrong kernels put where a kernel would store nothing (no code is 7)

PACK_WRONG = ("no_tail_mask", "pad_zero_all_planes", "leak_past_slice", "drop_xblock1", "pos_chunk_offset", "dst_chunk_offset",
              "line_tail_not_padded")
MERGE_WRONG = ("word_compare_past_8", "threshold_before_merge", "ties_by_table_order", "cap_701", "ids_4bit_at_15", "ids_8bit_at_255")


def stride_reads(n_reads):
    """Reads a plane row of a compact matrix of n_reads reads holds (xwin_stride: whole 128-byte lines)."""
    return -(-n_reads // LINE_READS) * LINE_READS


def shown_reads(n_reads):
    """Reads per column the interchange format of a download shows (jl_col_stride: 128-byte lines of nibbles = 256 reads)."""
    return -(-n_reads // 256) * 256


# ------------------------------------------------------------------------------------------------ the pack launch
def pack_expected(rows, pos_cols, read_begin, n_slice, stride_reads, wrong=None, dst=0, slices=None):
    """The compact matrix the pack launch writes for one destination, as rows uint8[stride_reads][3 vp]: position k's three columns
    sit at 3k..3k+2, reads read_begin..read_begin+n_slice of `rows` are copied, every cell past the slice is 6.

    wrong: one of the wrong kernels the shapes must tell from the right one (PACK_WRONG) — 'no_tail_mask' (the bits of the last
    byte that are no reads of the slice keep the source's), 'pad_zero_all_planes' (0x00 in planes 1 and 2 too: code 0),
    'leak_past_slice' (the row is copied up to the stride), 'drop_xblock1' (blockIdx.x >= 1 stores nothing), 'pos_chunk_offset'
    (the second chunk of positions lands on the first), 'dst_chunk_offset' (the second chunk of destinations lands on the first:
    destination `dst` of `slices` = [(begin, reads)]), 'line_tail_not_padded' (the pieces past the slice's last are not stored)."""
    rows = np.asarray(rows, dtype=np.uint8)
    n = rows.shape[0]
    vp = len(pos_cols)
    cols = np.concatenate([np.arange(c, c + 3) for c in pos_cols]).astype(np.int64) if vp else np.zeros(0, np.int64)
    src = np.full((max(stride_reads, n_slice) + LINE_READS, 3 * vp), 6, np.uint8)     # the source row from read_begin on, with its own padding
    avail = max(0, min(n - read_begin, len(src)))
    src[:avail] = rows[read_begin:read_begin + avail][:, cols]
    out = np.full((stride_reads, 3 * vp), 6, np.uint8)
    out[:n_slice] = src[:n_slice]
    if wrong == "no_tail_mask":
        out[n_slice:-(-n_slice // 8) * 8] = src[n_slice:-(-n_slice // 8) * 8]
    elif wrong == "pad_zero_all_planes":
        out[n_slice:] = 0
    elif wrong == "leak_past_slice":
        out[n_slice:] = src[n_slice:stride_reads]
    elif wrong == "drop_xblock1":
        out[XBLOCK_READS:] = UNWRITTEN
    elif wrong == "pos_chunk_offset":
        if vp > POS_MAX:
            out[:, :3 * (vp - POS_MAX)] = out[:, 3 * POS_MAX:].copy()
            out[:, 3 * POS_MAX:] = UNWRITTEN
    elif wrong == "dst_chunk_offset":
        if dst >= DST_MAX:
            out[:] = UNWRITTEN
        elif slices is not None and dst + DST_MAX < len(slices):
            b, k = slices[dst + DST_MAX]
            out[:] = pack_expected(rows, pos_cols, b, k, max(stride_reads, -(-k // LINE_READS) * LINE_READS))[:stride_reads]
    elif wrong == "line_tail_not_padded":
        out[-(-n_slice // PIECE_READS) * PIECE_READS:] = UNWRITTEN
    else:
        assert wrong is None, wrong
    return out


def positions_of(table, n_cols):
    """The distinct columns of the table's rows whose codon lies inside the n_cols columns, ascending."""
    col = np.asarray(table["col"], dtype=np.int64)
    return np.unique(col[col + 2 < n_cols])


def slice_groups(rows, table, begin, end):
    """What the exporting phase run of reads [begin, end) gives: `patterns` uint8[G][Vp] of the clean reads, ascending, their
    `counts`, the slice's `summary` (damaged reads and the three marginals; the clean reads are all insufficient until the merge)
    and `index` int64[end - begin]: each read's group (-1: damaged)."""
    rows = np.asarray(rows, dtype=np.uint8)[begin:end]
    pos = positions_of(table, rows.shape[1])
    vp = len(pos)
    codes = np.stack([rows[:, pos + k] for k in range(3)], axis=2).astype(np.int64).reshape(len(rows), vp, 3)
    gap, het, par = ((codes == s).any(axis=(1, 2)) for s in (4, 5, 6))
    damaged = gap | het | par
    pat = (16 * (codes[:, :, 0] & 3) + 4 * (codes[:, :, 1] & 3) + (codes[:, :, 2] & 3)).astype(np.uint8)
    index = np.full(len(rows), -1, np.int64)
    clean = np.flatnonzero(~damaged)
    if len(clean) and vp:
        uniq, inverse, counts = np.unique(pat[clean], axis=0, return_inverse=True, return_counts=True)
        index[clean] = inverse.reshape(-1)
    else:
        uniq, counts = np.zeros((0, vp), np.uint8), np.zeros(0, np.int64)
    summary = dict.fromkeys(pe.SUMMARY_FIELDS, 0)
    summary.update(damaged_reads=int(damaged.sum()), marginal_gap=int(gap.sum()), marginal_heteroduplex=int(het.sum()),
                   marginal_partial=int(par.sum()), insufficient_reads=int(len(clean)), n_positions=vp)
    return dict(patterns=uniq.astype(np.uint8).reshape(len(counts), vp), counts=counts.astype(np.uint32), summary=summary, index=index,
                pos_cols=pos.astype(np.uint32))


# ------------------------------------------------------------------------------------------------ merge, selection and ids
def sharded(rows, table, min_reads, bounds, wrong=None):
    """Merge and selection over the slices [bounds[s], bounds[s + 1]) in plain numpy: the fields of phase_edges.phase (summary,
    hap_count, hap_pattern, hit, cooc, read_hap) and `id_bits`.  With wrong=None this is phase_edges.phase of the whole matrix
    (tests/test_xwin_edges_host.py asserts it); wrong: MERGE_WRONG — 'word_compare_past_8' (patterns of more than 8 positions
    compared by their first 8), 'threshold_before_merge' (min_reads applied to a slice's count), 'ties_by_table_order' (equal
    merged counts in the order the groups first appear: slice, then row), 'cap_701', 'ids_4bit_at_15' / 'ids_8bit_at_255' (the
    narrower ids one haplotype too far: its reads read as insufficient)."""
    rows = np.asarray(rows, dtype=np.uint8)
    l = rows.shape[1]
    tabs = [slice_groups(rows, table, bounds[s], bounds[s + 1]) for s in range(len(bounds) - 1)]
    vp = tabs[0]["summary"]["n_positions"]
    pats = np.concatenate([t["patterns"].reshape(-1, vp) for t in tabs]).astype(np.int64)
    cnts = np.concatenate([t["counts"] for t in tabs]).astype(np.int64)
    first = np.arange(len(cnts))                                      # (slice, row) order of appearance
    if wrong == "threshold_before_merge":
        cnts = np.where(cnts >= min_reads, cnts, 0)
    key = pats[:, :MERGE_WORD_MAX] if wrong == "word_compare_past_8" else pats
    if len(cnts):
        _, rep, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
        mcount = np.bincount(inverse, weights=cnts, minlength=len(rep)).astype(np.int64)
        mpat = pats[rep]
        mfirst = np.full(len(rep), len(cnts), np.int64)
        np.minimum.at(mfirst, inverse, first)
    else:
        inverse, mcount, mpat, mfirst = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, vp), np.int64), np.zeros(0, np.int64)
    order = np.argsort(-mcount, kind="stable")                        # merged groups are in ascending pattern order already
    if wrong == "ties_by_table_order":
        order = np.lexsort((mfirst, -mcount))
    ranked = order[mcount[order] >= min_reads][:pe.MAX_HAPLOTYPES - 1 if wrong == "cap_701" else pe.MAX_HAPLOTYPES]
    h = len(ranked)
    hap_of_merged = np.full(len(mcount), pe.HAP_INSUFFICIENT, np.int64)
    hap_of_merged[ranked] = np.arange(h)
    summary = dict.fromkeys(pe.SUMMARY_FIELDS, 0)
    for t in tabs:
        for f in ("damaged_reads", "marginal_gap", "marginal_heteroduplex", "marginal_partial"):
            summary[f] += t["summary"][f]
    clean = sum(t["summary"]["insufficient_reads"] for t in tabs)
    hap_count = mcount[ranked].astype(np.uint32)
    summary.update(reported_reads=int(hap_count.sum()), insufficient_reads=int(clean - hap_count.sum()), n_positions=vp, n_haplotypes=h)
    hap_pattern = mpat[ranked].astype(np.uint8).reshape(h, vp)
    pos = positions_of(table, l)
    nv = len(table)
    hit = np.zeros((nv, h), np.uint8)
    for v in range(nv):
        if int(table["col"][v]) + 2 < l:
            hit[v] = hap_pattern[:, np.searchsorted(pos, table["col"][v])] == table["codon"][v]
    cooc = ((hit.astype(np.int64) * hap_count.astype(np.int64)) @ hit.T.astype(np.int64)).astype(np.uint32)
    bits = pe.id_bits(h, vp)
    if wrong == "ids_4bit_at_15" and vp and h == pe.ID4_MAX_H + 1:
        bits = 4
    if wrong == "ids_8bit_at_255" and vp and h == pe.ID8_MAX_H + 1:
        bits = 8
    read_hap = np.full(len(rows), pe.HAP_DAMAGED, np.uint16)
    off = 0
    for s, t in enumerate(tabs):
        g = np.full(bounds[s + 1] - bounds[s], pe.HAP_DAMAGED, np.int64)
        ok = t["index"] >= 0
        g[ok] = hap_of_merged[inverse[off + t["index"][ok]]]
        off += len(t["counts"])
        read_hap[bounds[s]:bounds[s + 1]] = g.astype(np.uint16)
    if bits < 16:                                                     # the two top values of a narrow id are the two categories
        read_hap[read_hap == (1 << bits) - 2] = pe.HAP_INSUFFICIENT
    return dict(summary=summary, pos_cols=pos.astype(np.uint32), hap_count=hap_count, hap_pattern=hap_pattern, hit=hit, cooc=cooc,
                read_hap=read_hap, id_bits=bits, n_merged=len(mcount))


# ------------------------------------------------------------------------------------------------ the cases
class XCase:
    """A phase_edges case or a new one: build() -> (rows, host table with every row inside the window), min_reads, and the table
    the call stage gives (called())."""

    def __init__(self, name, edge, build, min_reads=2, whole_path=True):
        self.name, self.edge, self._build, self.min_reads, self.whole_path = name, edge, build, min_reads, whole_path
        self._built = None

    def build(self):
        if self._built is None:
            rows, table = self._build()
            rows = np.ascontiguousarray(rows, dtype=np.uint8)
            self._built = (rows, table[table["col"].astype(np.int64) + 2 < rows.shape[1]])   # a row outside every window is refused here
        return self._built

    def called(self):
        rows = self.build()[0]
        return pe.table_of(pe.observed_variants(rows, range(0, rows.shape[1] - 2, 3)))


REUSED = ("vp1", "vp10", "vp11", "vp20", "vp21", "vp30", "vp31", "vp41", "vp20-last", "minreads-1", "minreads-2", "minreads-10", "ties",
          "haps-14", "haps-15", "haps-254", "haps-255", "haps-702", "haps-703", "lds-1024", "lds-1025", "lds-1026", "w1-last")
HOST_TABLE_ONLY = ("vp11-overlap",)      # overlapping codons: no call stage gives that table (phase_edges.NO_WHOLE_PATH)
CASES = {}
for _n in REUSED + HOST_TABLE_ONLY:
    _c = pe.CASES[_n]
    CASES[_n] = XCase(_n, _c.edge, _c._build, _c.min_reads, whole_path=_n not in HOST_TABLE_ONLY)


def _new(name, edge, **kw):
    def reg(build):
        assert name not in CASES
        CASES[name] = XCase(name, edge, build, **kw)
        return build
    return reg


for _vp in (MERGE_WORD_MAX, MERGE_WORD_MAX + 1):
    def _b(vp=_vp):
        return pe.by_positions(vp, [6 * i for i in range(vp)], 6 * vp + 4, False, 100 + vp)
    _new("vp%d" % _vp, "%d positions: jl_merge_groups compares patterns %s" % (_vp, "as one big-endian word" if _vp <= MERGE_WORD_MAX else "by memcmp"))(_b)

SPLIT_MIN = 6


@_new("split-minreads", "a group of exactly min_reads = 6 reads, two in each of three slices of 256, beside one of 5", min_reads=SPLIT_MIN)
def _split_minreads():
    n, cols = 3 * 256, [0, 3]
    rows = np.tile(pe.background(8), (n, 1))
    for s in range(3):
        pe.put_codon(rows, slice(256 * s + 10, 256 * s + 12), 0, 5)            # (5, 27): 2 + 2 + 2 = 6 reads
        pe.put_codon(rows, slice(256 * s + 20, 256 * s + 22 - (s == 2)), 3, 5)  # (27, 5): 2 + 2 + 1 = 5 reads
    return rows, pe.table_of([(c, 5) for c in cols])


@_new("split-ties", "three groups whose counts are equal (9) only after the merge, the pattern order against the order of appearance")
def _split_ties():
    n = 3 * 256
    rows = np.tile(pe.background(8), (n, 1))
    # patterns A < B < C; a slice's table is in pattern order, so the order of appearance runs against it only across slices:
    # slice 0 holds C alone (5 reads), slice 1 B (6) and C (4), slice 2 A (9) and B (3)
    plan = {0: [(63, 5)], 1: [(21, 6), (63, 4)], 2: [(5, 9), (21, 3)]}
    for s, groups in plan.items():
        i = 256 * s + 7
        for codon, k in groups:
            pe.put_codon(rows, slice(i, i + k), 0, codon)
            i += k
    return rows, pe.table_of([(0, 5), (0, 21), (0, 63), (3, 5)])


def _many_positions(vp, n=300):
    """vp positions three columns apart: position p's variant in the reads i with i % vp == p, and in every 7th read at p + 1 too."""
    cols = [3 * p for p in range(vp)]
    l = 3 * vp + 1
    rows = np.tile(pe.background(l), (n, 1))
    i = np.arange(n)
    for p, c in enumerate(cols):
        pe.put_codon(rows, (i % vp == p) | ((i % 7 == 0) & (i % vp == (p + 1) % vp)), c, 0 if p % 2 else 63)
    rows[5, 1], rows[n - 3, l - 2] = 4, 5
    return rows, pe.table_of(pe.observed_variants(rows, cols))


for _vp in (POS_MAX, POS_MAX + 1):
    def _b(vp=_vp):
        return _many_positions(vp)
    _new("pos-%d" % _vp, "%d positions owned by one rank: %s" % (_vp, "one pack launch" if _vp <= POS_MAX else "a second chunk of positions"))(_b)


def _many_rows(n_rows, n=400):
    """n_rows called variant rows: three variant codons at each position (every read carries one of four codons there)."""
    vp = -(-n_rows // 3)
    cols = [3 * p for p in range(vp)]
    l = 3 * vp + 1
    rows = np.tile(pe.background(l), (n, 1))
    i = np.arange(n)
    k = 0
    for p, c in enumerate(cols):
        for j, codon in enumerate((0, 21, 63)):
            if k < n_rows:
                pe.put_codon(rows, i % 40 == (3 * p + j) % 40, c, codon)
                k += 1
    return rows, pe.table_of(pe.observed_variants(rows, cols))


for _r in (XROWS0, XROWS0 + 1):
    def _b(r=_r):
        return _many_rows(r)
    _new("rows-%d" % _r, "%d called variant rows on one rank: %s" % (_r, "a table block holds them" if _r <= XROWS0 else "the table blocks grow and gather again"))(_b)

SELECTION = [n for n in CASES if n.startswith(("minreads-", "ties", "split-", "haps-"))]
POSITIONS = [n for n in CASES if n.startswith(("vp", "w1-", "pos-"))]
TABLES = [n for n in CASES if n.startswith(("lds-", "rows-"))]
assert sorted(SELECTION + POSITIONS + TABLES) == sorted(CASES)


# ------------------------------------------------------------------------------------------------ a case over slices and windows
def window_cuts(n_cols, pos_cols, n_windows):
    """[(begin, n_cols)] of n_windows non-overlapping windows: the cuts are multiples of 3 and no position straddles one."""
    cuts = [0]
    for w in range(1, n_windows):
        c = max(cuts[-1] + 3, n_cols * w // n_windows // 3 * 3)
        while any(p < c < p + 3 for p in pos_cols):
            c += 3
        cuts.append(min(c, n_cols))
    cuts.append(n_cols)
    assert all(c % 3 == 0 for c in cuts[:-1]) and cuts == sorted(cuts)
    assert not any(p < c < p + 3 for p in pos_cols for c in cuts), "a position straddles a cut"
    return [(cuts[w], cuts[w + 1] - cuts[w]) for w in range(n_windows) if cuts[w + 1] > cuts[w]]


class Spread:
    """A case spread over n_slices slices: padded to at least 256 (n_slices - 1) + 1 reads, the reads in a seeded order so that groups
    straddle slices (the split-* cases place their reads in slices themselves and keep their order).  The padding is reads that cover
    no column (code 6): reads of the background would be a group of their own, one haplotype more than haps-14 or haps-254 are
    named for; reads that cover nothing join no group and call no variant, they count as damaged (partial) and nothing else."""

    def __init__(self, case, n_slices, seed=0, table=None, n_min=0, bounds=None, min_cols=0):
        rows, host = case.build()
        if min_cols > rows.shape[1]:           # more columns of the background behind the case's: room for a window per rank
            rows = np.concatenate([rows, np.tile(pe.background(min_cols)[rows.shape[1]:], (len(rows), 1))], axis=1)
        self.case, self.table, self.min_reads = case, host if table is None else table, case.min_reads
        n = max(len(rows), 256 * (n_slices - 1) + 1, n_min)
        rows = np.concatenate([rows, np.full((n - len(rows), rows.shape[1]), 6, np.uint8)])
        if not case.name.startswith("split-"):
            rows = rows[np.random.default_rng(1000 * n_slices + seed).permutation(n)]
        self.rows = np.ascontiguousarray(rows)
        self.bounds = sharding.read_slices(n, n_slices) if bounds is None else list(bounds)
        assert self.bounds[0] == 0 and self.bounds[-1] == n and len(self.bounds) == n_slices + 1
        self.n_slices = n_slices
        self._exp = None

    def expected(self):
        if self._exp is None:
            self._exp = pe.phase(self.rows, self.table, self.min_reads)
        return self._exp

    def windows(self, n_windows=None):
        l = self.rows.shape[1]
        return window_cuts(l, positions_of(self.table, l).tolist(), n_windows or (2 if l < 12 else 3))


def spread(case, n_slices, seed=0, table=None, n_min=0, bounds=None, min_cols=0):
    return Spread(case, n_slices, seed, table, n_min, bounds, min_cols)


# ------------------------------------------------------------------------------------------------ the shapes of the pack checks
PACK_COLS, PACK_POS = 24, (3, 9, 15)       # two windows of 12 columns: positions 3 and 9 in the first (9 ends on its last column), 15 in the second
PACK_WINDOWS = ((0, 12), (12, 12))
PACK_SMALL = (1, 7, 8, 9, 121, 127, 128, 129, 1023, 1024, 1025)
PACK_MORE = (10, 115, 1020, 125, 126)            # the values of n & 7 and the byte count (15 mod 16) that PACK_SMALL leaves out
PACK_BIG = (XBLOCK_READS, XBLOCK_READS + 1, XBLOCK_READS + 8, XBLOCK_READS + 9, 2 * XBLOCK_READS + 777)
PACK_BEHIND = 300                           # reads behind a slice that ends mid-matrix


def pack_rows(n, seed=7):
    """n reads over PACK_COLS columns: column c carries one of two bases in a read (512 patterns over the three positions), about
    one cell in sixty is '-', N or not covered; no two neighbouring reads are alike for long."""
    rng = np.random.default_rng(seed)
    rows = ((np.arange(PACK_COLS) + rng.integers(0, 2, (n, PACK_COLS))) % 4).astype(np.uint8)
    bad = rng.integers(0, 180, (n, PACK_COLS))
    for sym in (4, 5, 6):
        rows[bad == sym] = sym
    return rows


def pack_table():
    return pe.table_of([(c, k) for c in PACK_POS for k in (0, 21, 27, 63)])


def pack_slices(n_slice):
    """(read_begin, n_slice, n_reads of the matrix) of the four runs of a shape: from read 0 and from a multiple of 256, ending at
    the matrix's last read and ending mid-matrix with other reads behind."""
    b = 256 * (3 if n_slice < 4096 else 1)
    return [(0, n_slice, n_slice), (b, n_slice, b + n_slice), (0, n_slice, b + n_slice + PACK_BEHIND), (b, n_slice, b + n_slice + PACK_BEHIND)]
