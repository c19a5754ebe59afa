"""Designed windows for the pileup kernels (test infrastructure, like call_edges.py; nothing of the product imports it).

The bit-plane pileup (minorseq_amd/csrc/kernels_pileup.hip) has its edges where a tile of reads ends, where a flush batch of the
packed 16-bit counters ends, where the load width of a single run changes, and where a chunk of columns is narrower than the
chunk table.  This module lays out windows that sit on those edges — read count x column layout x content — and states what
the pileup must count for them with plain numpy (no code shared with oracle/).

Symbols as everywhere: A C G T = 0..3, '-' = 4, N = 5, not covered = 6; codon index = 16 b0 + 4 b1 + b2."""
import zlib

import numpy as np

from minorseq_amd import synth

GENE = np.dtype([("begin", "<u4"), ("end", "<u4")])

# ------------------------------------------------------------------------------------------------ the launch formulas, mirrored
# (kernels_pileup.hip: plane_tile_bytes, plane_flush_tiles, planes_nq; capi.hip: jl_plane_stride.  tests/test_pileup_edges_host.py
# compares the stride with the library's and the derived read counts with the figures the kernel's comments give.)
LINE_BYTES, LINE_READS = 128, 1024
NQ4_SINGLE_STRIDE = 32768          # a single run of 3-column chunks reads 16 bytes a lane from this plane stride on


def plane_stride(n_reads):
    return (n_reads + LINE_READS - 1) // LINE_READS * LINE_BYTES


def tile_bytes(nq):
    return 256 * 4 * nq             # 256 lanes x nq dwords


def tile_reads(nq):
    return 8 * tile_bytes(nq)


def flush_tiles(nq):
    return 1023 // (32 * nq)        # 64 lanes x 32 nq reads x tiles < 2^16


def single_nq(w, n_reads):
    return 4 if w == 3 and plane_stride(n_reads) >= NQ4_SINGLE_STRIDE else 2


def group_nq(w):
    return 4 if w == 3 else 2


def tiling(n_reads, nq):
    """(tiles, lanes of the 256 that are live in the last tile, flush batches of a workgroup that counts every tile)."""
    stride, tb = plane_stride(n_reads), tile_bytes(nq)
    tiles = (stride + tb - 1) // tb
    rest = stride - (tiles - 1) * tb
    return tiles, min(256, (rest + 4 * nq - 1) // (4 * nq)), (tiles + flush_tiles(nq) - 1) // flush_tiles(nq)


# read counts: `edge` reads fill something exactly, `edge + 1` open the next
EDGES = {
    "line": LINE_READS,                                        # one 128-byte stride step
    "tile_nq2": tile_reads(2),                                 # one tile of 8-byte loads
    "tile_nq4": tile_reads(4),                                 # one tile of 16-byte loads
    "batch_nq4": flush_tiles(4) * tile_reads(4),               # a full flush batch of 16-byte loads
    "batch_nq2": flush_tiles(2) * tile_reads(2),               # a full flush batch of 8-byte loads
    "nq4_single": (NQ4_SINGLE_STRIDE // LINE_BYTES - 1) * LINE_READS,   # the last stride a single run reads 8 bytes a lane at
    "two_batches_nq4": 2 * flush_tiles(4) * tile_reads(4),     # two full batches, then a third
}
SHALLOW = [1] + [EDGES[k] + d for k in ("line", "tile_nq2", "tile_nq4") for d in (0, 1)]
DEEP = [EDGES[k] + d for k in ("batch_nq4", "batch_nq2", "nq4_single", "two_batches_nq4") for d in (0, 1)]


# ------------------------------------------------------------------------------------------------ column layouts
def genes_of(layout, l):
    """frame: one gene in frame (3-column chunks, all on the fast stream; a filler of 1 or 2 columns ends a window whose width
    is no multiple of 3).  hiv: consecutive genes in different frames with fillers of 1 and 2 columns between them, a one-codon
    gene that overlaps (its chunk loads the halo), a gene that runs past the window end and a one-codon gene on the last three
    columns (3-column chunks, general stream with and without halo).  six: three overlapping genes in three frames (the
    6-column table)."""
    if layout == "frame":
        g = [(1, l + 1)]
    elif layout == "six":
        g = [(1, l + 1), (2, l + 1), (3, l + 7)]
    elif layout == "hiv":
        assert l >= 33
        g = [(2, 14), (16, 28), (21, 24), (28, l + 7), (l - 2, l + 1)]
    else:
        raise ValueError(layout)
    return np.array(g, dtype=GENE)


def wide_genes(layout, l):
    """Layouts of a window made of a repeated 24-column block.  frame: one gene in frame plus, in every block, a one-codon gene
    one column behind the block's last codon start, so that it straddles the seam — seven chunks of the block stay on the fast
    stream, one loads its halo."""
    if layout == "six":
        return genes_of("six", l)
    g = [(1, l + 1)] + [(b + 23, b + 26) for b in range(0, l - 24, 24)]
    return np.array(g, dtype=GENE)


def plan(genes, l):
    """What the library's plan makes of genes over l columns: dict(pos_col: evaluated codon starts in (gene, codon) order, w:
    chunk width, chunks: [(first column, own columns, start flags, halo, fast)])."""
    flag = np.zeros(l + 2, dtype=bool)
    pos_col = []
    for b, e in genes.tolist():
        if b == 0 or e <= b:
            continue
        for k in range((e - b) // 3):
            c = b - 1 + 3 * k
            if c + 2 < l:
                pos_col.append(c)
                flag[c] = True
    total = int(flag.sum())
    crowded = sum(1 for c in range(max(0, l - 2)) if flag[c] and (flag[c + 1] or flag[c + 2]))
    w = 6 if total and crowded * 4 > total else 3
    spans = []
    c = 0
    while c < l:
        if w == 6:
            n = min(6, l - c)
        elif flag[c]:
            n = min(3, l - c)
        else:
            n = 1
            while n < 3 and c + n < l and not flag[c + n]:
                n += 1
        spans.append((c, n))
        c += n
    chunks = []
    for c0, n in spans:
        startf = sum(1 << j for j in range(n) if flag[c0 + j])
        halo = (startf >> (n - 2)) != 0 if n >= 2 else startf != 0
        chunks.append((c0, n, startf, halo, w == 3 and n == 3 and startf == 1 and not halo))
    return dict(pos_col=np.array(pos_col, dtype=np.int64), w=w, chunks=chunks)


# ------------------------------------------------------------------------------------------------ contents
MIX = dict(partial_rate=0.2, mask_rate=0.05, del_rate=0.03, sub_rate=0.02, minor_permille=(100, 50, 30, 20))
# uniform columns: the codons AAA, TTT and CGT, then one column of each of '-', N and not covered, and so on
UNIFORM = np.array(["ACGT-N ".index(ch) for ch in "AAATTTCGT-N GCACCCAGT-GA"], dtype=np.uint8)
LANES = (0, 15, 16, 31, 32, 63)
LANE_MINOR = (1, 3, 5, 2, 4, 0)   # C T N G '-' A: both halves of each packed counter pair


def lane_of(reads, nq):
    """The lane of its wave that holds each read's 32-read word when a lane loads nq dwords of a plane per tile."""
    word = np.asarray(reads, dtype=np.int64) >> 5
    return (word % (256 * nq)) // nq % 64


def contents(content, n, l, seed):
    """(rows uint8[n][l], ref uint8[l]) — ref: base codes the reads mostly agree with."""
    if content == "mixture":
        sp = synth.SynthParams(seed=seed, **MIX)
        ref = synth.reference(seed, l)
        return synth.rows(sp, l, 0, n, ref), ref
    if content == "uniform":
        pat = UNIFORM[np.arange(l) % len(UNIFORM)]
        return np.broadcast_to(pat, (n, l)).copy(), np.where(pat < 4, pat, 0).astype(np.uint8)
    if content == "lanes":
        # column c: the minority symbol only in the reads of ONE lane of every wave — lanes 0, 15, 16, 31, 32, 63 as 8-byte loads
        # spread the reads (columns 0..5 of every 12), then the same lanes as 16-byte loads spread them (columns 6..11)
        rows = np.empty((n, l), dtype=np.uint8)
        ref = np.empty(l, dtype=np.uint8)
        reads = np.arange(n)
        for c in range(l):
            p = c % 12
            minor = LANE_MINOR[p % 6]
            ref[c] = 0 if minor else 1
            rows[:, c] = np.where(lane_of(reads, 2 if p < 6 else 4) == LANES[p % 6], minor, ref[c])
        return rows, ref
    raise ValueError(content)


# ------------------------------------------------------------------------------------------------ the plain reference
def column_counts(rows):
    """uint32[l][6]: reads per column that carry A C G T - N."""
    return np.stack([np.bincount(rows[:, c], minlength=7)[:6] for c in range(rows.shape[1])]).astype(np.uint32)


def codon_counts(rows, starts, cyclic=False):
    """(hist uint32[len(starts)][64], coverage uint32[len(starts)]) over the reads whose three codes are all < 4; cyclic: the
    codon of a start in the last two columns goes on in the first (the window is this block repeated)."""
    l = rows.shape[1]
    hist = np.zeros((len(starts), 64), dtype=np.uint32)
    for i, c in enumerate(starts):
        cols = [(int(c) + k) % l if cyclic else int(c) + k for k in range(3)]
        a, b, d = (rows[:, k].astype(np.intp) for k in cols)
        ok = (a < 4) & (b < 4) & (d < 4)
        hist[i] = np.bincount((16 * a + 4 * b + d)[ok], minlength=64)
    return hist, hist.sum(axis=1, dtype=np.uint32)


def window_counts(block, pos_col, l=None):
    """dict(col_counts, hist, coverage) of the window made of `block` repeated to l columns (None: the block itself), at the
    codon starts pos_col — computed on the block alone, codons that straddle a seam taken cyclically."""
    lb = block.shape[1]
    pos_col = np.asarray(pos_col, dtype=np.int64)
    if l is None:
        hist, cov = codon_counts(block, pos_col)
        return dict(col_counts=column_counts(block), hist=hist, coverage=cov)
    assert lb % 3 == 0 and lb <= 24
    hist, cov = codon_counts(block, np.arange(lb), cyclic=True)
    return dict(col_counts=column_counts(block)[np.arange(l) % lb], hist=hist[pos_col % lb], coverage=cov[pos_col % lb])


# ------------------------------------------------------------------------------------------------ cases
LAYOUT_COLS = {"frame": (12, 13, 14), "hiv": (36, 35, 34), "six": (24, 21, 23)}   # multiples of the chunk width, and not
COMPANION_READS = 2500     # the second window of a case's group run


class Case:
    def __init__(self, layout, content, n, l):
        self.layout, self.content, self.n, self.l = layout, content, n, l
        self.name = "%s-%s-%dx%d" % (layout, content, n, l)
        self.seed = zlib.crc32(self.name.encode()) & 0xFFFFFF
        self.genes = genes_of(layout, l)
        self.plan = plan(self.genes, l)
        self.w = self.plan["w"]

    def build(self):
        return contents(self.content, self.n, self.l, self.seed)

    def companion(self, ref):
        """The shallow window that shares the case's group runs: a mixture around the same reference."""
        return synth.rows(synth.SynthParams(seed=self.seed + 1, **MIX), self.l, 0, COMPANION_READS, ref)

    def expected(self, rows):
        return window_counts(rows, self.plan["pos_col"])

    def streams(self):
        fast = sum(1 for ch in self.plan["chunks"] if ch[4])
        return (["fast"] if fast else []) + (["general"] if fast < len(self.plan["chunks"]) else [])


def reference_modes(ref):
    """The three seeds of the codon compare: the reference, a reference that differs in every base (every read takes the slow
    bin walk), and majority mode."""
    return [("ref", ref), ("wrong", ((ref.astype(np.int64) + 1) % 4).astype(np.uint8)), ("majority", None)]


def _cases():
    out = {}
    for layout in ("frame", "hiv", "six"):
        k = ("frame", "hiv", "six").index(layout)
        depths = {
            # deep windows one past an edge in every layout; exactly on it, in one layout per edge
            "mixture": SHALLOW + [n for i, n in enumerate(DEEP) if i % 2 == 1 or (i // 2) % 3 == k],
            "uniform": [EDGES["line"] + 1] + DEEP,
            "lanes": [EDGES["tile_nq2"] + 1, EDGES["tile_nq4"] + 1, EDGES["batch_nq4"] + 1, EDGES["batch_nq2"] + 1],
        }
        for content, ns in depths.items():
            out[layout + "-" + content] = [Case(layout, content, n, LAYOUT_COLS[layout][(i + k) % 3]) for i, n in enumerate(ns)]
    return out


PARTS = _cases()   # part name -> cases; a part is what one child process of tests/test_gpu_pileup_edges.py runs


def taken(kernel, w, nq, streams, batches):
    """Ledger entries of one launch: (kernel, chunk width, NQ, stream, more than one flush batch in a workgroup)."""
    return {(kernel, w, nq, s, batches > 1) for s in streams}


def case_forms(case, folded):
    """What a narrow case's launches take.  A narrow window has so few chunks that a single run splits its reads one tile to
    a workgroup: it stores (and folds) only where the window is one tile deep.  folded: the process of the stage API, the single
    run and the folded group run; otherwise the process of the unfolded group run."""
    nq = single_nq(case.w, case.n)
    tiles = tiling(case.n, nq)[0]
    out = set()
    if folded:
        out |= taken("plain", case.w, nq, case.streams(), 1)
        if tiles == 1:
            out |= taken("fold", case.w, nq, case.streams(), 1)
        out |= taken("fold_group", case.w, group_nq(case.w), case.streams(), tiling(case.n, group_nq(case.w))[2])
    else:
        out |= taken("group", case.w, group_nq(case.w), case.streams(), tiling(case.n, group_nq(case.w))[2])
    return out


# Windows wide enough that a single run counts a chunk with ONE workgroup (or two) although it is many tiles deep: the column
# count comes from the device's occupancy at run time (tests/pileup_edges_child.py), the window is a 24-column block repeated.
# (layout, reads, read splits wanted): <3,2> 16 tiles, <3,4> 8 tiles, <6,2> 16 tiles in one workgroup; 7 tiles over 2 workgroups
WIDE = [("frame", EDGES["batch_nq2"] + 1, 1), ("frame", EDGES["nq4_single"] + 1, 1), ("six", EDGES["batch_nq2"] + 1, 1),
        ("frame", 7 * tile_reads(2), 2)]
WIDE_BLOCK = 24


def wide_columns(layout, blocks_per_cu, tiles, rsplit):
    """The narrowest window whose single run splits its reads `rsplit` ways: target / n_chunks == rsplit (jl_pileup_rsplit)."""
    target = 256 * blocks_per_cu * (4 if tiles >= 64 else 1)
    n_chunks = target // (rsplit + 1) + 1
    assert target // n_chunks == rsplit
    return n_chunks * (6 if layout == "six" else 3)


def wide_forms(layout, n, rsplit, folded=True):
    """The same for a wide window: stage API and single run (single launches do not depend on the group's form)."""
    w = 6 if layout == "six" else 3
    nq = single_nq(w, n)
    tiles = tiling(n, nq)[0]
    streams = ["general"] if w == 6 else ["fast", "general"]
    per_block = (tiles + rsplit - 1) // rsplit
    out = taken("plain", w, nq, streams, (per_block + flush_tiles(nq) - 1) // flush_tiles(nq))
    if folded and rsplit == 1:
        out |= taken("fold", w, nq, streams, tiling(n, nq)[2])
    return out


# every instantiation on every stream it has, with one and with more than one flush batch.  Not reachable: the 6-column table
# has no fast stream; a single run reads 16 bytes a lane only from 8 tiles on, so where ONE workgroup counts a chunk (the folded
# single launch) it has always more than the 7 tiles of a batch.
REQUIRED = ({(k, 3, nq, s, m) for k in ("plain", "fold") for nq in (2, 4) for s in ("fast", "general") for m in (False, True)}
            | {(k, 3, 4, s, m) for k in ("group", "fold_group") for s in ("fast", "general") for m in (False, True)}
            | {(k, 6, 2, "general", m) for k in ("plain", "fold", "group", "fold_group") for m in (False, True)}) \
    - {("fold", 3, 4, s, False) for s in ("fast", "general")}
