"""The designed pileup windows of tests/pileup_edges.py, without a GPU: their plain numpy reference against the oracle, the
repeated-block reference against the materialised window, and every case's read count, layout and intended kernel form against
the figures the kernel's comments give.  tests/test_gpu_pileup_edges.py sends the same cases through the kernels."""
import numpy as np
import pytest

import pileup_edges as pe
from minorseq_amd import capi

ALL = [c for part in pe.PARTS.values() for c in part]


def test_read_counts_sit_on_the_edges_their_names_say():
    """The derived read counts are the ones of the kernel's own arithmetic (256 lanes x 8 or 16 bytes of a plane a tile, 15 or 7
    tiles a flush batch, 16-byte loads of a single run from a 32 KiB plane on), and the stride is the library's."""
    lib = capi.load_library()
    for n in pe.SHALLOW + pe.DEEP + [1000, 100000, 7 * pe.tile_reads(2)]:
        assert pe.plane_stride(n) == lib.jl_plane_stride(n)
    assert (pe.tile_reads(2), pe.tile_reads(4), pe.flush_tiles(2), pe.flush_tiles(4)) == (16384, 32768, 15, 7)
    assert pe.SHALLOW == [1, 1024, 1025, 16384, 16385, 32768, 32769]
    assert pe.DEEP == [229376, 229377, 245760, 245761, 261120, 261121, 458752, 458753]
    # the margin of the packed 16-bit fields: a wave's batch of reads that all carry one symbol
    assert 64 * 32 * 4 * pe.flush_tiles(4) == 57344 and 64 * 32 * 2 * pe.flush_tiles(2) == 61440
    # (read count, NQ) -> tiles, live lanes of the last tile, flush batches of one workgroup
    for n, nq, exp in [(1, 2, (1, 16, 1)), (1024, 4, (1, 8, 1)), (1025, 2, (1, 32, 1)), (16384, 2, (1, 256, 1)), (16385, 2, (2, 16, 1)),
                       (32768, 4, (1, 256, 1)), (32769, 4, (2, 8, 1)), (229376, 4, (7, 256, 1)), (229377, 4, (8, 8, 2)),
                       (245760, 2, (15, 256, 1)), (245761, 2, (16, 16, 2)), (458752, 4, (14, 256, 2)), (458753, 4, (15, 8, 3)),
                       (261121, 4, (8, 256, 2)), (7 * 16384, 2, (7, 256, 1))]:
        assert pe.tiling(n, nq) == exp, (n, nq)
    # the load width of a single run changes between 261 120 and 261 121 reads, for 3-column chunks only
    assert [pe.single_nq(3, n) for n in (261120, 261121)] == [2, 4] and [pe.single_nq(6, n) for n in (261120, 261121)] == [2, 2]
    assert (pe.group_nq(3), pe.group_nq(6)) == (4, 2)


@pytest.mark.parametrize("layout", ["frame", "hiv", "six"])
def test_layouts_give_the_chunk_tables_their_names_say(layout):
    for l in pe.LAYOUT_COLS[layout]:
        p = pe.plan(pe.genes_of(layout, l), l)
        chunks = p["chunks"]
        assert sum(n for _, n, _, _, _ in chunks) == l and len(p["pos_col"]) > 0
        last = chunks[-1]
        if layout == "six":
            assert p["w"] == 6 and not any(f for *_, f in chunks)
            assert last[1] == (l % 6 or 6)                                # the chunk that ends the window: fewer own columns than W
            assert all(h for _, n, s, h, _ in chunks[:-1]) and not last[3]   # (no codon starts in the window's last two columns)
        elif layout == "frame":
            assert p["w"] == 3 and sum(f for *_, f in chunks) == l // 3
            assert (len(chunks) - l // 3, last[1], last[2]) == ((1, l % 3, 0) if l % 3 else (0, 3, 1))   # a filler of 1 or 2 columns
        else:
            assert p["w"] == 3
            fillers = sorted(n for _, n, s, _, _ in chunks if s == 0)
            assert 1 in fillers and 2 in fillers
            halo = [(c0, n, s) for c0, n, s, h, _ in chunks if h]
            assert (18, 3, 5) in halo and len(halo) == (2 if l % 3 else 1)   # the overlapping codon; a pair at a ragged window end
            assert sum(f for *_, f in chunks) >= 6
            assert int(pe.genes_of(layout, l)["end"][3]) > l + 1          # a gene runs past the window end
            if l % 3 == 1:                                                # the halo of the last codon pair reaches column n_cols
                assert (l - 4, 3, 3) in halo
    for layout_w, l in (("frame", 24 * 5 + 9), ("six", 24 * 3 + 6)):
        p = pe.plan(pe.wide_genes(layout_w, l), l)
        assert p["w"] == (6 if layout_w == "six" else 3) and len(p["chunks"]) == -(-l // p["w"])
        if layout_w == "frame":
            assert sum(h for _, _, _, h, _ in p["chunks"]) == 5 and sum(f for *_, f in p["chunks"]) == len(p["chunks"]) - 5


def test_cases_reach_every_kernel_form():
    """Every instantiation of the four pileup kernels, on every stream it has, with one and with more than one flush batch, is
    what some designed case takes (the GPU test asserts through the library's read-out that the case really took it)."""
    got = set()
    for folded in (True, False):
        for c in ALL:
            got |= pe.case_forms(c, folded)
        for layout, n, rsplit in pe.WIDE:
            got |= pe.wide_forms(layout, n, rsplit, folded)
    assert pe.REQUIRED - got == set()
    # the uniform columns fill the packed fields to their margin: full batches of 16-byte and of 8-byte loads, in every layout
    for layout in pe.LAYOUT_COLS:
        ns = {c.n for c in pe.PARTS[layout + "-uniform"]}
        assert {229376, 245760, 458752, 458753} <= ns
    assert {c.n for c in ALL} == set(pe.SHALLOW + pe.DEEP)
    assert pe.wide_columns("frame", 3, 8, 1) == 3 * 385 and pe.wide_columns("six", 2, 16, 1) == 6 * 257
    assert pe.wide_columns("frame", 4, 7, 2) == 3 * 342 and 1024 // 342 == 2


def test_contents_are_what_they_claim():
    rows, ref = pe.contents("uniform", 50, 24, 0)
    assert (rows == rows[0]).all() and set(rows[0].tolist()) == set(range(7))            # a column of each of the seven codes
    assert [tuple(rows[0, c:c + 3]) for c in (0, 3, 6)] == [(0, 0, 0), (3, 3, 3), (1, 2, 3)] and (ref < 4).all()
    wrong = pe.reference_modes(ref)[1][1]
    assert (wrong != ref).all() and (wrong < 4).all()
    n = 2 * pe.tile_reads(4) + 77
    rows, ref = pe.contents("lanes", n, 12, 0)
    reads = np.arange(n)
    for c in range(12):
        nq = 2 if c < 6 else 4
        minority = rows[:, c] != ref[c]
        assert (rows[minority, c] == pe.LANE_MINOR[c % 6]).all()
        assert (pe.lane_of(reads[minority], nq) == pe.LANES[c % 6]).all() and minority.sum() >= 32 * nq * 4 * 2
    # a lane's reads as the kernel takes them: lane t of the workgroup reads bytes [4 nq t, 4 nq (t + 1)) of a tile's plane
    for nq in (2, 4):
        t = np.arange(256)
        first = 8 * 4 * nq * t
        assert (pe.lane_of(first, nq) == t % 64).all() and (pe.lane_of(first + 32 * nq - 1, nq) == t % 64).all()
        assert (pe.lane_of(first + pe.tile_reads(nq), nq) == t % 64).all()


@pytest.mark.parametrize("part", sorted(pe.PARTS))
def test_numpy_reference_equals_oracle(oracle, part):
    for c in pe.PARTS[part]:
        rows, ref = c.build()
        assert rows.shape == (c.n, c.l) and rows.max() <= 6 and (ref < 4).all()
        exp = c.expected(rows)
        assert (exp["col_counts"] == oracle.pileup(rows)).all(), c.name
        hist, cov = oracle.codon_hist(rows, c.plan["pos_col"])
        assert (exp["hist"] == hist).all() and (exp["coverage"] == cov).all(), c.name
        assert (exp["col_counts"].sum(axis=1) == (rows != 6).sum(axis=0)).all()


@pytest.mark.parametrize("layout,l", [("frame", 24 * 4), ("frame", 24 * 3 + 13), ("six", 24 * 3 + 10)])
def test_block_reference_equals_materialised_window(oracle, layout, l):
    block, _ = pe.contents("mixture", 3000, pe.WIDE_BLOCK, 5)
    rows = np.tile(block, (1, -(-l // pe.WIDE_BLOCK)))[:, :l]
    pos_col = pe.plan(pe.wide_genes(layout, l), l)["pos_col"]
    assert (pos_col % pe.WIDE_BLOCK >= pe.WIDE_BLOCK - 2).any()       # codons that straddle a seam
    got = pe.window_counts(block, pos_col, l)
    exp = pe.window_counts(rows, pos_col)
    for k in exp:
        assert (got[k] == exp[k]).all(), k
    assert (got["col_counts"] == oracle.pileup(rows)).all()
    hist, cov = oracle.codon_hist(rows, pos_col)
    assert (got["hist"] == hist).all() and (got["coverage"] == cov).all()
