"""jl_class_codons_async on the device (docs/SPEC.md §24): the codon histograms of the resident matrix by class of reads at
chosen codon starts.  The expected table is always the numpy mirror (tests/class_codons_mirror.py) over the rows that are
resident, compared for equality on every integer, never with another device result — except where the rule itself says that
the table with one class is jl_pileup_fetch's."""
import numpy as np
import pytest

import class_codons_mirror as mirror
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

CELLS = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def code_rows(n, l, seed):
    """Seeded codes, bases four times as likely as '-' and N, one codon dominant per column triple, ragged code-6 ends."""
    rng = np.random.default_rng(seed)
    rows = np.broadcast_to(rng.integers(0, 4, size=l, dtype=np.uint8), (n, l)).copy()
    noise = rng.random((n, l))
    other = rng.choice(np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 5], dtype=np.uint8), size=(n, l))
    rows[noise < 0.3] = other[noise < 0.3]
    lo, hi = rng.integers(0, l // 3 + 1, size=n), l - rng.integers(0, l // 3 + 1, size=n)
    ci = np.arange(l)[None, :]
    rows[(ci < lo[:, None]) | (ci >= hi[:, None])] = 6
    return rows


def labels(name, n, k, seed):
    rng = np.random.default_rng(seed)
    if name == "all_one":
        return np.zeros(n, dtype=np.uint16)
    if name == "random":
        return rng.integers(0, k, size=n).astype(np.uint16)
    if name == "empty":            # classes with no read: one in the middle, the last of the first pass, the last of all
        lab = rng.integers(0, k, size=n).astype(np.uint16)
        for e in {k // 2, min(15, k - 1), k - 1}:
            lab[lab == e] = 0 if e else 0xFFFF
        return lab
    if name == "mixed":            # members beside 0xFFFE, 0xFFFF and n_classes itself, which fall out
        pool = np.array(list(range(k)) + [0xFFFE, 0xFFFF, k], dtype=np.uint16)
        lab = pool[rng.integers(0, len(pool), size=n)]
        lab[: min(n, 3)] = [0xFFFE, 0xFFFF, k][: min(n, 3)]
        return lab
    raise ValueError(name)


def starts(l, limit=None):
    """Every codon start of the window — column 0, l - 3, the three frames together, 61..64 where they exist — or, under a
    limit, those edges first."""
    cols = list(range(l - 2))
    if limit is not None and len(cols) > limit:
        edges = [c for c in (0, 1, 2, 61, 62, 63, 64, l - 3) if 0 <= c <= l - 3]
        cols = sorted(set(edges))[-limit:] if len(set(edges)) > limit else sorted(set(edges))
    return np.array(cols, dtype=np.uint32)


def check(j, rows, lab, k, cols):
    hist, reads = j.class_codons(lab, k, cols)
    exp_hist, exp_reads = mirror.class_codons(rows, lab, k, cols)
    assert hist.shape == exp_hist.shape and hist.dtype == np.uint32
    assert (reads == exp_reads).all()
    assert (hist == exp_hist).all()
    return hist


# (reads, columns, classes, labels): the 32-read word, the 512-read tile, the 1024-read mask line and one more tile against one
# pass, the pass edge, a leftover pass and JL_CLASS_MAX, sparsely paired; 704 classes with at most 8 positions
CASES = [
    (1, 3, 1, "all_one"), (31, 64, 15, "mixed"), (32, 65, 16, "empty"), (33, 130, 17, "random"), (511, 3, 33, "mixed"),
    (512, 64, 704, "random"), (513, 65, 1, "mixed"), (1023, 130, 15, "empty"), (1024, 3, 16, "random"), (1025, 64, 17, "mixed"),
    (2049, 65, 33, "empty"), (2049, 130, 704, "mixed"), (1, 130, 704, "all_one"), (33, 64, 1, "all_one"), (513, 130, 16, "mixed"),
    (1025, 65, 15, "random"), (31, 3, 17, "empty"), (1023, 64, 33, "random"), (2049, 130, 1, "all_one"), (512, 65, 17, "mixed"),
    (32, 130, 33, "empty"), (1024, 130, 15, "mixed"), (511, 65, 16, "random"),
]


@pytest.mark.parametrize("n,l,k,name", CASES)
def test_class_codons_equal_the_mirror(ctx, n, l, k, name):
    rows = code_rows(n, l, n * 1000 + l)
    lab = labels(name, n, k, n + 7 * l + k)
    cols = starts(l, 8 if k == 704 else None)
    ctx.upload_rows(rows, win_begin=3)
    hist = check(ctx, rows, lab, k, cols)
    # a class's coverage at a position is its reads with three bases there, and nobody else's
    full = (rows < 4)
    for p, c in enumerate(cols):
        assert int(hist[:, p].sum()) == int((full[:, c:c + 3].all(axis=1) & (lab < k)).sum())
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_one_position(ctx):
    rows = code_rows(600, 70, 5)
    ctx.upload_rows(rows)
    for c in (0, 62, 63, 67):
        check(ctx, rows, labels("mixed", 600, 5, c), 5, [c])


def test_a_few_thousand_positions_of_two_classes(ctx):
    """Every start of a window of n_pos + 2 columns: dozens of position groups in one launch."""
    n, l = 33, 3002
    rows = code_rows(n, l, 8)
    ctx.upload_rows(rows)
    check(ctx, rows, labels("mixed", n, 2, 1), 2, starts(l))


def test_one_class_is_the_pileups_histogram(ctx):
    """Every read in class 0: hist[0] is jl_pileup_fetch's hist at the same columns — all positions of three whole-window genes,
    one per frame."""
    n, l = 1025, 130
    rows = code_rows(n, l, 21)
    ctx.upload_rows(rows)
    genes = np.array([(1 + f, 1 + f + 3 * ((l - f) // 3)) for f in range(3)], dtype=capi.GENE)
    ctx.pileup_async(genes)
    pile = ctx.pileup_fetch()
    order = np.argsort(pile["pos_col"], kind="stable")
    cols = pile["pos_col"][order]
    assert len(cols) == l - 2 and (np.diff(cols) == 1).all()
    hist, reads = ctx.class_codons(np.zeros(n, dtype=np.uint16), 1, cols)
    assert reads.tolist() == [n]
    assert (hist[0] == pile["hist"][order]).all() and (hist[0].sum(axis=1) == pile["coverage"][order]).all()
    assert (hist[0] == mirror.class_codons(rows, np.zeros(n), 1, cols)[0]).all()


def test_planted_cells(ctx):
    """Three classes of 400 reads and 400 outside, interleaved; everybody reads ACG at every start but for what is planted per
    class: at start 3 k of class k ten reads with a '-', at start 3 k + 9 ten with an N, at start 3 k + 18 ten with an uncovered
    cell in each of the codon's three columns in turn; start 36 where every read deviates from ACG and the first reads do not
    agree on a codon either (nobody is the dominant one's), starts 27 to 33, 39 and 42 where nobody deviates."""
    n, k, l = 1600, 3, 45
    rows = np.broadcast_to(np.array([0, 1, 2] * 15, dtype=np.uint8), (n, l)).copy()
    lab = (np.arange(n) % 4).astype(np.uint16)
    lab[lab == 3] = 0xFFFF
    member = {c: np.flatnonzero(lab == c) for c in range(k)}
    for c in range(k):
        m = member[c]
        rows[m[0:10], 3 * c + 1] = 4
        rows[m[10:20], 3 * c + 9 + 2] = 5
        for f in range(3):
            rows[m[20 + 10 * f:30 + 10 * f], 18 + 3 * c + f] = 6   # (start 18 + 3 c: each of its three columns in turn)
    rng = np.random.default_rng(3)
    every = rng.integers(0, 4, size=(n, 3), dtype=np.uint8)
    every[(every == [0, 1, 2]).all(axis=1)] = [3, 3, 3]
    every[:128] = [[1, 1, 1], [2, 2, 2]] * 64          # the first reads do not agree on a codon either
    rows[:, 36:39] = every
    cols = np.arange(0, 43, 3, dtype=np.uint32)
    ctx.upload_rows(rows)
    hist = check(ctx, rows, lab, k, cols)
    acg = 0 * 16 + 1 * 4 + 2
    for c in range(k):
        for p in range(len(cols)):
            planted = 10 if cols[p] in (3 * c, 3 * c + 9) else 30 if cols[p] == 18 + 3 * c else 0
            if cols[p] == 36:
                assert hist[c, p, acg] == 0 and hist[c, p].sum() == 400
            else:                                           # one cell says it: the class's reads less the planted ones
                assert hist[c, p, acg] == 400 - planted and hist[c, p].sum() == 400 - planted, (c, p)


# ---------------------------------------------------------------------------------------------- every kind of resident matrix
def resident_rows(j):
    return msa.unpack_columns(j.download_columns(), j.n_reads)


def test_packed_upload(ctx):
    n, l = 1025, 65
    rows = code_rows(n, l, 31)
    ctx.upload_columns(msa.pack_columns(rows), n)
    check(ctx, rows, labels("mixed", n, 17, 1), 17, starts(l))


def test_synthetic_fill(ctx):
    n, l = 2049, 66
    sp = synth.SynthParams(seed=5, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    ctx.alloc(n, l)
    ctx.synth_fill(sp, ref)
    rows = synth.rows(sp, l, 0, n, ref)
    assert (resident_rows(ctx) == rows).all()
    check(ctx, rows, labels("random", n, 5, 2), 5, starts(l))


def test_record_build():
    n, l = 1500, 90
    rec = synth.raw_records(11, n, l)
    j = capi.Juliet(0)
    j.ingest_records(l, 0, rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"])
    rows = resident_rows(j)
    assert len(np.unique(rows)) >= 5                    # bases, and gaps or uncovered cells: not one symbol repeated
    check(j, rows, labels("mixed", n, 4, 3), 4, starts(l))
    j.close()


def test_segments_of_four_tiles():
    """The smallest window at which a workgroup of this kernel's own shape (jl_class_codons_shape_for) walks four tiles, so that the
    prefetching schedule has an iteration with a tile before and a tile after: 4609 tiles in 1153 segments, the last of one tile that
    ends inside it.  The rows are a 1536-read block — three tiles, so that tiles t and t + 2 differ — repeated with a tail, the labels too; the histograms are the block's
    times the repeats plus the tail's (tests/test_walk_host.py holds that property)."""
    import second_turn
    import walk_shape
    l, k = 12, 3
    cols = starts(l)
    n, seg_tiles, n_segs = walk_shape.deep_case(lambda n: walk_shape.class_codons(n, len(cols), k))
    assert seg_tiles >= 4 and n_segs >= 2 and -(-n // 512) % seg_tiles != 0 and n % 512 == 300
    block, lab = code_rows(1536, l, 11), labels("mixed", 1536, k, 5)
    reps, tail = second_turn.split(n, 1536)
    h, r = mirror.class_codons(block, lab, k, cols)
    th, tr = mirror.class_codons(block[:tail], lab[:tail], k, cols)
    exp_hist, exp_reads = (reps * h.astype(np.uint64) + th).astype(np.uint32), (reps * r.astype(np.uint64) + tr).astype(np.uint32)
    assert int((reps * h.astype(np.uint64) + th).max()) < 2 ** 32 and (exp_hist.sum(axis=(1, 2)) > 0).all() and th.any()
    j = capi.Juliet(0)
    try:
        second_turn.adopt_tiled(j, block, n)
        hist, reads = j.class_codons(second_turn.tiled(lab, n), k, cols)
        assert (reads == exp_reads).all()
        assert (hist == exp_hist).all(), np.argwhere(hist != exp_hist)[:8]
    finally:
        j.close()


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride, and that of the mask rows, is
    384), all ones in the bytes past the last read of every plane row — code 7 there, and bases once plane 2 is looked at alone.
    None of it may count."""
    import torch
    n, l, stride = 2049, 67, 272
    assert stride != msa.plane_stride(n) and stride % 16 == 0
    rows = code_rows(n, l, 99)
    planes = msa.pack_planes(rows, stride)
    planes[:, :, (n + 7) // 8:] = 0xFF
    planes[:, :, n // 8] |= (0xFF << (n % 8)) & 0xFF    # ... from the first bit behind the last read on
    planes[:, 2, (n + 7) // 8 + 1::2] = 0               # and every other byte of it a run of T's: codes < 4
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
    for k, name in ((17, "random"), (2, "mixed"), (1, "all_one")):
        check(j, rows, labels(name, n, k, k), k, starts(l))
    j.close()


# ---------------------------------------------------------------------------------------------- the contract
def fetch_copy(j):
    out = j.run_fetch(True, True, cap_var=64)
    return dict(variants=out["variants"].copy(), phase={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out["phase"].items()})


def assert_same_run(a, b):
    assert (a["variants"] == b["variants"]).all()
    assert a["phase"]["summary"] == b["phase"]["summary"]
    for key in ("pos_cols", "hap_count", "hap_pattern", "hit", "read_hap", "cooc"):
        assert (a["phase"][key] == b["phase"][key]).all(), key


def test_stage_results_and_the_class_pileup_are_kept(ctx):
    """A run with phasing and a class pileup, both fetched; the codon tables by the run's own ids; both fetched again: the same."""
    n, l = 2049, 130
    sp = synth.SynthParams(seed=5, minor_permille=(150, 120, 100, 80))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctx.upload_rows(rows)
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    first = fetch_copy(ctx)
    pile = ctx.pileup_fetch()
    h = first["phase"]["summary"]["n_haplotypes"]
    assert len(first["variants"]) >= 2 and h >= 2          # the input was chosen so that there is something to keep
    read_hap = first["phase"]["read_hap"]
    counts, creads = ctx.class_pileup(read_hap, h)
    hist = check(ctx, rows, read_hap, h, pile["pos_col"])
    assert (hist.sum(axis=(1, 2)) > 0).all()
    # a haplotype's reads show its own pattern at the variant positions
    at = {int(c): i for i, c in enumerate(pile["pos_col"])}
    for hh in range(h):
        for q, c in enumerate(first["phase"]["pos_cols"]):
            row = hist[hh, at[int(c)]]
            assert row[first["phase"]["hap_pattern"][hh][q]] == row.sum() == first["phase"]["hap_count"][hh]
    assert_same_run(first, fetch_copy(ctx))
    pile2 = ctx.pileup_fetch()
    for key in pile:
        assert (pile[key] == pile2[key]).all(), key
    counts2, creads2 = ctx.class_pileup_fetch()
    assert (counts2 == counts).all() and (creads2 == creads).all()
    assert (resident_rows(ctx) == rows).all()
    ctx.run_async(genes, ref, capi.default_params(), None, True, 10, True)
    assert_same_run(first, fetch_copy(ctx))


def test_a_large_call_then_a_smaller_one(ctx):
    n, l = 1025, 130
    rows = code_rows(n, l, 12)
    ctx.upload_rows(rows)
    check(ctx, rows, labels("random", n, 33, 1), 33, starts(l))
    check(ctx, rows, labels("mixed", n, 2, 2), 2, [5, 6, 70])
    check(ctx, rows, labels("random", n, 17, 3), 17, starts(l)[::2])


def test_two_calls_one_fetch_gives_the_last(ctx):
    n, l = 1025, 40
    rows = code_rows(n, l, 13)
    ctx.upload_rows(rows)
    lab = labels("random", n, 5, 4)
    keep = lab.copy()
    ctx.class_codons(labels("mixed", n, 17, 9), 17, starts(l), wait=False)
    cols = np.array([1, 2, 3, 30], dtype=np.uint32)
    ctx.class_codons(lab, 5, cols, wait=False)
    lab[:] = 0                                           # the inputs are copied before the call returns
    cols_keep = cols.copy()
    cols[:] = 0
    hist, reads = ctx.class_codons_fetch()
    exp_hist, exp_reads = mirror.class_codons(rows, keep, 5, cols_keep)
    assert (hist == exp_hist).all() and (reads == exp_reads).all()


def test_refusals_change_nothing():
    lib = capi.load_library()
    j = capi.Juliet(0)
    n, l = 40, 9
    lab = np.zeros(n, dtype=np.uint16)
    col = np.array([0, 3, 6], dtype=np.uint32)

    def refused(status, lab_ptr, k, col_arr, n_pos, word):
        rc = lib.jl_class_codons_async(j.h, lab_ptr, k, None if col_arr is None else col_arr.ctypes.data, n_pos)
        assert rc == status
        assert word in lib.jl_last_error(j.h).decode(), lib.jl_last_error(j.h)

    refused(-4, lab.ctypes.data, 3, col, 3, "no resident matrix")
    rows = code_rows(n, l, 1)
    j.upload_rows(rows)
    out = np.zeros((3, 3, 64), dtype=np.uint32)
    assert lib.jl_class_codons_fetch(j.h, out.ctypes.data, None) == -4            # a fetch before any call
    assert "before jl_class_codons_async" in lib.jl_last_error(j.h).decode()
    good = labels("random", n, 3, 5)
    hist, reads = j.class_codons(good, 3, col)
    assert (hist == mirror.class_codons(rows, good, 3, col)[0]).all()
    refused(-1, None, 3, col, 3, "no labels")
    refused(-1, lab.ctypes.data, 3, None, 3, "no positions array")
    refused(-1, lab.ctypes.data, 0, col, 3, "no classes")
    refused(-1, lab.ctypes.data, 705, col, 3, "at most 704")
    refused(-1, lab.ctypes.data, 3, col, 0, "no positions")
    refused(-1, lab.ctypes.data, 3, np.array([0, 3, 3], dtype=np.uint32), 3, "not strictly ascending")
    refused(-1, lab.ctypes.data, 3, np.array([3, 0, 6], dtype=np.uint32), 3, "not strictly ascending")
    refused(-1, lab.ctypes.data, 3, np.array([0, 3, 7], dtype=np.uint32), 3, "ends beyond")       # col + 2 == n_cols
    # one cell above the cap: the cap is checked before the columns are looked at, so the array need not be that long
    refused(-1, lab.ctypes.data, 1, col, CELLS + 1, "cells")
    refused(-1, lab.ctypes.data, 704, col, CELLS // 704 + 1, "cells")
    again, reads2 = j.class_codons_fetch()                                       # what was enqueued before is still there
    assert (again == hist).all() and (reads2 == reads).all()
    assert (j.class_codons(good, 704, col)[0][:3] == hist).all()                 # 704 itself is accepted
    assert (msa.unpack_columns(j.download_columns(), n) == rows).all()
    j.close()
