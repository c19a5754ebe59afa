"""jl_read_orf_async on the device (docs/SPEC.md §27): per (span, read) of the resident matrix the covered cells, the gap cells, the
codons read in full, the stops the reference does not have and the first of them; jl_orf_classify, jl_orf_filter and jl_msa_take on
top of it.  Every expectation is tests/orf_mirror.py — a loop by row over the rows that were uploaded, written from the SPEC —, all
five arrays compared for equality on every entry; never another device result.  The sizes are the edges of the launch shape, named
by the function the launcher calls (tests/orf_shape.py): a workgroup owns WG = 2048 reads (a lane one 32-read word) and one segment
of one span, SEG codons of it; the bit-sliced counters are flushed every FLUSH codons."""
import itertools

import numpy as np
import pytest

import orf_mirror as om
import orf_shape
import readstats_mirror as rm
from minorseq_amd import capi, msa

pytestmark = pytest.mark.gpu

A, C_, G, T = om.A, om.C, om.G, om.T
WG = orf_shape.shape([40], 97)["wg_reads"]
FLUSH = orf_shape.shape([40], 97)["flush_codons"]
SEG = orf_shape.shape([400], 97)["seg_codons"]          # the codons of a segment at up to 2048 reads: the smallest a long span gets
SEG_MAX = orf_shape.constants()["seg_codons_max"]
TRIPLES = np.array(list(itertools.product(range(7), repeat=3)), dtype=np.uint8)      # all 7^3 cell triples, one per read
STOPS = sorted(om.STOP_CODONS)


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def random_case(n, n_cols, seed, stops=0.15):
    """All seven codes at random, T A G in excess so that stops are common; a ref of all six meanings and bytes beyond."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 7, size=(n, n_cols), dtype=np.uint8)
    base = rng.random((n, n_cols)) < 0.75
    rows[base] = rng.choice(np.array([A, G, T, T, A, C_], dtype=np.uint8), size=int(base.sum()))
    for k in range(0, n_cols - 2):                         # whole stop codons at every offset, so that every frame has some
        hit = rng.random(n) < stops / 3
        rows[hit, k:k + 3] = np.array(STOPS, dtype=np.uint8)[rng.integers(0, 3, size=int(hit.sum()))]
    ref = rng.integers(0, 6, size=n_cols, dtype=np.uint8)
    ref[rng.random(n_cols) < 0.05] = 0xFF
    for k in range(0, n_cols - 2, 7):                      # ... and reference stops that mask some of them
        ref[k:k + 3] = STOPS[k % 3]
    return rows, ref


def check(j, rows, spans, ref):
    """All five arrays equal the mirror's on every entry.  Returns (counts, first_stop)."""
    exp_c, exp_f = om.counters(rows, spans, ref)
    got_c, got_f = j.read_orf(spans, ref)
    assert got_c.dtype == np.uint32 and got_c.shape == (4, len(spans), rows.shape[0])
    assert got_f.dtype == np.uint32 and got_f.shape == (len(spans), rows.shape[0])
    for q in range(4):
        assert (got_c[q] == exp_c[q]).all(), (q, np.argwhere(got_c[q] != exp_c[q])[:8])
    assert (got_f == exp_f).all(), np.argwhere(got_f != exp_f)[:8]
    return got_c, got_f


# ---------------------------------------------------------------------------------------------- the truth table
REF_CODONS = [np.array(c, dtype=np.uint8) for c in itertools.product(range(4), repeat=3)]
REF_ODD = [np.array([code if p == at else T if p == 0 else A for p in range(3)], dtype=np.uint8) for code in (4, 5, 0xFF) for at in range(3)]


@pytest.fixture(scope="module")
def triples_ctx():
    j = capi.Juliet(0)
    j.upload_rows(TRIPLES)
    yield j
    j.close()


@pytest.mark.parametrize("ref", REF_CODONS + REF_ODD, ids=lambda r: "-".join(str(int(x)) for x in r))
def test_truth_table(triples_ctx, ref):
    """All 343 triples of cells as 343 reads of one span of one codon, under every reference codon and under reference codes 4, 5
    and 0xFF in each position."""
    got_c, got_f = check(triples_ctx, TRIPLES, [(0, 1)], ref)
    ref_is_stop = tuple(int(x) for x in ref) in om.STOP_CODONS
    assert got_c[om.CODONS_READ].sum() == 64 and got_c[om.STOPS].sum() == (0 if ref_is_stop else 3)
    assert (got_f != om.NO_STOP).sum() == (0 if ref_is_stop else 3) and set(got_f[got_f != om.NO_STOP].tolist()) <= {0}
    assert got_c[om.COVERED].sum() == 3 * 6 * 49 and got_c[om.GAP_CELLS].sum() == 3 * 49


# ---------------------------------------------------------------------------------------------- read and span edges
@pytest.mark.parametrize("n", [1, 31, 32, 33, WG - 1, WG, WG + 1])
def test_read_edges(ctx, n):
    rows, ref = random_case(n, 125, 100 + n)
    ctx.upload_rows(rows, win_begin=5)
    got_c, got_f = check(ctx, rows, [(2, 40)], ref)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched
    if n >= 31:
        assert got_c[om.STOPS].any() and (got_f != om.NO_STOP).any()


@pytest.mark.parametrize("n_cols", [3, 4, 5])
def test_windows_of_one_codon(ctx, n_cols):
    rows, ref = random_case(97, n_cols, 30 + n_cols, stops=0.9)
    ctx.upload_rows(rows)
    for col in range(n_cols - 2):      # the one span that fits, at every column it fits at
        check(ctx, rows, [(col, 1)], ref)


def test_span_edges(ctx):
    n, n_cols = 97, 3 * 41 + 2
    rows, ref = random_case(n, n_cols, 7)
    ctx.upload_rows(rows)
    check(ctx, rows, [(0, 5)], ref)                                   # col = 0
    check(ctx, rows, [(n_cols - 15, 5)], ref)                         # ends at n_cols
    check(ctx, rows, [(0, 41)], ref)                                  # the whole window (but its last two columns: no codon)
    check(ctx, rows, [(2, 41)], ref)                                  # ... and ending at n_cols
    got_c, got_f = check(ctx, rows, [(0, 40), (1, 40), (2, 40)], ref)  # the same columns in frames 0, 1, 2
    assert not (got_f[0] == got_f[1]).all() and not (got_f[1] == got_f[2]).all()
    got_c, _ = check(ctx, rows, [(9, 12), (9, 12)], ref)              # two identical spans
    assert (got_c[:, 0] == got_c[:, 1]).all()
    spans = [((5 * g) % 50, 1 + (g % 25)) for g in range(capi.ORF_MAX_SPANS)]   # 64 spans, in no order, every frame
    assert len(spans) == 64 and {c % 3 for c, _ in spans} == {0, 1, 2}
    check(ctx, rows, spans, ref)


# ---------------------------------------------------------------------------------------------- flush and segment edges
CODON_EDGES = sorted({FLUSH - 1, FLUSH, FLUSH + 1, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, SEG_MAX, SEG_MAX + 1, 2 * SEG_MAX + 1})


def test_the_edges_are_the_shape_functions():
    assert (SEG_MAX, SEG_MAX + 1, 2 * SEG_MAX + 1) == (85, 86, 171)
    for nc in CODON_EDGES:
        s = orf_shape.shape([nc], 3 * nc + 1)
        assert s["seg_codons"] == SEG and s["flush_codons"] == FLUSH and s["span_segs"] == [-(-nc // SEG)]


@pytest.mark.parametrize("nc", CODON_EDGES)
def test_gap_staircase(ctx, nc):
    """Read i has i gap cells, the first i of the span: every value of GAP_CELLS from 0 to the span's 3 nc, every carry, counts
    that straddle a flush and a segment; the other cells are bases, and a column outside the span is all gaps."""
    n, n_cols = 3 * nc + 1, 3 * nc + 2
    rows = np.full((n, n_cols), C_, dtype=np.uint8)
    rows[:, 0] = rows[:, -1] = om.GAP
    for i in range(n):
        rows[i, 1:1 + i] = om.GAP
    ctx.upload_rows(rows)
    got_c, got_f = check(ctx, rows, [(1, nc)], np.full(n_cols, C_, dtype=np.uint8))
    assert got_c[om.GAP_CELLS, 0].tolist() == list(range(n)) and (got_c[om.COVERED] == 3 * nc).all()
    assert got_c[om.CODONS_READ, 0].tolist() == [nc - -(-i // 3) for i in range(n)] and (got_f == om.NO_STOP).all()


@pytest.mark.parametrize("nc", CODON_EDGES)
def test_all_stop_window(ctx, nc):
    """Every codon of every read a stop: COVERED, CODONS_READ and STOPS reach the span's maximum, first_stop is 0; in frame 1 of
    the same columns TAGTAG reads AGT: no stop at all."""
    n, n_cols = 70, 3 * nc + 1
    rows = np.tile(np.array([T, A, G], dtype=np.uint8), (n, nc + 1))[:, :n_cols]
    rows[1::2] = np.tile(np.array([T, G, A], dtype=np.uint8), (n // 2, nc + 1))[:, :n_cols]
    ctx.upload_rows(rows)
    spans = [(0, nc)] + ([(1, nc)] if nc > 0 else [])
    got_c, got_f = check(ctx, rows, spans, np.full(n_cols, A, dtype=np.uint8))
    assert (got_c[om.COVERED] == 3 * nc).all() and (got_c[om.CODONS_READ] == nc).all() and not got_c[om.GAP_CELLS].any()
    assert (got_c[om.STOPS, 0] == nc).all() and (got_f[0] == 0).all()
    assert not got_c[om.STOPS, 1].any() and (got_f[1] == om.NO_STOP).all()


def test_first_stop_across_segments(ctx):
    """One span of three segments; reads whose stops lie at chosen codons, and a reference stop that masks one of them."""
    nc = 2 * SEG + 3
    assert orf_shape.shape([nc], 8)["span_segs"] == [3]
    n_cols = 3 * nc + 1
    where = [[SEG - 1], [SEG], [2 * SEG + 1], [3, 2 * SEG], [5, SEG + 2], [0], [nc - 1], []]
    rows = np.full((len(where), n_cols), C_, dtype=np.uint8)
    for i, ks in enumerate(where):
        for k in ks:
            rows[i, 1 + 3 * k:4 + 3 * k] = STOPS[(i + k) % 3]
    ref = np.full(n_cols, C_, dtype=np.uint8)
    ref[1 + 3 * 5:4 + 3 * 5] = (T, A, A)                   # the reference has a stop at codon 5 (segment 0): read 4's stop there is not counted
    ctx.upload_rows(rows)
    got_c, got_f = check(ctx, rows, [(1, nc)], ref)
    assert got_f[0].tolist() == [SEG - 1, SEG, 2 * SEG + 1, 3, SEG + 2, 0, nc - 1, om.NO_STOP]
    assert got_c[om.STOPS, 0].tolist() == [1, 1, 1, 2, 1, 1, 1, 0]


def test_a_deep_window(ctx):
    """More than one chunk and more than one segment together."""
    n, n_cols = 2 * WG + 1, 330
    spans = [(0, 100), (29, 100)]
    s = orf_shape.shape([100, 100], n)
    assert s["n_chunks"] == 3 and min(s["span_segs"]) > 1
    rows, ref = random_case(n, n_cols, 17, stops=0.05)
    ctx.upload_rows(rows)
    got_c, got_f = check(ctx, rows, spans, ref)
    assert all(got_c[q].any() for q in range(4)) and len(set(got_f[0].tolist())) > 20


def test_longest_segments_of_a_deep_window():
    """So many reads that the chunks alone fill the chip: the segments are the longest a byte counter allows, 85 codons, and spans
    of 85, 86 and 171 codons are one full segment, one and a codon, two and a codon.  Filled on the device; no rows on the host at
    this size: 3000 reads of it are taken into a second window (jl_msa_take), downloaded, and their mirror compared with the same
    reads' entries of the deep arrays."""
    from minorseq_amd import synth
    n, l = 2048 * 1025, 3 * (2 * SEG_MAX + 1) + 3
    spans = [(0, SEG_MAX), (1, SEG_MAX + 1), (2, 2 * SEG_MAX + 1)]
    s = orf_shape.shape([nc for _, nc in spans], n)
    assert s["seg_codons"] == SEG_MAX and s["span_segs"] == [1, 2, 3] and s["n_chunks"] == 1025
    ref = synth.reference(3, l)
    j, part = capi.Juliet(0), capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(synth.SynthParams(seed=3, sub_rate=0.2, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), ref)
    deep_c, deep_f = j.read_orf(spans, ref)
    idx = np.sort(np.random.default_rng(3).choice(n, size=3000, replace=False)).astype(np.uint32)
    idx[:3], idx[-3:] = (0, 1, 2), (n - 3, n - 2, n - 1)
    part.take([(j, idx)])
    rows = msa.unpack_columns(part.download_columns(), len(idx))
    exp_c, exp_f = om.counters(rows, spans, ref)
    assert (deep_c[:, :, idx] == exp_c).all(), np.argwhere(deep_c[:, :, idx] != exp_c)[:8]
    assert (deep_f[:, idx] == exp_f).all(), np.argwhere(deep_f[:, idx] != exp_f)[:8]
    assert all(exp_c[q].any() for q in range(4)) and ((exp_f[2] >= SEG_MAX) & (exp_f[2] != om.NO_STOP)).any() and (exp_f[2] < SEG_MAX).any()
    part.close()
    j.close()


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384); every bit past the last
    read spells a stop codon in every frame somewhere.  None of it may show — and the output holds n_reads entries per span."""
    import torch
    n, n_cols, stride = 2049, 3 * (SEG + 2) + 2, 272
    assert stride > (n + 7) // 8 and stride != msa.plane_stride(n) and stride % 64 != 0 and stride % 16 == 0
    rows, ref = random_case(n, n_cols, 99)
    pad = 8 * stride - n
    wrong = np.tile(np.array([T, A, G], dtype=np.uint8), (pad, n_cols // 3 + 1))[:, :n_cols]
    planes = msa.pack_planes(np.concatenate([rows, wrong]), stride)
    assert planes.shape == (n_cols, 3, stride)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, n_cols, stride, keep_alive=t)
    check(j, rows, [(0, SEG + 2), (1, SEG + 2), (2, SEG + 2)], ref)
    j.close()


# ---------------------------------------------------------------------------------------------- the stage contract
@pytest.fixture(scope="module")
def window(ctx):
    """One window of reads close to a reference with two overlapping reading frames, some reads with planted defects, resident on
    `ctx` for the tests below: (rows, ref, spans, counts, first_stop)."""
    rng = np.random.default_rng(5)
    n, n_cols = 3000, 400
    ref = rng.integers(0, 4, size=n_cols, dtype=np.uint8)
    spans = [(3, 90), (200, 60), (100, 66)]
    for col, nc in spans:                                   # a reference without stops in its own frames
        for k in range(nc):
            if tuple(ref[col + 3 * k:col + 3 * k + 3].tolist()) in om.STOP_CODONS:
                ref[col + 3 * k] = C_
    rows = np.repeat(ref[None, :], n, axis=0)
    noise = rng.random((n, n_cols)) < 0.004
    rows[noise] = rng.integers(0, 6, size=int(noise.sum()), dtype=np.uint8)
    for i in np.flatnonzero(rng.random(n) < 0.1):           # deletions of 1 .. 6 columns
        at = int(rng.integers(0, n_cols - 6))
        rows[i, at:at + int(rng.integers(1, 7))] = om.GAP
    for i in np.flatnonzero(rng.random(n) < 0.1):           # ragged ends
        rows[i, :int(rng.integers(1, 150))] = om.UNCOVERED
    ctx.upload_rows(rows)
    got_c, got_f = check(ctx, rows, spans, ref)
    return rows, ref, spans, got_c, got_f


def test_beside_other_stages_and_fetched_in_the_other_order(ctx, window):
    rows, ref, spans, got_c, got_f = window
    n = rows.shape[0]
    import hypermut_mirror as hm
    assert ctx.read_stats(ref, wait=False) is None
    assert ctx.read_orf(spans, ref, wait=False) is None
    assert ctx.read_hypermut(ref, wait=False) is None
    hyper = ctx.read_hypermut_fetch()
    orf = ctx.read_orf_fetch()
    stats = ctx.read_stats_fetch()
    assert (stats == rm.stats(rows, ref)).all() and (hyper[0] == hm.counts(rows, ref)).all()
    assert (orf[0] == got_c).all() and (orf[1] == got_f).all()
    for _ in range(2):                                      # a second fetch of each
        assert (ctx.read_orf_fetch()[1] == got_f).all() and (ctx.read_stats_fetch() == stats).all()
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_refusals_change_nothing(window):
    rows, ref, spans, got_c, got_f = window
    lib = capi.load_library()
    j = capi.Juliet(0)
    sp = capi.orf_spans(spans)
    n_cols = rows.shape[1]

    def call(s=sp, ns=None, r=ref):
        return lib.jl_read_orf_async(j.h, s.ctypes.data if s is not None else None, len(sp) if ns is None else ns, r.ctypes.data if r is not None else None)

    assert call() == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
    j.upload_rows(rows[:40])
    with pytest.raises(capi.JulietError) as e:              # a fetch before any call
        j.read_orf_fetch()
    assert e.value.status == -4 and "before jl_read_orf_async" in str(e.value)
    good = check(j, rows[:40], spans, ref)
    assert call(s=None) == -1 and "no spans" in lib.jl_last_error(j.h).decode()
    assert call(r=None) == -1 and "no reference row" in lib.jl_last_error(j.h).decode()
    assert call(ns=0) == -1 and call(ns=65) == -1 and "1 .. 64" in lib.jl_last_error(j.h).decode()
    for bad in ([(0, 0)], [(n_cols - 2, 1)], [(0, n_cols // 3 + 1)], [(2**32 - 1, 1)], [(4, (2**32 - 1) // 3 + 2)], [(3, 5), (n_cols, 1)]):
        b = capi.orf_spans(bad)
        assert lib.jl_read_orf_async(j.h, b.ctypes.data, len(b), ref.ctypes.data) == -1, bad
        assert "outside the window" in lib.jl_last_error(j.h).decode()
    assert lib.jl_read_orf_fetch(j.h, None, None) == 0      # NULL: only wait
    after = j.read_orf_fetch()                              # ... and the refused calls changed nothing
    assert all((a == b).all() for a, b in zip(after, good))
    only_f = np.zeros((len(spans), 40), dtype=np.uint32)
    assert lib.jl_read_orf_fetch(j.h, None, only_f.ctypes.data) == 0 and (only_f == good[1]).all()
    j.close()


def test_composition_with_classify_filter_and_take(ctx, window):
    """counters -> jl_orf_classify -> jl_orf_filter -> jl_msa_take: the taken window's own counters are the mirror's rows of the
    kept reads."""
    rows, ref, spans, got_c, got_f = window
    flags = capi.orf_classify(got_c, got_f, spans, max_gap_cells=4, tail_codons=2)
    exp_flags = om.classify(*om.counters(rows, spans, ref), spans, max_gap_cells=4, tail_codons=2)
    assert (flags == exp_flags).all() and all((flags & bit).any() for bit in (1, 2, 4, 8))
    for mask in (om.STOP | om.FRAMESHIFT, om.DELETION, om.STOP | om.FRAMESHIFT | om.DELETION):
        idx, flagged = capi.orf_filter(flags, mask)
        exp_idx, exp_flagged = om.keep(exp_flags, mask)
        assert idx.tolist() == exp_idx.tolist() and flagged == exp_flagged and 50 < flagged < len(rows) // 2
    taken = capi.Juliet(0)
    taken.take([(ctx, idx)])
    assert (msa.unpack_columns(taken.download_columns(), len(idx)) == rows[exp_idx]).all()
    kept_c, kept_f = check(taken, rows[exp_idx], spans, ref)
    assert (kept_c == got_c[:, :, exp_idx]).all() and (kept_f == got_f[:, exp_idx]).all()
    again = capi.orf_classify(kept_c, kept_f, spans, max_gap_cells=4, tail_codons=2)
    assert not (again & (om.STOP | om.FRAMESHIFT | om.DELETION)).any()
    taken.close()
