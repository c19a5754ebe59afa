"""jl_read_hypermut_async on the device (docs/SPEC.md §26): per read of the resident matrix its G->A sites in APOBEC's target and
control contexts, the mutated ones of each, and the one-sided exact test; jl_hypermut_eval, jl_hypermut_filter and jl_msa_take on top
of it.  Every expectation is tests/hypermut_mirror.py — a few numpy comparisons over the three shifted views of the rows that were
uploaded, and exact rational p-values —, the counters compared for equality on every entry; never another device result.  The sizes
are the edges of the launch shape, named by the function the launcher calls (tests/readstats_shape.py): a workgroup owns WG = 2048
reads (a lane one 32-read word), a column segment SEG columns and reads two more for context (the halo), the bit-sliced counters
are flushed every F = 2^k - 1 columns."""
import itertools

import numpy as np
import pytest

import hypermut_mirror as hm
import readstats_mirror as rm
import readstats_shape
from hypermut_tables import assert_p_close, designed_tables, exhaustive_tables, to_counts
from minorseq_amd import capi, msa

pytestmark = pytest.mark.gpu

F = readstats_shape.shape(97, 64)["flush"]
WG = readstats_shape.shape(97, 64)["wg_reads"]
SEG = readstats_shape.shape(1025, 3000)["seg_cols"]      # the columns of a segment at up to 2048 reads: the smallest a long window gets
A, C_, G, T = hm.A, hm.C, hm.G, hm.T
TRIPLES = np.array(list(itertools.product(range(7), repeat=3)), dtype=np.uint8)      # all 7^3 cell triples, one per read


@pytest.fixture(scope="module")
def ctx():
    j = capi.Juliet(0)
    yield j
    j.close()


def random_case(n, n_cols, seed):
    """All seven codes at random; a ref of all six meanings and bytes beyond, about half of it G."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 7, size=(n, n_cols), dtype=np.uint8)
    rows[rng.random((n, n_cols)) < 0.4] = G                  # ... and enough purines for sites to be common
    rows[rng.random((n, n_cols)) < 0.2] = A
    ref = rng.integers(0, 6, size=n_cols, dtype=np.uint8)
    ref[rng.random(n_cols) < 0.1] = 0xFF
    ref[rng.random(n_cols) < 0.5] = G
    return rows, ref


def check(j, rows, ref):
    """The counters equal the mirror's on every entry; the p-values are those of the exact test.  Returns (counts, p, log_p)."""
    exp = hm.counts(rows, ref)
    got, p, lp = j.read_hypermut(ref)
    assert got.dtype == np.uint32 and got.shape == (4, rows.shape[0])
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    assert p.shape == lp.shape == (rows.shape[0],)
    return got, p, lp


# ---------------------------------------------------------------------------------------------- the counters
@pytest.mark.parametrize("ref0", [0, 1, 2, 3, 4, 5, 0xFF])
def test_truth_table(ctx, ref0):
    """All 343 triples of cells as 343 reads of a 3-column window: the one possible site, under every meaning of its ref byte."""
    ref = np.array([ref0, G, G], dtype=np.uint8)
    ctx.upload_rows(TRIPLES)
    got, _, _ = check(ctx, TRIPLES, ref)
    if ref0 == G:      # x in {A, G}, y and z bases: 2 * 4 * 4 sites, 2 * 2 * 3 of them in the target context
        assert got[hm.TARGET_SITES].sum() == 12 and got[hm.CONTROL_SITES].sum() == 20 and got[hm.TARGET_MUT].sum() == 6 and got[hm.CONTROL_MUT].sum() == 10
    else:
        assert not got.any()


@pytest.mark.parametrize("where", ["SEG-2", "SEG-1", "end"])
def test_truth_table_across_a_segment_boundary_and_at_the_window_end(ctx, where):
    """The same triples inside a longer window of random cells: the context crosses into the next segment by one column and by
    two (the halo), and ends on the window's last column."""
    n, n_cols = len(TRIPLES), 2 * SEG + 1
    s = readstats_shape.shape(n, n_cols)
    assert s["seg_cols"] == SEG and s["n_segs"] == 3
    at = {"SEG-2": SEG - 2, "SEG-1": SEG - 1, "end": n_cols - 3}[where]
    rows, ref = random_case(n, n_cols, 300 + at)
    rows[:, at:at + 3] = TRIPLES
    ref[at] = G
    ctx.upload_rows(rows)
    check(ctx, rows, ref)
    alone = hm.counts(TRIPLES, np.array([G, G, G], dtype=np.uint8))
    assert alone.any() and (hm.counts(rows, ref) >= alone).all()      # (the planted site is among those counted)


@pytest.mark.parametrize("n_cols", [1, 2])
def test_windows_too_short_for_a_site(ctx, n_cols):
    n = 1025
    rows = np.full((n, n_cols), A, dtype=np.uint8)
    ctx.upload_rows(rows)
    got, p, lp = check(ctx, rows, np.full(n_cols, G, dtype=np.uint8))
    assert not got.any() and (p == 1.0).all() and (lp == 0.0).all()


@pytest.mark.parametrize("n_cols", [3, F - 1, F, F + 1, 2 * F + 1, SEG, SEG + 1, SEG + 2, 2 * SEG + 1])
def test_column_edges(ctx, n_cols):
    n = 1025
    s = readstats_shape.shape(n, n_cols)
    assert s["n_segs"] == -(-n_cols // SEG) and s["seg_cols"] == min(SEG, n_cols) and s["flush"] == F      # the cases are the edges they claim to be
    rows, ref = random_case(n, n_cols, 200 + n_cols)
    ctx.upload_rows(rows)
    got, _, _ = check(ctx, rows, ref)
    assert got.any() == bool((ref[:-2] == G).any())


@pytest.mark.parametrize("n", [1, 31, 32, 33, WG - 1, WG, WG + 1])
def test_read_edges(ctx, n):
    rows, ref = random_case(n, 9, 100 + n)
    ctx.upload_rows(rows, win_begin=5)
    check(ctx, rows, ref)
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_adopted_matrix_with_its_own_stride():
    """A torch tensor as the matrix: 2049 reads in planes of 272 bytes (the library's own stride is 384); every bit past the last
    read holds an A under a G of the ref, followed by A: a mutated target site in every column.  None of it may show."""
    import torch
    n, n_cols, stride = 2049, 2 * SEG + 3, 272
    assert stride > (n + 7) // 8 and stride != msa.plane_stride(n) and stride % 64 != 0 and stride % 16 == 0
    rows, ref = random_case(n, n_cols, 99)
    pad = 8 * stride - n
    wrong = np.full((pad, n_cols), A, dtype=np.uint8)
    planes = msa.pack_planes(np.concatenate([rows, wrong]), stride)
    assert planes.shape == (n_cols, 3, stride)
    assert hm.counts(wrong, np.full(n_cols, G, dtype=np.uint8))[hm.TARGET_MUT].min() == n_cols - 2
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(planes).cuda(non_blocking=False)
    stream.synchronize()
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.adopt(t.data_ptr(), n, n_cols, stride, keep_alive=t)
    check(j, rows, ref)
    check(j, rows, np.full(n_cols, G, dtype=np.uint8))
    j.close()


@pytest.mark.parametrize("kind", ["target", "control"])
def test_staircase(ctx, kind):
    """Read r carries exactly r mod (S + 1) mutations of one kind in a window whose ref is all G and whose S sites are all of that
    kind: every count value, every carry 2^j - 1 -> 2^j, counts that straddle a flush and a segment, and totals above 255."""
    if kind == "target":      # G throughout: every column but the last two is a GGG site; an A at x leaves y and z purines
        n_cols = 4 * SEG + 7
        base = np.full(n_cols, G, dtype=np.uint8)
        sites = np.arange(n_cols - 2)
    else:                     # G T G T ...: the even columns are sites with y = T; the odd ones have no purine at x
        n_cols = 8 * SEG + 7
        base = np.where(np.arange(n_cols) % 2 == 0, G, T).astype(np.uint8)
        sites = np.arange(0, n_cols - 2, 2)
    S = len(sites)
    n = S + 1 + 40
    assert S > 255 and readstats_shape.shape(n, n_cols)["seg_cols"] == SEG
    want = (np.arange(n) % (S + 1)).astype(np.uint32)
    rows = np.repeat(base[None, :], n, axis=0)
    for r in range(n):
        rows[r, sites[:want[r]]] = A
    ctx.upload_rows(rows)
    got, p, _ = check(ctx, rows, np.full(n_cols, G, dtype=np.uint8))
    sites_k, mut_k = (hm.TARGET_SITES, hm.TARGET_MUT) if kind == "target" else (hm.CONTROL_SITES, hm.CONTROL_MUT)
    assert (got[sites_k] == S).all() and (got[mut_k] == want).all()       # the staircase itself
    assert not got[[k for k in range(4) if k not in (sites_k, mut_k)]].any()
    assert set(want.tolist()) == set(range(S + 1)) and (p == 1.0).all()   # (only one kind of site: nothing to test against)


@pytest.mark.parametrize("n_cols", [3, SEG, SEG + 1, SEG + 2, 2 * SEG, 255, 256, 257])
def test_last_two_columns_of_an_all_site_window(ctx, n_cols):
    n = 97
    rows = np.full((n, n_cols), G, dtype=np.uint8)
    rows[::2] = A
    ctx.upload_rows(rows)
    got, _, _ = check(ctx, rows, np.full(n_cols, G, dtype=np.uint8))
    assert (got[hm.TARGET_SITES] == n_cols - 2).all() and (got[hm.TARGET_MUT][::2] == n_cols - 2).all() and not got[hm.TARGET_MUT][1::2].any()


def test_several_chunks_and_segments(ctx):
    n, n_cols = 5000, 3 * SEG + 1
    s = readstats_shape.shape(n, n_cols)
    assert s["n_chunks"] == 3 and s["n_segs"] == 4
    rows, ref = random_case(n, n_cols, 17)
    ctx.upload_rows(rows)
    check(ctx, rows, ref)


def test_longest_segments_of_a_deep_window():
    """So many reads that the chunks alone fill the chip: the segments are the longest a byte counter allows, 255 columns (a
    multiple of F), and the halo of the first is the second's first two columns.  Filled on the device; no rows on the host at this
    size: 3000 reads of it are taken into a second window (jl_msa_take), downloaded, and their mirror compared with the same reads'
    entries of the deep table."""
    from minorseq_amd import synth
    n, l = 2048 * 1025, 300
    s = readstats_shape.shape(n, l)
    assert s["seg_cols"] == readstats_shape.SEG_COLS_MAX == 255 and 255 % F == 0 and s["n_segs"] == 2 and s["n_chunks"] == 1025
    ref = synth.reference(3, l)
    j, part = capi.Juliet(0), capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(synth.SynthParams(seed=3, sub_rate=0.2, del_rate=4e-3, mask_rate=1e-2, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), ref)
    deep, p, lp = j.read_hypermut(ref)
    idx = np.sort(np.random.default_rng(3).choice(n, size=3000, replace=False)).astype(np.uint32)
    idx[:3], idx[-3:] = (0, 1, 2), (n - 3, n - 2, n - 1)
    part.take([(j, idx)])
    rows = msa.unpack_columns(part.download_columns(), len(idx))
    exp = hm.counts(rows, ref)
    assert (deep[:, idx] == exp).all(), np.argwhere(deep[:, idx] != exp)[:8]
    assert all(exp[k].any() for k in range(4))                       # every counter moves
    assert_p_close(p[idx], lp[idx], exp)
    part.close()
    j.close()


# ---------------------------------------------------------------------------------------------- the test kernel
@pytest.fixture(scope="module")
def window(ctx):
    """One random window with hypermutated reads, resident on `ctx` for the tests below: (rows, ref, counts, p, log_p)."""
    rng = np.random.default_rng(5)
    n, n_cols = 3000, 400
    ref = rng.integers(0, 4, size=n_cols, dtype=np.uint8)
    ref[rng.random(n_cols) < 0.4] = G
    rows = np.repeat(ref[None, :], n, axis=0)
    noise = rng.random((n, n_cols)) < 0.02
    rows[noise] = rng.integers(0, 7, size=int(noise.sum()), dtype=np.uint8)
    edited = np.flatnonzero(rng.random(n) < 0.1)            # a minority of the reads: G -> A at most of their target sites
    for r in edited:
        tgt = np.flatnonzero((rows[r, :-2] == G) & ((rows[r, 1:-1] == A) | (rows[r, 1:-1] == G)) & (rows[r, 2:] < 4) & (rows[r, 2:] != C_))
        rows[r, tgt[rng.random(len(tgt)) < 0.6]] = A
    ctx.upload_rows(rows)
    got, p, lp = check(ctx, rows, ref)
    return rows, ref, got, p, lp


def test_fused_p_values_are_the_eval_of_their_counters_and_the_exact_test(ctx, window):
    rows, ref, got, p, lp = window
    ep, elp = ctx.hypermut_eval(got)
    assert (ep.view(np.uint64) == p.view(np.uint64)).all() and (elp.view(np.uint64) == lp.view(np.uint64)).all()      # bit for bit
    assert_p_close(p, lp, got)
    assert (p < 0.05).sum() > 100 and (p >= 0.05).sum() > 2000


def test_eval_over_the_count_domain(ctx):
    for tables in (exhaustive_tables(), designed_tables()):
        cnt = to_counts(tables)
        p, lp = ctx.hypermut_eval(cnt)
        assert_p_close(p, lp, cnt)
        nothing = (cnt[hm.TARGET_SITES] == 0) | (cnt[hm.CONTROL_SITES] == 0) | (cnt[hm.TARGET_MUT] == 0)
        assert (p[nothing] == 1.0).all() and (lp[nothing] == 0.0).all()
    bad = to_counts([(1, 2, 3, 4), (3, 2, 0, 4)])
    with pytest.raises(capi.JulietError) as e:
        ctx.hypermut_eval(bad)
    assert e.value.status == -1 and "more mutations than sites" in str(e.value)


# ---------------------------------------------------------------------------------------------- the stage contract
def test_beside_other_stages_and_fetched_in_the_other_order(ctx, window):
    rows, ref, got, p, lp = window
    n, n_cols = rows.shape
    assert ctx.read_hypermut(ref, wait=False) is None
    assert ctx.read_stats(ref, wait=False) is None
    ctx.pileup_async(np.array([(1, n_cols + 1)], dtype=capi.GENE))
    col_counts = ctx.pileup_fetch()["col_counts"].copy()
    stats = ctx.read_stats_fetch()
    again = ctx.read_hypermut_fetch()
    assert (col_counts == rm.column_counts(rows)).all()
    assert (stats == rm.stats(rows, ref)).all()
    assert (again[0] == got).all() and (again[1].view(np.uint64) == p.view(np.uint64)).all() and (again[2].view(np.uint64) == lp.view(np.uint64)).all()
    # ... the other way round, and a second fetch of each
    ctx.pileup_async(np.array([(1, n_cols + 1)], dtype=capi.GENE))
    ctx.read_stats(ref, wait=False)
    ctx.read_hypermut(ref, wait=False)
    for _ in range(2):
        assert (ctx.read_hypermut_fetch()[0] == got).all()
        assert (ctx.read_stats_fetch() == stats).all()
    assert (ctx.pileup_fetch()["col_counts"] == col_counts).all()
    assert (msa.unpack_columns(ctx.download_columns(), n) == rows).all()     # the matrix is untouched


def test_refusals(window):
    rows, ref, got, p, lp = window
    lib = capi.load_library()
    j = capi.Juliet(0)
    assert lib.jl_read_hypermut_async(j.h, ref.ctypes.data) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
    j.upload_rows(rows[:40])
    with pytest.raises(capi.JulietError) as e:                       # a fetch before any call
        j.read_hypermut_fetch()
    assert e.value.status == -4 and "before jl_read_hypermut_async" in str(e.value)
    good = check(j, rows[:40], ref)
    assert lib.jl_read_hypermut_async(j.h, None) == -1 and "no reference row" in lib.jl_last_error(j.h).decode()
    assert lib.jl_read_hypermut_fetch(j.h, None, None, None) == 0    # NULL: only wait
    after = j.read_hypermut_fetch()                                  # ... and the refused call changed nothing
    assert all((a == b).all() for a, b in zip(after, good))
    only_p = np.zeros(40)
    assert lib.jl_read_hypermut_fetch(j.h, None, only_p.ctypes.data, None) == 0 and (only_p == good[1]).all()
    j.close()


def test_composition_with_filter_and_take(ctx, window):
    """counts -> p -> jl_hypermut_filter -> jl_msa_take: the taken window is the mirror's kept rows."""
    rows, ref, got, p, lp = window
    _, _, frs = hm.p_values(got)
    assert all(abs(f - hm.Fraction(0.05)) > hm.Fraction(0.05) / 10**9 for f in frs)
    exp_idx, exp_flagged = hm.keep(frs, hm.Fraction(0.05))
    idx, flagged = capi.hypermut_filter(p, 0.05)
    assert idx.tolist() == exp_idx.tolist() and flagged == exp_flagged and 100 < flagged < len(rows) // 2
    taken = capi.Juliet(0)
    taken.take([(ctx, idx)])
    assert (msa.unpack_columns(taken.download_columns(), len(idx)) == rows[exp_idx]).all()
    kept_counts, kept_p, _ = check(taken, rows[exp_idx], ref)        # ... and the stage on the taken window
    assert (kept_p >= 0.05).all()
    taken.close()
