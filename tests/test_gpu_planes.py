"""The resident matrix byte for byte (include/juliet_hip.h "THE resident format"): what every producer writes into the planes,
read back by jl_msa_download_planes — a plain copy, no kernel — and compared with msa.pack_planes of by-row codes built in numpy
over the WHOLE plane row, so that the padding the pileup kernels rely on (code 6 to the row's end) is pinned where no download
through planes_to_nibbles_kernel shows it; and that kernel alone, on adopted tensors.  Shapes: tests/planes_cases.py, whose
wrong producers tests/test_planes_host.py tells apart with them.  Every comparison is == on whole arrays."""
import ctypes as C
import time

import numpy as np
import pytest

import planes_cases as pc
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

ERR_ARG = -1
MESSAGE = "matrix holds a symbol code outside 0..6"


@pytest.fixture(scope="module")
def jl():
    j = capi.Juliet(0)
    yield j
    j.close()


@pytest.fixture(scope="module")
def ctxs():
    c = [capi.Juliet(0) for _ in range(3)]
    yield c
    for j in c:
        j.close()


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def image_is(ctx, rows, what, stride=None):
    """The context's planes are the image of `rows`, padding included, at its plane stride."""
    stride = msa.plane_stride(len(rows)) if stride is None else stride
    assert ctx.plane_stride == stride and (ctx.n_reads, ctx.n_cols) == rows.shape, what
    same(ctx.download_planes(), msa.pack_planes(rows, stride), what)


def on_device(planes):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    torch.cuda.synchronize()
    return t


def has_no_matrix(ctx):
    lib, buf = ctx.lib, np.zeros(16, dtype=np.uint8)
    return lib.jl_msa_download_planes(ctx.h, capi._p(buf), 1) == ERR_ARG and lib.jl_msa_download(ctx.h, capi._p(buf), 1) == ERR_ARG


# ------------------------------------------------------------------------------------------------ a. the download alone
@pytest.mark.parametrize("n", pc.READS)
def test_download_of_adopted_planes(n):
    """planes_to_nibbles_kernel and the copy on tensors that hold msa.pack_planes: at the library's stride, at the smallest
    a caller may choose and one piece more, the bytes behind the smallest stride padding, 0x00 (code 0) or 0xFF (code 7).  The
    download shows the n reads, then the STORED bits of every read position the planes hold, then padding; a download of fewer
    bytes is the prefix of the full one and writes nothing behind it."""
    l = pc.cols_for(n)
    rows = pc.code_rows(n, l)
    lib = capi.load_library()
    for stride in pc.strides(n):
        for fill in (None, 0x00, 0xFF):
            if fill is not None and stride == pc.stride16(n):
                continue                                                     # (no byte behind the smallest stride)
            what = (n, stride, fill)
            planes = msa.pack_planes(rows, stride)
            if fill is not None:
                planes = pc.tail_filled(planes, n, fill)
            t = on_device(planes)
            ctx = capi.Juliet(0)
            ctx.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
            same(ctx.download_planes(), planes, what)
            full = ctx.download_columns()
            same(msa.unpack_columns(full, n), rows, what)
            same(full, pc.download_of_planes(planes, n), what)
            if fill is None:
                same(full, msa.pack_columns(rows), what)
            cs, total = msa.col_stride(n), msa.col_stride(n) * l
            for nbytes in sorted({b for b in (0, cs, cs + 1, total - 1, total) if b <= total}):
                part = np.full(total + 16, 0xA5, dtype=np.uint8)
                assert lib.jl_msa_download(ctx.h, capi._p(part), nbytes) == 0, (what, nbytes)
                assert (part[:nbytes] == full.reshape(-1)[:nbytes]).all() and (part[nbytes:] == 0xA5).all(), (what, nbytes)
            part = np.full(total + 16, 0xA5, dtype=np.uint8)
            assert lib.jl_msa_download(ctx.h, capi._p(part), total + 1) == ERR_ARG and (part == 0xA5).all(), what
            size = planes.size
            for nbytes in (0, stride + 1, size - 1):
                raw = np.full(size + 16, 0xA5, dtype=np.uint8)
                assert lib.jl_msa_download_planes(ctx.h, capi._p(raw), nbytes) == 0, (what, nbytes)
                assert (raw[:nbytes] == planes.reshape(-1)[:nbytes]).all() and (raw[nbytes:] == 0xA5).all(), (what, nbytes)
            raw = np.full(size + 16, 0xA5, dtype=np.uint8)
            assert lib.jl_msa_download_planes(ctx.h, capi._p(raw), size + 1) == ERR_ARG and (raw == 0xA5).all(), what
            same(t.cpu().numpy(), planes, what)                               # a download writes nothing
            ctx.close()


def test_download_planes_without_a_matrix():
    ctx = capi.Juliet(0)
    assert has_no_matrix(ctx)
    assert ctx.lib.jl_msa_download_planes(None, capi._p(np.zeros(4, np.uint8)), 1) == ERR_ARG
    ctx.alloc(9, 2)
    assert ctx.lib.jl_msa_download_planes(ctx.h, None, 1) == ERR_ARG
    ctx.close()


# ------------------------------------------------------------------------------------------------ b. the upload
@pytest.mark.parametrize("n", pc.READS)
def test_upload_writes_the_image(jl, n):
    """nibbles_to_planes_kernel: the caller's column stride may be wider than jl_col_stride(n) and whatever the buffer holds behind
    read n - 1 — valid codes, 7, or nibbles with bit 3 set, the high nibble of the last read's byte for odd n among them — is
    ignored: the same image, padding to the row's end."""
    l = pc.cols_for(n)
    rows = pc.code_rows(n, l)
    jl.upload_columns(msa.pack_columns(rows), n, win_begin=3)
    image_is(jl, rows, n)
    for wider in (0, 128, 384):
        for behind in (pc.PAD, 0x7, 0x8, 0xF):
            buf = pc.nibble_buffer(rows, msa.col_stride(n) + wider, behind)
            assert buf.shape == (l, msa.col_stride(n) + wider)
            if n & 1:
                assert (buf[:, n // 2] >> 4 == behind).all()
            jl.upload_columns(buf, n)
            image_is(jl, rows, (n, wider, behind))


@pytest.mark.parametrize("n", [1, 9, 64, 257, 1025])
def test_upload_rejects_a_bad_read_and_leaves_no_matrix(jl, n):
    l = pc.cols_for(n)
    rows = pc.code_rows(n, l)
    for at in (0, n - 1):
        for bad in (7, 8, 15):
            cells = np.full((l, 2 * msa.col_stride(n)), pc.PAD, dtype=np.uint8)
            cells[:, :n] = rows.T
            cells[l - 1, at] = bad
            jl.upload_columns(msa.pack_columns(rows), n)
            with pytest.raises(capi.JulietError) as e:
                jl.upload_columns(pc.to_nibbles(cells), n)
            assert e.value.status == ERR_ARG and MESSAGE in str(e.value), (n, at, bad)
            assert has_no_matrix(jl), (n, at, bad)


def test_upload_into_a_context_that_held_an_adopted_tensor():
    n, l, stride = 257, 3, 48
    planes = msa.pack_planes(pc.code_rows(n, l), stride)
    t = on_device(planes)
    ctx = capi.Juliet(0)
    ctx.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
    other = pc.code_rows(n, 5)[:, 2:]                              # another matrix of the same shape
    assert (other != pc.code_rows(n, l)).any()
    ctx.upload_columns(msa.pack_columns(other), n)
    image_is(ctx, other, "after adopt")
    same(t.cpu().numpy(), planes, "the adopted tensor")
    ctx.upload_rows(other)
    same(t.cpu().numpy(), planes, "the adopted tensor")
    ctx.close()


# ------------------------------------------------------------------------------------------------ c. the staging loop
def test_upload_and_download_in_two_staging_chunks(jl):
    """The only case that moves more than a few megabytes: 129 columns of 2^20 + 1 reads are 64.5 MiB of nibbles, two chunks of
    127 and 2 columns through the 64 MiB staging buffer, in both directions.  The buffer is random valid bytes, column c a window
    of one random vector (no two columns alike); behind read n - 1 it holds valid codes that are no padding."""
    t0 = time.perf_counter()
    sh = pc.staging_shape()
    n, l, cs = sh.n, sh.l, sh.col_stride
    per = pc.stage_per(l, cs)
    assert 1 < per < l <= 2 * per and l * cs > pc.STAGE_BYTES
    rng = np.random.default_rng(20)
    base = (rng.integers(0, 7, size=cs + l, dtype=np.uint8) | (rng.integers(0, 7, size=cs + l, dtype=np.uint8) << 4)).astype(np.uint8)
    buf = np.lib.stride_tricks.sliding_window_view(base, cs)[:l]
    buf = np.ascontiguousarray(buf)
    cols = pc.staging_columns(sh)
    assert cols == [0, per - 1, per, l - 1]
    jl.upload_columns(buf, n)
    assert jl.plane_stride == sh.stride
    planes = jl.download_planes()
    shown = jl.download_columns()
    assert shown.shape == buf.shape
    for c in cols:
        cells = pc.from_nibbles(buf[c:c + 1])[0, :n]
        same(planes[c:c + 1], msa.pack_planes(cells[:, None], sh.stride), ("planes of column", c))
        got = pc.from_nibbles(shown[c:c + 1])[0]
        assert (got[:n] == cells).all() and (got[n:] == pc.PAD).all(), ("download of column", c)
    print("staging case: %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ d. pack_rows, the synthetic fill
@pytest.mark.parametrize("n", pc.READS)
def test_pack_rows_writes_the_image(jl, n):
    for l in {pc.cols_for(n), 5}:
        rows = pc.code_rows(n, l)
        jl.upload_rows(rows, win_begin=1)
        image_is(jl, rows, (n, l))


@pytest.mark.parametrize("n", [1, 9, 257, 1025])
def test_pack_rows_rejects_a_bad_code_and_leaves_no_matrix(jl, n):
    l = pc.cols_for(n)
    for at in ((0, 0), (n - 1, l - 1)):
        for bad in (7, 8, 255):
            rows = pc.code_rows(n, l)
            jl.upload_rows(rows)
            rows[at] = bad
            with pytest.raises(capi.JulietError) as e:
                jl.upload_rows(rows)
            assert e.value.status == ERR_ARG and MESSAGE in str(e.value), (n, at, bad)
            assert has_no_matrix(jl), (n, at, bad)


SP = synth.SynthParams(seed=4, sub_rate=0.05, del_rate=0.1, mask_rate=0.1, partial_rate=0.5, minor_permille=(100, 100, 100, 100))


@pytest.mark.parametrize("l", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 9, 513, 1025])
def test_synth_fill_writes_the_image(jl, n, l):
    """synth_kernel: one block is 2048 reads x 64 columns.  Into a matrix of the library's and into a tensor adopted at a stride
    that is no whole line and held 0xAB everywhere: the fill writes every byte of it."""
    ref = synth.reference(SP.seed, l)
    rows = synth.rows(SP, l, 0, n, ref)
    if n * l > 500 and l > 1:
        assert len(np.unique(rows)) == 7
    jl.alloc(n, l)
    jl.synth_fill(SP, ref)
    image_is(jl, rows, (n, l))
    stride = pc.stride16(n) + 16
    t = on_device(np.full((l, 3, stride), 0xAB, dtype=np.uint8))
    ctx = capi.Juliet(0)
    ctx.adopt(t.data_ptr(), n, l, stride, keep_alive=t)
    ctx.synth_fill(SP, ref)
    image_is(ctx, rows, (n, l, stride), stride)
    same(t.cpu().numpy(), msa.pack_planes(rows, stride), (n, l, "tensor"))
    ctx.close()


@pytest.mark.parametrize("n", [9, 1025])
def test_synth_fill_window_writes_the_image(jl, n):
    l_full, b, l = 200, 71, 65
    ref = synth.reference(SP.seed, l_full)
    rows = synth.rows(SP, l_full, 0, n, ref)[:, b:b + l]
    jl.alloc(n, l, win_begin=b)
    jl.synth_fill_window(SP, ref)
    image_is(jl, np.ascontiguousarray(rows), n)


# ------------------------------------------------------------------------------------------------ e. the other producers
OTHER_READS = (1, 255, 257, 513, 1025)
_records = {}


def records(n):
    """n reads over about 40 columns from explicit cigars: deletions, insertions, clips, late starts and early ends; qualities on
    both sides of MIN_QV"""
    from test_gpu_ingest_edges import records_of
    if n not in _records:
        rng = np.random.default_rng(n)
        cigars, pos = [], []
        for i in range(n):
            a, b = int(rng.integers(1, 20)), int(rng.integers(1, 20))
            mid = [("D", int(rng.integers(1, 4)))] if i % 3 == 0 else [("I", 3)] if i % 3 == 1 else [("X", 1)]
            cigars.append(([("S", 2)] if i % 5 == 0 else []) + [("=", a)] + mid + [("=", b)])
            pos.append(int(rng.integers(0, 12)))
        _records[n] = records_of(cigars, 1000 + n, pos)
    return _records[n]


ING_COLS, ING_BEGIN = 37, 2


@pytest.mark.parametrize("n", OTHER_READS)
def test_record_ingest_writes_the_image(ctxs, n):
    import records_expand
    from test_gpu_qmask import MIN_QV, five, np_mask
    rec = records(n)
    plain = records_expand.expand(rec, ING_COLS, ING_BEGIN, 0)
    filt = records_expand.expand(rec, ING_COLS, ING_BEGIN, MIN_QV)
    if n > 200:
        assert len(np.unique(filt)) == 7 and (plain != filt).any()
    jl, win = ctxs[0], ctxs[1]
    jl.ingest_records(ING_COLS, ING_BEGIN, *five(rec))
    image_is(jl, plain, (n, "one piece"))
    jl.ingest_records(ING_COLS, ING_BEGIN, *five(rec), rec["qual"], rec["qual_off"], min_qv=MIN_QV)
    image_is(jl, filt, (n, "one piece, bytes"))
    for chunk in (1, 37):
        jl.ingest_records_chunked(ING_COLS, ING_BEGIN, *five(rec), rec["qual"], rec["qual_off"], min_qv=MIN_QV, chunk_reads=chunk)
        image_is(jl, filt, (n, "chunked", chunk))
    mask = np_mask(rec, MIN_QV)
    jl.ingest_records(ING_COLS, ING_BEGIN, *five(rec), min_qv=MIN_QV, qmask=mask)
    image_is(jl, filt, (n, "masked"))
    jl.ingest_records_chunked(ING_COLS, ING_BEGIN, *five(rec), min_qv=MIN_QV, chunk_reads=37, qmask=mask)
    image_is(jl, filt, (n, "masked, chunked"))
    jl.records_upload(*five(rec), qual=rec["qual"], qual_off=rec["qual_off"])
    try:
        win.records_window(jl, ING_COLS, ING_BEGIN, MIN_QV)
        image_is(win, filt, (n, "window"))
        win.records_window(jl, ING_COLS - 5, ING_BEGIN + 4, 0)
        image_is(win, np.ascontiguousarray(plain[:, 4:ING_COLS - 1]), (n, "second window"))
    finally:
        jl.records_drop()


@pytest.mark.parametrize("n", OTHER_READS)
def test_take_writes_the_image(ctxs, n):
    from test_gpu_take import code_rows
    a, b, dst = ctxs
    rows_a, rows_b = code_rows(300, 7, 1), code_rows(1100, 7, 2)
    a.upload_rows(rows_a, win_begin=5)
    b.upload_rows(rows_b, win_begin=5)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 300, size=n).astype(np.uint32)
    dst.take([(a, idx)])
    image_is(dst, rows_a[idx], (n, "one part"))
    if n > 1:
        first = n // 2 - (n // 2) % 8 + 3                            # the first part ends mid-byte, and so does the second
        assert first % 8 and n % 8 and 0 < first < n
        ia, ib = idx[:first], rng.integers(0, 1100, size=n - first).astype(np.uint32)
        dst.take([(a, ia), (b, ib)])
        image_is(dst, np.concatenate([rows_a[ia], rows_b[ib]]), (n, "two parts"))


@pytest.mark.parametrize("n", OTHER_READS)
def test_sites_assemble_writes_the_image(ctxs, n):
    import sites_mirror as sm
    from test_gpu_sites import mixed_case
    src, pc_ = ctxs[0], ctxs[1]
    rows, sites = mixed_case(n, 100 + n)
    src.upload_rows(rows, win_begin=7)
    pc_.sites_assemble(src, sites)
    image_is(pc_, sm.recode(rows, sites), n)
    image_is(src, rows, (n, "source"))


@pytest.mark.parametrize("n", OTHER_READS)
def test_sites_assemble_alleles_writes_the_image(ctxs, n):
    import insertion_sites_mirror as ism
    from test_insertion_sites_host import L, site_case
    src, pc_ = capi.Juliet(0), ctxs[1]
    rec, rows, evs, sites, alleles = site_case(n, 50 + n)
    src.track_insertion_reads()
    src.ingest_records(L, 0, rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"], min_qv=0)
    image_is(src, rows, (n, "source"))
    pc_.sites_assemble_alleles(src, sites, alleles)
    image_is(pc_, ism.site_matrix(rows, evs, sites, alleles), n)
    src.close()


@pytest.mark.parametrize("n", OTHER_READS)
def test_cross_window_pack_writes_the_image(n):
    """Into `pc` through both assemblies.  The slice assembly keeps whole lines (xwin_edges.stride_reads); the whole-column assembly
    keeps the windows' stride — here 16-byte multiples that are no whole line, adopted with garbage wherever no read is, and the
    pack still writes code 6 to the end of every row (include/juliet_hip.h)."""
    import xwin_edges as xe
    from test_gpu_xwin_edges import adopt_windows, assemble_whole, close_all, upload_windows
    table = xe.pack_table()
    rows = xe.pack_rows(n + 256, seed=n)
    cols = np.concatenate([np.arange(c, c + 3) for c in xe.PACK_POS])
    ctxs = upload_windows(rows, xe.PACK_WINDOWS)
    for begin, k in ((0, n), (256, n), (0, n + 256)):
        pc_ = capi.Juliet(0)
        _, pos = pc_.xwin_assemble_slice_local(ctxs, table, begin, k)
        assert pos.tolist() == list(xe.PACK_POS)
        image_is(pc_, np.ascontiguousarray(rows[begin:begin + k][:, cols]), (n, "slice", begin, k), xe.stride_reads(k) // 8)
        pc_.close()
    pc_ = capi.Juliet(0)
    assemble_whole(pc_, ctxs, table)
    image_is(pc_, np.ascontiguousarray(rows[:, cols]), (n, "whole"))
    pc_.close()
    close_all(ctxs)
    stride = pc.stride16(n + 256) + 16
    ctxs = adopt_windows(rows, xe.PACK_WINDOWS, stride)
    pc_ = capi.Juliet(0)
    assemble_whole(pc_, ctxs, table)
    image_is(pc_, np.ascontiguousarray(rows[:, cols]), (n, "whole, adopted"), stride)
    pc_.close()
    close_all(ctxs)


# ------------------------------------------------------------------------------------------------ f. consensus ties
def test_consensus_ties_take_the_lowest_symbol(jl):
    """consensus_kernel and jl_consensus_of_counts: `>` only, so the first of equal counts stays; N and uncovered reads vote for nothing."""
    A, Cc, G, T, GAP, N_, OUT = range(7)
    columns = [[A, Cc] * 5, [T, GAP] * 5, [A, Cc, G, T, GAP] * 2, [Cc, A] * 5, [GAP, T, N_, OUT, N_] * 2, [N_] * 10, [OUT] * 10, [G, GAP, N_, N_, N_] * 2]
    exp = [A, T, A, A, T, 5, 5, G]
    rows = np.array(columns, dtype=np.uint8).T.copy()
    jl.upload_rows(rows)
    image_is(jl, rows, "ties")
    jl.pileup_async(np.array([(1, 7)], dtype=capi.GENE))
    got = jl.consensus()
    counts = jl.pileup_fetch()["col_counts"]
    assert (counts == np.stack([np.bincount(c, minlength=7)[:6] for c in columns])).all()
    assert got.tolist() == exp
    assert capi.consensus_of_counts(counts).tolist() == exp
