"""Cross-window phasing at its edges (tests/xwin_edges.py): what the pack launch writes, cell by cell, for slices that end on every
bit of a byte, on both sides of a 16-byte piece, a 128-byte line and a 16 KiB x-block, through both assemblies and from windows
adopted at a stride that is no whole line; every designed case sharded on one device, through a one-rank session with and
without a communicator, and through sessions of 2, 3 and 9 ranks as threads.  Every comparison is integer ==, against the numpy
statements of xwin_edges.py and phase_edges.phase of the whole matrix.  Runs only on a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import phase_edges as pe
import xwin_edges as xe
from minorseq_amd import capi, msa
from rank_threads import ranks_in_threads

pytestmark = pytest.mark.gpu

LOOSE = capi.default_params(alpha=0.9, n_tests=1.0)       # as phase_edges_child.LOOSE: every codon that is not the reference's is called
PARTIALS = ("damaged_reads", "marginal_gap", "marginal_heteroduplex", "marginal_partial", "n_positions")
COMPARED = {"sharded": set(), "session": set(), "ranks": set()}


def close_all(ctxs):
    for c in ctxs:
        c.close()


def upload_windows(rows, wins):
    ctxs = []
    for b, k in wins:
        c = capi.Juliet(0)
        c.upload_rows(rows[:, b:b + k], win_begin=b)
        ctxs.append(c)
    return ctxs


def adopt_windows(rows, wins, stride):
    """The windows as caller-owned planes at `stride` bytes a plane, with random bits wherever no read is."""
    import torch
    n = len(rows)
    rng = np.random.default_rng(n)
    ctxs = []
    for b, k in wins:
        planes = msa.pack_planes(rows[:, b:b + k], stride)
        nb = (n + 7) // 8
        planes[:, :, nb:] = rng.integers(0, 256, size=(k, 3, stride - nb), dtype=np.uint8)
        if n & 7:
            planes[:, :, nb - 1] ^= rng.integers(0, 256, size=(k, 3), dtype=np.uint8) & np.uint8(0xFF & ~((1 << (n & 7)) - 1))
        t = torch.from_numpy(planes).cuda()
        torch.cuda.synchronize()
        c = capi.Juliet(0)
        c.adopt(t.data_ptr(), n, k, stride, win_begin=b, keep_alive=t)
        ctxs.append(c)
    return ctxs


def assemble_whole(pc, ctxs, table):
    """jl_xwin_assemble_local: whole columns at the windows' plane stride."""
    arr = (C.c_void_p * len(ctxs))(*[w.h for w in ctxs])
    merged = np.ascontiguousarray(table, dtype=capi.VARIANT)
    remapped = np.zeros(max(1, len(merged)), dtype=capi.VARIANT)
    pos = np.zeros(max(1, len(merged)), dtype=np.uint32)
    vp = C.c_uint32()
    pc._chk(pc.lib.jl_xwin_assemble_local(pc.h, arr, len(ctxs), capi._p(merged), len(merged), capi._p(remapped), capi._p(pos), C.byref(vp)))
    pc._shape(ctxs[0].n_reads, 3 * vp.value, ctxs[0].plane_stride)
    return remapped[:len(merged)], pos[:vp.value]


def check_cells(what, pc, rows, pos, begin, k, plane_reads):
    """Every cell a download shows: the slice's reads, and 6 in every cell beyond (past the planes a download shows padding)."""
    shown = 2 * pc.col_stride
    got = msa.unpack_columns(pc.download_columns(), shown)
    exp = np.full((shown, 3 * len(pos)), 6, np.uint8)
    m = min(shown, plane_reads)
    exp[:m] = xe.pack_expected(rows, pos, begin, k, plane_reads)[:m]
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
    assert (got[k:] == 6).all(), what


def canon(t):
    p, c = np.asarray(t["patterns"]), np.asarray(t["counts"])
    order = np.lexsort(p.T[::-1]) if len(c) else np.zeros(0, np.int64)
    return p[order], c[order]


def check_groups(what, pc, remapped, rows, table, begin, end):
    """The exporting run on the assembled context: counts, patterns and partials of the slice."""
    pc.phase_groups_async(remapped)
    t = pc.phase_groups_fetch(cap_var=max(1, len(remapped)))
    exp = xe.slice_groups(rows, table, begin, end)
    (gp, gc), (ep, ec) = canon(t), canon(exp)
    assert gp.shape == ep.shape and (gp == ep).all() and (gc == ec).all(), (what, gp.shape, ep.shape)
    assert {f: t["summary"][f] for f in PARTIALS} == {f: exp["summary"][f] for f in PARTIALS}, (what, t["summary"], exp["summary"])
    assert int(gc.sum()) + t["summary"]["damaged_reads"] == end - begin, what


# ------------------------------------------------------------------------------------------------ the pack launch, cell by cell
@pytest.mark.parametrize("n_slice", xe.PACK_SMALL + xe.PACK_MORE + xe.PACK_BIG)
def test_pack_cell_by_cell(n_slice):
    table = xe.pack_table()
    runs = xe.pack_slices(n_slice)
    all_rows = xe.pack_rows(max(t for _, _, t in runs))
    for total in sorted({t for _, _, t in runs}):
        rows = all_rows[:total]
        ctxs = upload_windows(rows, xe.PACK_WINDOWS)
        for b, k, t in runs:
            if t != total:
                continue
            what = "n_slice %d from %d of %d" % (k, b, total)
            pc = capi.Juliet(0)
            remapped, pos = pc.xwin_assemble_slice_local(ctxs, table, b, k)
            assert pos.tolist() == list(xe.PACK_POS) and remapped["col"].tolist() == (3 * np.searchsorted(pos, table["col"])).tolist()
            check_cells(what, pc, rows, pos, b, k, xe.stride_reads(k))
            check_groups(what, pc, remapped, rows, table, b, b + k)
            pc.close()
            if b == 0 and k == total:        # the same reads through the whole-column assembly (the stride override)
                pc = capi.Juliet(0)
                remapped, pos = assemble_whole(pc, ctxs, table)
                check_cells(what + " whole", pc, rows, pos, 0, total, 8 * ctxs[0].plane_stride)
                check_groups(what + " whole", pc, remapped, rows, table, 0, total)
                pc.close()
        close_all(ctxs)


@pytest.mark.parametrize("n,stride", [(1, 16), (129, 32), (1025, 144), (1279, 160), (xe.XBLOCK_READS + 1, xe.XBLOCK_BYTES + 16)])
def test_pack_from_windows_adopted_at_a_stride_that_is_no_whole_line(n, stride):
    assert stride % 16 == 0 and stride % 128 != 0 and stride >= (n + 7) // 8
    table = xe.pack_table()
    rows = xe.pack_rows(n, seed=11)
    ctxs = adopt_windows(rows, xe.PACK_WINDOWS, stride)
    pc = capi.Juliet(0)
    remapped, pos = assemble_whole(pc, ctxs, table)
    assert pc.plane_stride == stride
    check_cells("adopted whole %d" % n, pc, rows, pos, 0, n, 8 * stride)
    check_groups("adopted whole %d" % n, pc, remapped, rows, table, 0, n)
    pc.close()
    for b, k in [(0, n)] + ([(256, n - 256), (256, 300)] if n > 600 else []):
        pc = capi.Juliet(0)
        remapped, pos = pc.xwin_assemble_slice_local(ctxs, table, b, k)
        check_cells("adopted slice %d+%d of %d" % (b, k, n), pc, rows, pos, b, k, xe.stride_reads(k))
        check_groups("adopted slice %d+%d of %d" % (b, k, n), pc, remapped, rows, table, b, b + k)
        pc.close()
    close_all(ctxs)


@pytest.mark.parametrize("name", ["pos-48", "pos-49"])
def test_pack_position_chunks_through_both_assemblies(name):
    rows, table = xe.CASES[name].build()
    n, l = rows.shape
    ctxs = upload_windows(rows, [(0, l)])
    pos_exp = xe.positions_of(table, l)
    assert len(pos_exp) == int(name[4:])
    for b, k in ((0, n), (256, n - 256)):
        pc = capi.Juliet(0)
        remapped, pos = pc.xwin_assemble_slice_local(ctxs, table, b, k)
        assert pos.tolist() == pos_exp.tolist()
        check_cells(name, pc, rows, pos, b, k, xe.stride_reads(k))
        check_groups(name, pc, remapped, rows, table, b, b + k)
        pc.close()
    pc = capi.Juliet(0)
    remapped, pos = assemble_whole(pc, ctxs, table)
    check_cells(name + " whole", pc, rows, pos, 0, n, 8 * ctxs[0].plane_stride)
    check_groups(name + " whole", pc, remapped, rows, table, 0, n)
    pc.close()
    close_all(ctxs)


# ------------------------------------------------------------------------------------------------ every field and every read's id
def assert_result(what, got, exp, nv):
    assert got["summary"] == exp["summary"], (what, got["summary"], exp["summary"])
    h = exp["summary"]["n_haplotypes"]
    for k in ("pos_cols", "hap_count", "hap_pattern"):
        g = np.asarray(got[k])
        assert g.shape == exp[k].shape and (g == exp[k]).all(), (what, k)
    assert np.asarray(got["hit"]).shape == (nv, h) and (got["hit"] == exp["hit"]).all(), (what, "hit")
    assert np.asarray(got["cooc"]).shape == (nv, nv) and (got["cooc"] == exp["cooc"]).all(), (what, "cooc")
    if "read_hap" in got and got["read_hap"] is not None and len(got["read_hap"]) == len(exp["read_hap"]):
        ids = np.asarray(got["read_hap"])
        assert (ids == exp["read_hap"]).all(), (what, "read_hap", np.flatnonzero(ids != exp["read_hap"])[:8].tolist())


@pytest.mark.parametrize("shards", [1, 2, 3, 8])
@pytest.mark.parametrize("group", ["SELECTION", "POSITIONS", "TABLES"])
def test_cases_sharded_on_one_device(group, shards):
    """capi.phase_sharded_by_reads with the case's host table: slice assembly, exporting run, host merge and selection, ids from
    jl_phase_regroup.  (The width jl_phase_regroup stores the ids at shows nowhere in the public API: the ids themselves pin it —
    the reads of haplotype 14 of 15, or 254 of 255, come back insufficient from ids one step too narrow.)"""
    for name in getattr(xe, group):
        sp = xe.spread(xe.CASES[name], shards)
        exp = sp.expected()
        ctxs = upload_windows(sp.rows, sp.windows())
        got, pos_global = capi.phase_sharded_by_reads(ctxs, sp.table, shards, min_reads=sp.min_reads)
        assert got is not None and len(got["read_hap"]) == len(sp.rows), name
        assert_result((name, shards), got, exp, len(sp.table))
        assert (pos_global == exp["pos_cols"]).all()
        close_all(ctxs)
        COMPARED["sharded"].add((name, shards))


def run_windows(rows, wins, which, min_reads):
    """The call stage of the windows `which` (indices into wins): one gene in frame over the whole reference, the background as
    reference."""
    l = rows.shape[1]
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ctxs = []
    for w in which:
        b, k = wins[w]
        c = capi.Juliet(0)
        c.upload_rows(rows[:, b:b + k], win_begin=b)
        c.run_async(genes, pe.background(l), LOOSE, None, False, min_reads, False)
        ctxs.append(c)
    return ctxs


def one_rank_comm(ctx):
    idbuf = np.zeros(128, dtype=np.uint8)
    assert ctx.lib.jl_comm_unique_id(idbuf.ctypes.data_as(C.c_void_p)) == 0
    comm = C.c_void_p()
    ctx._chk(ctx.lib.jl_comm_create(ctx.h, idbuf.ctypes.data_as(C.c_void_p), 0, 1, C.byref(comm)))
    return comm


def assert_session(what, res, called, exp):
    m = res["merged"]
    assert m["col"].tolist() == called["col"].tolist() and m["codon"].tolist() == called["codon"].tolist(), what
    assert_result(what, res, exp, len(called))
    h, vp = exp["summary"]["n_haplotypes"], exp["summary"]["n_positions"]
    assert res["read_hap_bits"] == pe.id_bits(h, vp), (what, res["read_hap_bits"], h)


WHOLE_PATH = [n for n in xe.CASES if xe.CASES[n].whole_path]


@pytest.mark.parametrize("with_comm", [False, True])
@pytest.mark.parametrize("group", ["SELECTION", "POSITIONS", "TABLES"])
def test_cases_through_a_one_rank_session(group, with_comm):
    anchor = capi.Juliet(0)                  # one communicator for the group's sessions (creating one takes most of a second)
    comm = one_rank_comm(anchor) if with_comm else None
    try:
        _one_rank_sessions(group, with_comm, comm)
    finally:
        if comm is not None:
            anchor.lib.jl_comm_destroy(comm)
        anchor.close()


def _one_rank_sessions(group, with_comm, comm):
    for name in [n for n in getattr(xe, group) if n in WHOLE_PATH]:
        c = xe.CASES[name]
        called = c.called()
        sp = xe.spread(c, 1, table=called)
        exp = sp.expected()
        n = len(sp.rows)
        wins = sp.windows()
        ctxs = run_windows(sp.rows, wins, range(len(wins)), sp.min_reads)
        xw = capi.Xwin(ctxs, [b for b, _ in wins], [k for _, k in wins], [0] * len(wins), [0, n], comm)
        try:
            for rep in range(2):
                res = xw.phase(sp.min_reads)
                assert_session((name, with_comm, rep), res, called, exp)
                assert len(res["read_hap"]) == n
                if name in ("lds-1024", "lds-1025"):      # no growth and the by-value table / a grown block and the table through HBM
                    assert res["n_groups"] == int(name[4:]) == len(exp["group_counts"]), (name, res["n_groups"])
        finally:
            xw.close()
        close_all(ctxs)
        COMPARED["session"].add((name, with_comm))


def session_in_ranks(name, world, sp, wins, win_rank, called, exp):
    n = len(sp.rows)
    idbuf = np.frombuffer(np.random.default_rng(n * 7 + world).bytes(128), dtype=np.uint8).copy()

    def body(rank):
        ctxs = run_windows(sp.rows, wins, [w for w in range(len(wins)) if win_rank[w] == rank], sp.min_reads)
        comm = C.c_void_p()
        ctxs[0]._chk(ctxs[0].lib.jl_comm_create_inproc(ctxs[0].h, idbuf.ctypes.data_as(C.c_void_p), rank, world, C.byref(comm)))
        xw = capi.Xwin(ctxs, [b for b, _ in wins], [k for _, k in wins], win_rank, sp.bounds, comm)
        try:
            return [xw.phase(sp.min_reads) for _ in range(2)]
        finally:
            xw.close()
            ctxs[0].lib.jl_comm_destroy(comm)
            close_all(ctxs)

    outs = ranks_in_threads(world, body, limit=60.0)
    for rep in range(2):
        ids = np.full(n, 0xABCD, dtype=np.uint16)
        for rank in range(world):
            r = outs[rank][rep]
            assert_session((name, world, rank, rep), r, called, exp)
            b, cnt = r["slice"]
            assert (b, cnt) == (sp.bounds[rank], sp.bounds[rank + 1] - sp.bounds[rank]) and len(r["read_hap"]) == cnt
            ids[b:b + cnt] = r["read_hap"]
        assert (ids == exp["read_hap"]).all(), (name, world, rep, np.flatnonzero(ids != exp["read_hap"])[:8].tolist())


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("group", ["SELECTION", "POSITIONS"])
def test_cases_through_sessions_of_several_ranks(group, world):
    for name in [n for n in getattr(xe, group) if n in WHOLE_PATH]:
        c = xe.CASES[name]
        called = c.called()
        sp = xe.spread(c, world, table=called, min_cols=6 * world)      # (no window narrower than a codon)
        wins = sp.windows(world)
        assert len(wins) == world and min(k for _, k in wins) >= 3, (name, wins)
        session_in_ranks(name, world, sp, wins, list(range(world)), called, sp.expected())
        COMPARED["ranks"].add((name, world))


def test_nine_ranks_take_the_second_chunk_of_destinations():
    c = xe.CASES["vp20"]
    called = c.called()
    n = 9 * 256 + 5
    sp = xe.spread(c, 9, table=called, n_min=n, bounds=[256 * s for s in range(9)] + [n])
    assert len(sp.rows) == n and xe.DST_MAX == 8
    wins = sp.windows(9)
    assert len(wins) == 9
    session_in_ranks("vp20 x9", 9, sp, wins, list(range(9)), called, sp.expected())


@pytest.mark.parametrize("name", ["rows-256", "rows-257"])
def test_table_blocks_of_a_rank_with_many_rows(name):
    c = xe.CASES[name]
    called = c.called()
    l = c.build()[0].shape[1]
    sp = xe.spread(c, 2, table=called, min_cols=l + 5)
    wins = [(0, l - 1), (l - 1, 6)]          # every row on rank 0; rank 1 holds two codons of the background and no position
    assert (l - 1) % 3 == 0 and sp.rows.shape[1] == l + 5 and len(called) == int(name[5:])
    session_in_ranks(name, 2, sp, wins, [0, 1], called, sp.expected())


def test_a_position_no_window_holds_whole_is_refused():
    """Non-overlapping windows cut at column 12 and a codon at 10: both assemblies answer JL_ERR_ARG.  (A session cannot meet it
    with an honest layout: every codon a window calls lies whole inside that window; jl_xwin_create refuses a layout that does
    not describe the contexts.)"""
    rows = xe.pack_rows(600)
    table = pe.table_of([(3, 0), (10, 0), (15, 0)])
    ctxs = upload_windows(rows, xe.PACK_WINDOWS)
    pc = capi.Juliet(0)
    with pytest.raises(capi.JulietError) as e:
        pc.xwin_assemble_slice_local(ctxs, table, 0, 600)
    assert e.value.status == xe.ERR_ARG and "not fully inside any window" in str(e.value)
    with pytest.raises(capi.JulietError) as e:
        assemble_whole(pc, ctxs, table)
    assert e.value.status == xe.ERR_ARG and "not fully inside any window" in str(e.value)
    with pytest.raises(capi.JulietError) as e:
        capi.Xwin(ctxs, [0, 10], [12, 12], [0, 0], [0, 600])
    assert e.value.status == xe.ERR_ARG
    pc.close()
    close_all(ctxs)


def test_every_case_was_compared():
    """No case is skipped or sampled: the tests above compared every case on every route it can take (deselected ones run here)."""
    for shards in (1, 2, 3, 8):
        for group in ("SELECTION", "POSITIONS", "TABLES"):
            if not all((n, shards) in COMPARED["sharded"] for n in getattr(xe, group)):
                test_cases_sharded_on_one_device(group, shards)
    for with_comm in (False, True):
        for group in ("SELECTION", "POSITIONS", "TABLES"):
            if not all((n, with_comm) in COMPARED["session"] for n in getattr(xe, group) if n in WHOLE_PATH):
                test_cases_through_a_one_rank_session(group, with_comm)
    assert COMPARED["sharded"] == {(n, s) for n in xe.CASES for s in (1, 2, 3, 8)}
    assert COMPARED["session"] == {(n, w) for n in WHOLE_PATH for w in (False, True)} and len(WHOLE_PATH) == len(xe.CASES) - 1
