"""The designed cases of tests/xwin_edges.py, without a GPU: the mirrored constants are the library's; the library's host merge and
selection (jl_merge_groups, jl_select_haplotypes) give phase_edges.phase of the whole matrix for every case over 1, 2, 3 and 8
slices, every read's id included; the slice plan equals a numpy formula; window ownership; and the cases tell thirteen wrong
kernels and merges from the right ones.  tests/test_gpu_xwin_edges.py sends the same cases through the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import phase_edges as pe
import xwin_edges as xe
from minorseq_amd import capi, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minorseq_amd", "csrc")
SLICE_COUNTS = (1, 2, 3, 8)
FIELDS = ("hap_count", "hap_pattern", "hit", "cooc")


def source(name):
    with open(os.path.join(CSRC, name) if not name.startswith("include") else os.path.join(ROOT, name)) as f:
        return f.read()


def define(text, name):
    m = re.search(r"^\s*#\s*define\s+%s\s+(\d+)u?\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_mirrored_constants_are_the_librarys():
    internal, kern, host, merge, sched, api = (source(f) for f in ("jl_internal.h", "kernels_xwin.hip", "capi_xwin.hip", "capi_merge.hip",
                                                                    "xwin_schedule.h", "include/juliet_hip.h"))
    assert xe.POS_MAX == define(internal, "JL_XW_POS_MAX") and xe.DST_MAX == define(internal, "JL_XW_DST_MAX")
    assert xe.TAB_MAX == define(internal, "JL_XW_TAB_MAX")
    assert xe.GCAP0 == define(host, "JL_XW_GCAP0") and xe.XROWS0 == define(host, "JL_XW_XROWS0")
    assert "p0 += JL_XW_POS_MAX" in host and "d0 += JL_XW_DST_MAX" in host and "x->my_groups > JL_XW_TAB_MAX" in host
    assert xe.PACK_PIECES == int(re.search(r"constexpr uint32_t kPackPieces = (\d+);", kern).group(1))
    assert "off[k] = (((uint64_t)blockIdx.x * kPackPieces + k) * 256u + threadIdx.x) * 16u;" in kern
    assert xe.XBLOCK_BYTES == 16384 and "(max_stride + 16383u) / 16384u" in kern and xe.XBLOCK_READS == 131072 and xe.PIECE_READS == 128
    assert "if (off[k] + 16u >= bytes)" in kern and "const uint32_t pad = (j % 3u) == 0u ? 0u : 0xFFu;" in kern
    assert "d.tail_mask = (n_s & 7u) ? (1u << (n_s & 7u)) - 1u : 0xFFu;" in host
    assert "(slice_begin[s] & 255u)" in sched and xe.SLICE_ALIGN == 256
    assert "static inline uint64_t xwin_stride(uint64_t n_reads) { return (n_reads + 1023) / 1024 * 128; }" in sched and xe.LINE_READS == 1024
    assert xe.MERGE_WORD_MAX == int(re.search(r"const bool by_word = vp <= (\d+)u;", merge).group(1))
    assert xe.ERR_ARG == int(re.search(r"JL_ERR_ARG = (-\d+)", api).group(1))
    assert "x->bits = H <= JL_ID4_MAX_H ? 4u : (H <= JL_ID8_MAX_H ? 8u : 16u);" in host
    lib = capi.load_library()
    for n in xe.PACK_SMALL + xe.PACK_MORE + xe.PACK_BIG:
        assert lib.jl_plane_stride(n) * 8 == xe.stride_reads(n) and lib.jl_col_stride(n) * 2 == xe.shown_reads(n)
    # the shapes: every value of n & 7; 1, 15, 16 and 17 bytes mod 16; the row's last byte in x-block 0, and in x-block 1 at offsets 0 and 1
    assert {n & 7 for n in xe.PACK_SMALL} == {0, 1, 7} and {n & 7 for n in xe.PACK_SMALL + xe.PACK_MORE} == set(range(8))
    assert {-(-n // 8) for n in (1, 115, 121, 127, 128, 129)} == {1, 15, 16, 17} and {-(-n // 8) % 16 for n in (1023, 1024, 1025)} == {0, 1}
    assert xe.PACK_BIG[:4] == (131072, 131073, 131080, 131081) and [(-(-n // 8) - 1) // xe.XBLOCK_BYTES for n in xe.PACK_BIG] == [0, 1, 1, 1, 2]
    assert [((-(-n // 8) - 1) % xe.XBLOCK_BYTES, n & 7) for n in xe.PACK_BIG[:4]] == [(xe.XBLOCK_BYTES - 1, 0), (0, 1), (0, 0), (1, 1)]
    for n in xe.PACK_SMALL + xe.PACK_MORE + xe.PACK_BIG:
        for b, k, total in xe.pack_slices(n):
            assert b % xe.SLICE_ALIGN == 0 and k == n and b + k <= total
        assert {b > 0 for b, _, _ in xe.pack_slices(n)} == {False, True} and {b + k == t for b, k, t in xe.pack_slices(n)} == {False, True}


# ------------------------------------------------------------------------------------------------ merge + selection on the host
def remapped_table(table, n_cols):
    """The table on the compact matrix: col = 3 * index of its position."""
    pos = xe.positions_of(table, n_cols)
    out = table.copy()
    out["col"] = 3 * np.searchsorted(pos, table["col"])
    return out, 3 * np.arange(len(pos), dtype=np.uint32)


def library_sharded(sp):
    """The case's slices through jl_merge_groups and jl_select_haplotypes; the ids through hap_of_merged[index[s]][group of read]."""
    tabs = [xe.slice_groups(sp.rows, sp.table, sp.bounds[s], sp.bounds[s + 1]) for s in range(sp.n_slices)]
    patterns, counts, index = sharding.merge_groups(tabs)
    remapped, pos_cols = remapped_table(sp.table, sp.rows.shape[1])
    got = sharding.select_haplotypes(patterns, counts, remapped, pos_cols, sp.min_reads, [t["summary"] for t in tabs])
    ids = np.full(len(sp.rows), pe.HAP_DAMAGED, np.uint16)
    for s, t in enumerate(tabs):
        mine = ids[sp.bounds[s]:sp.bounds[s + 1]]
        ok = t["index"] >= 0
        mine[ok] = got["hap_of_merged"][index[s]][t["index"][ok]].astype(np.uint16)
    got["read_hap"] = ids
    return got, tabs, len(counts)


def assert_equal(got, exp, what):
    assert got["summary"] == exp["summary"], (what, got["summary"], exp["summary"])
    for k in FIELDS + ("read_hap",):
        assert got[k].shape == exp[k].shape and (got[k] == exp[k]).all(), (what, k)


@pytest.fixture(scope="module")
def spreads():
    return {}


def spread_of(spreads, name, n_slices):
    if (name, n_slices) not in spreads:
        spreads[(name, n_slices)] = xe.spread(xe.CASES[name], n_slices)
    return spreads[(name, n_slices)]


@pytest.mark.parametrize("group", ["SELECTION", "POSITIONS", "TABLES"])
def test_host_merge_and_selection_equal_the_whole_matrix(spreads, group):
    lib = capi.load_library()
    for name in getattr(xe, group):
        for n_slices in SLICE_COUNTS:
            sp = spread_of(spreads, name, n_slices)
            assert len(sp.rows) >= 256 * (n_slices - 1) + 1 and len(sp.bounds) == n_slices + 1
            exp = sp.expected()
            got, tabs, m = library_sharded(sp)
            assert_equal(got, exp, (name, n_slices, "library"))
            mirror = xe.sharded(sp.rows, sp.table, sp.min_reads, sp.bounds)
            assert_equal(mirror, exp, (name, n_slices, "mirror"))
            assert mirror["id_bits"] == pe.id_bits(exp["summary"]["n_haplotypes"], exp["summary"]["n_positions"]) and mirror["n_merged"] == m
            if n_slices == 3 and m > 1:      # cap one below the merged count: the overflow status, n_merged still the true count
                vp = exp["summary"]["n_positions"]
                pats = [np.ascontiguousarray(t["patterns"]) for t in tabs]
                cnts = [np.ascontiguousarray(t["counts"]) for t in tabs]
                pp = (C.c_void_p * 3)(*[p.ctypes.data if p.size else None for p in pats])
                cp = (C.c_void_p * 3)(*[c.ctypes.data if len(c) else None for c in cnts])
                strides = np.full(3, vp, np.uint32)
                ng = np.array([len(c) for c in cnts], np.uint32)
                mp, mc, n_merged = np.zeros((m - 1) * vp, np.uint8), np.zeros(m - 1, np.uint64), C.c_uint32()
                rc = lib.jl_merge_groups(pp, capi._p(strides), cp, capi._p(ng), 3, vp, capi._p(mp), capi._p(mc), m - 1, C.byref(n_merged), None)
                assert (rc, n_merged.value) == (pe.ERR_OVERFLOW, m), (name, rc, n_merged.value)


def test_cases_sit_on_the_edges_their_names_say(spreads):
    assert len(xe.CASES) == 32 and set(xe.REUSED) <= set(pe.CASES)
    vp_of = {n: xe.spread(xe.CASES[n], 1).expected()["summary"]["n_positions"] for n in xe.POSITIONS}
    assert [vp_of[n] for n in ("vp8", "vp9", "vp10", "vp11", "vp20", "vp21", "vp30", "vp31", "vp41", "pos-48", "pos-49")] == [8, 9, 10, 11, 20, 21, 30, 31, 41, 48, 49]
    for name, rows_ in (("rows-256", 256), ("rows-257", 257)):
        c = xe.CASES[name]
        assert len(c.build()[1]) == len(c.called()) == rows_
    for name in ("pos-48", "pos-49", "rows-256", "rows-257", "split-minreads"):      # the new cases: the host table is what the call stage gives
        c = xe.CASES[name]
        if c.whole_path:
            assert [(int(r["col"]), int(r["codon"])) for r in c.called()] == [(int(r["col"]), int(r["codon"])) for r in c.build()[1]], name
    # split-minreads: fewer than min_reads in every slice, exactly min_reads in all; the neighbour one short
    sp = spread_of(spreads, "split-minreads", 3)
    tabs = [xe.slice_groups(sp.rows, sp.table, sp.bounds[s], sp.bounds[s + 1]) for s in range(3)]
    assert all(sorted(t["counts"].tolist())[:-1] in ([2, 2], [1, 2]) for t in tabs) and sp.min_reads == 6
    e = sp.expected()
    assert e["hap_count"].tolist() == [len(sp.rows) - 11, 6] and e["summary"]["insufficient_reads"] == 5
    # split-ties: no two slices agree on the counts, the merged ones are 9, 9 and 9; order of appearance C, B, A against the pattern order
    sp = spread_of(spreads, "split-ties", 3)
    e = sp.expected()
    assert e["hap_count"].tolist()[1:] == [9, 9, 9] and e["hap_pattern"][1:, 0].tolist() == [5, 21, 63]
    per_slice = [xe.slice_groups(sp.rows, sp.table, 256 * s, 256 * s + 256) for s in range(3)]
    assert [[(p, k) for p, k in zip(t["patterns"][:, 0].tolist(), t["counts"].tolist()) if p != 27] for t in per_slice] == [[(63, 5)], [(21, 6), (63, 4)], [(5, 9), (21, 3)]]
    # the id widths on the merged count, the name capacity, the session's blocks
    h_of = {n: spread_of(spreads, n, 3).expected()["summary"]["n_haplotypes"] for n in xe.CASES if n.startswith("haps-")}
    assert h_of == {"haps-14": 14, "haps-15": 15, "haps-254": 254, "haps-255": 255, "haps-702": 702, "haps-703": 702}
    for name, groups in (("lds-1024", 1024), ("lds-1025", 1025), ("lds-1026", 1026)):
        assert len(spread_of(spreads, name, 1).expected()["group_counts"]) == groups
    assert (xe.GCAP0, xe.TAB_MAX) == (1024, 1024)


# ------------------------------------------------------------------------------------------------ the slice plan
def plan_formula(k_begin, k_count, slice_begin, world, rank):
    """The ops of `rank` in issue order: its own slice, then per peer (ascending) the send and the receive."""
    def op(kind, peer, owner, receiver):
        n = slice_begin[receiver + 1] - slice_begin[receiver]
        stride = -(-n // 1024) * 128
        return dict(op=kind, peer=peer, k_begin=k_begin[owner], k_count=k_count[owner], read_begin=slice_begin[receiver], n_reads=n,
                    dst_stride=stride, bytes=9 * k_count[owner] * stride, dst_offset=9 * k_begin[owner] * stride)
    n_mine = slice_begin[rank + 1] - slice_begin[rank]
    ops = [op(capi.XWIN_OP_LOCAL, rank, rank, rank)] if k_count[rank] and n_mine else []
    for s in range(world):
        if s != rank:
            if k_count[rank] and slice_begin[s + 1] > slice_begin[s]:
                ops.append(op(capi.XWIN_OP_SEND, s, rank, s))
            if k_count[s] and n_mine:
                ops.append(op(capi.XWIN_OP_RECV, s, s, rank))
    return ops


@pytest.mark.parametrize("world", [1, 2, 9])
def test_slice_plan_equals_the_formula(world):
    table = pe.table_of([(c, 0) for c in (0, 3, 30, 33, 36, 90)] + [(30, 63)])
    pos = np.unique(table["col"]).tolist()
    sizes = (1, 1023, 1024, 1025, 131072, 131073)
    for variant in range(3):
        # windows of 12 columns, one per rank (world 9: ranks 1, 4.. hold no position); variant 1: two windows on rank 0; variant 2: ranks without reads
        n_windows = max(world, 8) + (variant == 1)
        wb = [12 * w for w in range(n_windows)]
        wn = [12] * n_windows
        wr = [min(world - 1, max(0, w - (variant == 1))) for w in range(n_windows)]
        sb = [0]
        for s in range(world):
            n = sizes[(s + variant) % len(sizes)] if not (variant == 2 and s % 2) else 0
            sb.append(sb[-1] + (n if s == world - 1 or n == 0 else -(-n // 256) * 256))
        owner = [next(w for w in range(n_windows) if wb[w] <= c and c + 3 <= wb[w] + wn[w]) for c in pos]
        k_count = [sum(1 for w in owner if wr[w] == r) for r in range(world)]
        k_begin = [next((k for k, w in enumerate(owner) if wr[w] == r), 0) for r in range(world)]
        if world > 2:
            assert 0 in k_count
        plans = [capi.xwin_slice_plan(wb, wn, wr, table, sb, world, r) for r in range(world)]
        for r in range(world):
            assert plans[r] == plan_formula(k_begin, k_count, sb, world, r), (world, variant, r)
        sends = sorted((r, o["peer"], o["bytes"], o["read_begin"], o["n_reads"], o["k_begin"]) for r in range(world) for o in plans[r] if o["op"] == capi.XWIN_OP_SEND)
        recvs = sorted((o["peer"], r, o["bytes"], o["read_begin"], o["n_reads"], o["k_begin"]) for r in range(world) for o in plans[r] if o["op"] == capi.XWIN_OP_RECV)
        assert sends == recvs and (world == 1 or sends)
    # the slice sizes themselves, one rank
    for n in sizes:
        (o,) = capi.xwin_slice_plan([0], [96], [0], table, [0, n], 1, 0)
        assert (o["n_reads"], o["dst_stride"], o["bytes"], o["dst_offset"]) == (n, xe.stride_reads(n) // 8, 9 * len(pos) * (xe.stride_reads(n) // 8), 0)


def test_window_ownership():
    table = pe.table_of([(0, 0), (9, 0), (10, 0), (12, 0)])
    # overlapping windows [0, 14) and [10, 24): the codons at 10 and 9 lie whole in both / in the first: owned by the first
    _, pos, owner = capi.xwin_plan([0, 10], [14, 14], table)
    assert pos.tolist() == [0, 9, 10, 12] and owner.tolist() == [0, 0, 0, 1]
    # non-overlapping windows cut at 12: the codon at 10 lies across the cut
    remapped, pos, owner = capi.xwin_plan([0, 12], [12, 12], table)
    assert owner.tolist() == [0, 0, -1, 1] and remapped["col"].tolist() == [0, 3, 6, 9]
    with pytest.raises(capi.JulietError) as e:
        capi.xwin_slice_plan([0, 12], [12, 12], [0, 0], table, [0, 100], 1, 0)
    assert e.value.status == xe.ERR_ARG
    for name in xe.CASES:
        sp = xe.spread(xe.CASES[name], 1)
        wins = sp.windows()
        assert 2 <= len(wins) <= 3 and sum(k for _, k in wins) == sp.rows.shape[1], name
        _, pos, owner = capi.xwin_plan([b for b, _ in wins], [k for _, k in wins], sp.table)
        assert (owner >= 0).all() and pos.tolist() == xe.positions_of(sp.table, sp.rows.shape[1]).tolist(), name
    assert len(set(capi.xwin_plan(*zip(*xe.spread(xe.CASES["vp20"], 1).windows()), xe.CASES["vp20"].build()[1])[2].tolist())) == 3


# ------------------------------------------------------------------------------------------------ the wrong kernels
# the case (pack: the shape) that tells each wrong kernel from the right one; the test finds every one that does and requires these
PACK_CATCHES = {
    "no_tail_mask": "n_slice 9, from read 768, other reads behind",
    "pad_zero_all_planes": "n_slice 1, from read 0, ending at the last read",
    "leak_past_slice": "n_slice 129, from read 0, other reads behind",
    "drop_xblock1": "n_slice 131073, from read 0, ending at the last read",
    "line_tail_not_padded": "n_slice 121, from read 0, ending at the last read",
    "pos_chunk_offset": "pos-49",
    "dst_chunk_offset": "world 9",
}
MERGE_CATCHES = {
    "word_compare_past_8": "vp9", "threshold_before_merge": "split-minreads", "ties_by_table_order": "split-ties", "cap_701": "haps-702",
    "ids_4bit_at_15": "haps-15", "ids_8bit_at_255": "haps-255",
}


def shape_name(b, k, total):
    return "n_slice %d, from read %d, %s" % (k, b, "ending at the last read" if b + k == total else "other reads behind")


def test_pack_shapes_tell_wrong_kernels_from_the_right_one():
    table = xe.pack_table()
    caught = {w: [] for w in xe.PACK_WRONG}
    seen_by_download = {}
    for n in xe.PACK_SMALL + xe.PACK_MORE + xe.PACK_BIG[:2]:
        for b, k, total in xe.pack_slices(n):
            rows = xe.pack_rows(total)
            right = xe.pack_expected(rows, xe.PACK_POS, b, k, xe.stride_reads(k))
            assert (right[:k] == rows[b:b + k][:, [c + j for c in xe.PACK_POS for j in range(3)]]).all() and (right[k:] == 6).all()
            for w in ("no_tail_mask", "pad_zero_all_planes", "leak_past_slice", "drop_xblock1", "line_tail_not_padded"):
                wrong = xe.pack_expected(rows, xe.PACK_POS, b, k, xe.stride_reads(k), wrong=w)
                shown = xe.shown_reads(k)              # what a download shows of the plane rows
                if (wrong[:shown] != right[:shown]).any():
                    caught[w].append(shape_name(b, k, total))
                elif (wrong != right).any():
                    seen_by_download.setdefault(w, []).append(shape_name(b, k, total))
    # the chunk loops: 49 positions on one rank; nine destinations
    for name in ("pos-48", "pos-49"):
        rows, t = xe.CASES[name].build()
        pos = xe.positions_of(t, rows.shape[1])
        right = xe.pack_expected(rows, pos, 0, len(rows), xe.stride_reads(len(rows)))
        if (xe.pack_expected(rows, pos, 0, len(rows), xe.stride_reads(len(rows)), wrong="pos_chunk_offset") != right).any():
            caught["pos_chunk_offset"].append(name)
    for world in (8, 9):
        rows = xe.pack_rows(256 * world + 5)
        sb = sharding.read_slices(len(rows), world + 1)[:world] + [len(rows)] if world == 8 else [256 * s for s in range(9)] + [len(rows)]
        slices = [(sb[s], sb[s + 1] - sb[s]) for s in range(world)]
        for d, (b, k) in enumerate(slices):
            right = xe.pack_expected(rows, xe.PACK_POS, b, k, xe.stride_reads(k))
            if (xe.pack_expected(rows, xe.PACK_POS, b, k, xe.stride_reads(k), wrong="dst_chunk_offset", dst=d, slices=slices) != right).any():
                caught["dst_chunk_offset"].append("world %d" % world)
    for w in xe.PACK_WRONG:
        print("%-22s caught by %d: %s" % (w, len(caught[w]), "; ".join(sorted(set(caught[w]))[:6])))
        assert PACK_CATCHES[w] in caught[w], (w, caught[w])
    assert "pos-48" not in caught["pos_chunk_offset"] and "world 8" not in caught["dst_chunk_offset"]
    # What a download does not show.  A plane row is whole 1024-read lines, a download shows whole 256-read lines: a kernel that
    # leaves the pieces past the slice's last unwritten is seen by the download wherever the slice ends in the first half of a
    # 256-read line (above), and where it is not — 129 reads — the difference lies in reads 256.. of the line alone.  Nothing
    # reads those: every phasing kernel cuts the reads at n_reads (kernels_phase.hip valid_reads8), so no summary can show them.
    assert "n_slice 129, from read 0, ending at the last read" in seen_by_download["line_tail_not_padded"]
    assert "if (t * 8u + r < n_reads) valid |= 1u << (4 * r);" in source("kernels_phase.hip")


def test_cases_tell_wrong_merges_from_the_right_one(spreads):
    caught = {w: [] for w in xe.MERGE_WRONG}
    for name in xe.CASES:
        sp = spread_of(spreads, name, 3)
        exp = sp.expected()
        for w in xe.MERGE_WRONG:
            e = xe.sharded(sp.rows, sp.table, sp.min_reads, sp.bounds, wrong=w)
            same = e["summary"] == exp["summary"] and all(e[k].shape == exp[k].shape and (e[k] == exp[k]).all() for k in FIELDS + ("read_hap",))
            if not same or e["id_bits"] != pe.id_bits(exp["summary"]["n_haplotypes"], exp["summary"]["n_positions"]):
                caught[w].append(name)
    for w in xe.MERGE_WRONG:
        print("%-22s caught by %d cases: %s" % (w, len(caught[w]), " ".join(caught[w])))
        assert MERGE_CATCHES[w] in caught[w], (w, caught[w])
    assert "vp8" not in caught["word_compare_past_8"] and "haps-14" not in caught["ids_4bit_at_15"] and "haps-254" not in caught["ids_8bit_at_255"]
