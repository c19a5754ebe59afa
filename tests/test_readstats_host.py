"""The host-only half of the per-read counters (docs/SPEC.md §20): the numpy mirror on a matrix small enough to count by hand,
jl_read_filter against the mirror on rows designed around every bound, the launch shape's invariants, and what the library refuses.
No GPU: the library only has to load."""
import ctypes as C

import numpy as np
import pytest

import readstats_mirror as rm
import readstats_shape
from minorseq_amd import capi

NAMES = ("jl_read_stats_async", "jl_read_stats_fetch", "jl_read_filter")


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
HAND_ROWS = np.array([
    [0, 1, 2, 3, 0, 0, 0, 0],      # the compare row where it is one, bases throughout
    [1, 1, 4, 5, 6, 3, 2, 2],      # every kind of cell
    [6, 6, 6, 6, 6, 6, 6, 6],      # covers nothing
    [4, 4, 4, 4, 4, 4, 4, 4],      # deleted throughout
    [5, 0, 5, 0, 5, 0, 5, 0],      # N on the even columns, A on the odd ones
    [3, 2, 1, 0, 3, 2, 1, 6],      # a base that differs wherever the column is compared
], dtype=np.uint8)
HAND_COMPARE = np.array([0, 1, 2, 3, 4, 5, 0, 0xFF], dtype=np.uint8)   # columns 0..3 and 6 are compared
HAND_STATS = {
    rm.BASES: [8, 5, 0, 0, 4, 7],
    rm.GAPS: [0, 1, 0, 8, 0, 0],
    rm.MASKED: [0, 1, 0, 0, 4, 0],
    rm.COMPARED: [5, 3, 0, 0, 2, 5],
    rm.MISMATCHES: [0, 2, 0, 0, 2, 5],
}


def test_mirror_on_the_hand_counted_matrix():
    got = rm.stats(HAND_ROWS, HAND_COMPARE)
    assert got.dtype == np.uint32 and got.shape == (5, 6)
    for k, exp in HAND_STATS.items():
        assert got[k].tolist() == exp, k
    none = rm.stats(HAND_ROWS)                                  # no compare row: nothing is compared
    assert (none[:3] == got[:3]).all() and not none[3:].any()
    assert rm.consensus(HAND_ROWS).tolist() == [0, 1, 4, 0, 0, 0, 0, 0]
    assert rm.column_counts(HAND_ROWS)[2].tolist() == [0, 1, 1, 0, 2, 1]


# ---------------------------------------------------------------------------------------------- jl_read_filter
def table(*reads):
    """stats[5, n] from (bases, gaps, masked, compared, mismatches) per read."""
    return np.ascontiguousarray(np.array(reads, dtype=np.uint32).T)


def same_as_mirror(st, **rule):
    idx, failed = capi.read_filter(st, **rule)
    exp_idx, exp_failed = rm.read_filter(st, **rule)
    assert idx.dtype == np.uint32 and idx.tolist() == exp_idx.tolist(), (rule, idx, exp_idx)
    assert failed.tolist() == exp_failed.tolist(), (rule, failed, exp_failed)
    return idx.tolist(), failed.tolist()


def test_exports_and_struct():
    lib = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert C.sizeof(capi.ReadRule) == 32
    assert capi.READ_STATS == 5 and len(capi.READ_RULES) == 5
    assert hasattr(capi.Juliet, "read_stats") and callable(capi.read_filter)


def test_each_rule_at_its_bound_and_one_past():
    #             bases gaps masked compared mismatches
    st = table((10, 0, 0, 10, 0), (9, 0, 0, 9, 0))
    assert same_as_mirror(st, min_bases=10) == ([0], [1, 0, 0, 0, 0])
    st = table((50, 0, 0, 50, 3), (50, 0, 0, 50, 4))
    assert same_as_mirror(st, max_mismatches=3) == ([0], [0, 1, 0, 0, 0])
    assert same_as_mirror(st, max_mismatches=0) == ([], [0, 2, 0, 0, 0])
    st = table((100, 0, 0, 100, 2), (100, 0, 0, 100, 3), (150, 0, 0, 150, 3), (149, 0, 0, 149, 3))
    assert same_as_mirror(st, max_mismatch_perc=2.0) == ([0, 2], [0, 0, 2, 0, 0])
    st = table((95, 5, 7, 0, 0), (94, 6, 7, 0, 0))              # (the masked cells are not part of the gap rule's denominator)
    assert same_as_mirror(st, max_gap_perc=5.0) == ([0], [0, 0, 0, 1, 0])
    st = table((90, 9, 1, 0, 0), (90, 8, 2, 0, 0))              # (the gaps are part of the N rule's)
    assert same_as_mirror(st, max_masked_perc=1.0) == ([0], [0, 0, 0, 0, 1])
    # a bound that is no binary fraction: the products decide, in double, as the mirror forms them
    st = table((1000, 0, 0, 1000, 1), (1000, 0, 0, 1000, 2), (3000, 0, 0, 3000, 3), (2999, 0, 0, 2999, 3))
    same_as_mirror(st, max_mismatch_perc=0.1)
    same_as_mirror(st, max_mismatch_perc=0.3)
    # both ends of the accepted range
    st = table((10, 0, 0, 10, 0), (10, 0, 0, 10, 1), (10, 0, 0, 10, 10))
    assert same_as_mirror(st, max_mismatch_perc=0.0)[0] == [0]
    assert same_as_mirror(st, max_mismatch_perc=100.0)[0] == [0, 1, 2]


def test_nothing_compared_passes_a_percentage_rule():
    st = table((40, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 3, 0, 0, 0))
    assert same_as_mirror(st, max_mismatch_perc=0.0, max_gap_perc=100.0, max_masked_perc=0.0) == ([0, 1, 2], [0, 0, 0, 0, 0])
    assert same_as_mirror(st, max_gap_perc=0.0) == ([0, 1], [0, 0, 0, 1, 0])      # 0 <= 0 is kept; 300 <= 0 is not


def test_every_rule_disabled_keeps_every_read():
    rng = np.random.default_rng(5)
    st = rng.integers(0, 3000, size=(5, 257), dtype=np.uint32)
    st[:, 0] = 0
    st[:, 1] = 0xFFFFFFFF
    idx, failed = same_as_mirror(st)
    assert idx == list(range(257)) and failed == [0] * 5


def test_a_read_failing_three_rules_counts_three_times():
    st = table((5, 60, 0, 5, 5), (100, 0, 0, 100, 0))
    idx, failed = same_as_mirror(st, min_bases=10, max_mismatches=4, max_mismatch_perc=50.0, max_gap_perc=50.0, max_masked_perc=50.0)
    assert idx == [1] and failed == [1, 1, 1, 1, 0] and sum(failed) == 4
    idx, failed = same_as_mirror(st, min_bases=10, max_mismatches=4, max_gap_perc=50.0)
    assert idx == [1] and failed == [1, 1, 0, 1, 0] and sum(failed) == 3


def test_seeded_tables_against_the_mirror():
    rng = np.random.default_rng(11)
    for n in (1, 2, 1000):
        b, g, m = (rng.integers(0, 400, size=n, dtype=np.uint32) for _ in range(3))
        c = (b * rng.random(n)).astype(np.uint32)
        x = (c * rng.random(n) * 0.2).astype(np.uint32)
        st = np.stack([b, g, m, c, x])
        same_as_mirror(st, min_bases=100, max_mismatches=20, max_mismatch_perc=7.5, max_gap_perc=60.0, max_masked_perc=55.5)
        same_as_mirror(st, max_mismatch_perc=10.0)


def test_argument_refusals():
    lib = capi.load_library()
    st = table((10, 0, 0, 10, 0), (9, 0, 0, 9, 1))
    idx, kept, failed = np.full(2, 77, dtype=np.uint32), C.c_uint64(99), np.full(5, 55, dtype=np.uint64)

    def call(s=st.ctypes.data, n=2, r=capi.read_rule(), i=idx.ctypes.data, k=C.byref(kept), f=failed.ctypes.data):
        return lib.jl_read_filter(s, n, C.byref(r) if r is not None else None, i, k, f)

    def refused(word, **kw):
        assert call(**kw) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)
        assert idx.tolist() == [77, 77] and kept.value == 99 and failed.tolist() == [55] * 5      # a refused call writes nothing

    refused("NULL", s=None)
    refused("NULL", r=None)
    refused("NULL", i=None)
    refused("NULL", k=None)
    refused("above 100", r=capi.read_rule(max_mismatch_perc=100.0001))
    refused("above 100", r=capi.read_rule(max_gap_perc=1e9))
    refused("above 100", r=capi.read_rule(max_masked_perc=float("nan")))
    refused("32 bits", n=2**32)
    assert call(f=None) == 0 and kept.value == 2 and idx.tolist() == [0, 1]       # failed may be NULL
    assert call(n=0) == 0 and kept.value == 0
    with pytest.raises(capi.JulietError) as e:
        capi.read_filter(st, max_gap_perc=101.0)
    assert e.value.status == -1


def test_stage_refused_without_a_matrix():
    """With a device: a context without a matrix is a state error, and so is a fetch.  Without one no context exists (the loud
    refusal of test_capi_exports.py), and the entry points refuse the NULL context."""
    lib = capi.load_library()
    if lib.jl_device_count() > 0:
        j = capi.Juliet(0)
        assert lib.jl_read_stats_async(j.h, None) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
        assert lib.jl_read_stats_fetch(j.h, None) == -4
        j.close()
    else:
        with pytest.raises(capi.JulietError) as e:
            capi.Juliet(0)
        assert e.value.status == -2
        assert lib.jl_read_stats_async(None, None) == -1 and lib.jl_read_stats_fetch(None, None) == -1


# ---------------------------------------------------------------------------------------------- the launch shape
def test_shape_invariants():
    for n_reads in (1, 31, 2047, 2048, 2049, 100_000, 2**22, 2**31 - 1):
        for n_cols in (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 3000, 100_000, 2**24):
            s = readstats_shape.shape(n_reads, n_cols)
            case = (n_reads, n_cols, s)
            assert s["wg_reads"] == 2048 and s["n_chunks"] == -(-n_reads // 2048), case
            assert 1 <= s["seg_cols"] <= readstats_shape.SEG_COLS_MAX == 255, case       # what a byte counter holds
            assert s["n_segs"] * s["seg_cols"] >= n_cols, case                           # every column is in a segment
            assert (s["n_segs"] - 1) * s["seg_cols"] < n_cols, case                      # ... in one, and no segment is empty
            assert s["seg_cols"] >= min(n_cols, readstats_shape.SEG_COLS_MIN), case
            assert 4 <= s["k"] <= 6 and s["flush"] == 2 ** s["k"] - 1, case
            assert s["combine"] in (0, 1), case
    # a short window is one segment; the bench window splits; so many reads that the chunks fill the chip: the longest segments
    assert readstats_shape.shape(97, 64)["n_segs"] == 1 and readstats_shape.shape(97, 127)["seg_cols"] == 64
    assert readstats_shape.shape(100_000, 3000)["n_segs"] > 1
    assert readstats_shape.shape(2**23, 3000)["seg_cols"] == 255
