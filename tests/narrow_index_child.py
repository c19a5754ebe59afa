"""Child process of tests/test_gpu_narrow_index.py (not a test module: the form of a launch depends on the process's environment
and on the library build, and a process loads one library — as tests/index_forms_child.py, whose helpers it uses).

    python narrow_index_child.py
    JL_LIB: the library to load (the -DJL_TUNING build: jl_tuning_group_forms_by_count)
    JL_NO_FOLD_CALL=1: the unfolded kernels (walk depth 2); without it the folded ones (walk depth 16)

The stored entry of the deviation index is 16 bits (csrc/deviation_index.h): a lane's round is one 8-byte load of four entries,
two to a dword, and a list begins on 8 bytes against its neighbour's end.  Every window below is run alone three times (run 1 from
the planes, run 2 with the build behind it, run 3 from the lists) and in a group of two windows three more times (launch 3 from the
lists); the index-form results must equal the plane-form run's bit for bit and the oracle's: column counts, codon histograms, the
variant table.  Prints NARROW-OK folded|unfolded as its last line.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import index_forms_child as ifc  # noqa: E402
import oracle_lib  # noqa: E402
from minorseq_amd import capi  # noqa: E402

CAP_VAR = 512


def padded(e):
    return (e + 3) & ~3


def parent_bytes(stride, n_cols, n_plain):
    """jl_index_info.bytes as the 4-byte entry had it: the allocation in entries (the smaller of the two bounds, + 4) x 4."""
    by_chunk = n_plain * padded(9 * stride // 8)
    by_total = padded(3 * n_cols * stride // 8)
    return (min(by_chunk, by_total) + 4) * 4


def planted_rows(n, lists, seed):
    """All reads equal the reference; chunk k has exactly lists[k] reads with one substitution in one of its three columns: three in
    four of them the same one (frequent enough to be called in the long lists), the others any."""
    rng = np.random.default_rng(seed)
    l = 3 * len(lists)
    ref = rng.integers(0, 4, l).astype(np.uint8)
    rows = np.tile(ref, (n, 1))
    for k, e in enumerate(lists):
        who = rng.choice(n, e, replace=False)
        same = rng.random(e) < 0.75
        col = np.where(same, 3 * k + 1, 3 * k + rng.integers(0, 3, e))
        rows[who, col] = (ref[col] + np.where(same, 1, 1 + rng.integers(0, 3, e))) % 4
    return rows.astype(np.uint8), ref, list(lists)


def every_code_rows(n, n_chunks, seed, share=0.10):
    """`share` of the reads, chosen per chunk, carry a code drawn from 0..6 (bases, gap, N, uncovered) in EVERY column of the chunk;
    the lists' lengths are counted from the rows (a draw of the reference's own three bases is no deviation)."""
    rng = np.random.default_rng(seed)
    l = 3 * n_chunks
    ref = rng.integers(0, 4, l).astype(np.uint8)
    rows = np.tile(ref, (n, 1))
    lists = []
    for k in range(n_chunks):
        who = np.flatnonzero(rng.random(n) < share)
        rows[np.ix_(who, np.arange(3 * k, 3 * k + 3))] = rng.integers(0, 7, (len(who), 3))
        for c in range(3 * k, 3 * k + 3):
            assert set(np.unique(rows[who, c])) == set(range(7)), (k, c)    # every code, in every column
        lists.append(int((rows[:, 3 * k:3 * k + 3] != ref[3 * k:3 * k + 3]).any(axis=1).sum()))
    return rows.astype(np.uint8), ref, lists


# name, reads, the chunk bound 9 x plane_stride / 8 at that many reads, the rows
WINDOWS = (
    # lists that end inside a dword (1, 3, 5), inside an 8-byte load (1, 2, 3, 5) or on one (0, 4), each against its neighbour's start
    ("adjacent", 1025, 288, lambda: planted_rows(1025, (0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0), 11)),
    # a round is 256 lanes x 4 entries
    ("round edge", 8192, 1152, lambda: planted_rows(8192, (1023, 1024, 1025, 0), 12)),
    # a batch of the unfolded kernels: 2 rounds
    ("unfolded batch edge", 15360, 2160, lambda: planted_rows(15360, (2047, 2048, 2049, 1), 13)),
    # a batch of the folded kernels: 16 rounds
    ("folded batch edge", 116000, 16416, lambda: planted_rows(116000, (16383, 16384, 16385, 3), 14)),
    ("every code", 8192, 1152, lambda: every_code_rows(8192, 4, 15)),
)


def snapshot(jl):
    jl.run_wait()
    v = jl.run_fetch(False, False, cap_var=CAP_VAR)
    assert len(v["variants"]) < CAP_VAR
    return v["variants"].copy(), jl.pileup_fetch()


def one_window(lib, orc, name, n, bound, rows, ref, lists, unfolded):
    l = rows.shape[1]
    stride = capi.load_library().jl_plane_stride(n)
    assert 9 * stride // 8 == bound and max(lists) <= bound and 12 <= l <= 36, (name, stride)
    genes = ifc.one_frame(l)
    prm = capi.default_params()
    a, b = capi.Juliet(0), capi.Juliet(0)
    try:
        a.upload_rows(rows)
        a.sync()
        a.run_async(genes, ref, prm, None, False, 10, False)
        planes = snapshot(a)
        assert a.index_info()["last_form"] == 0, name
        exp_hist, exp_cov = orc.codon_hist(rows, planes[1]["pos_col"])
        exp = (orc.pileup(rows), exp_hist, exp_cov, orc.call(rows, genes, refseq=ref))
        ifc.assert_oracle(exp, planes, (name, "planes"))
        a.run_async(genes, ref, prm, None, False, 10, False)
        a.run_wait()
        info = a.index_info(wait=True, chunk_flags=True)
        assert info["state"] == capi.INDEX_BUILT and info["plain_chunks"] == len(lists) and info["indexed_chunks"] == len(lists), (name, info)
        assert list(info["chunk_flags"][:len(lists)]) == [1] * len(lists) and info["entries"] == sum(lists), (name, info, lists)
        assert 2 * info["bytes"] == parent_bytes(stride, l, len(lists)), (name, info)      # exactly half of the 4-byte entry's
        a.run_async(genes, ref, prm, None, False, 10, False)
        single = snapshot(a)
        assert a.index_info()["last_form"] == 1, name
        ifc.assert_same(planes, single, (name, "single run from the index"))
        ifc.assert_oracle(exp, single, (name, "single run from the index"))
        # the same rows in a group of two windows: launches 1 and 2 from the planes (window b is a run behind), launch 3 from the lists
        b.upload_rows(rows)
        b.sync()
        grp = capi.Group([a, b])
        before = ifc.by_count(lib)
        for launch in range(3):
            grp.run_async(genes, ref, prm, False, 10, False)
            snaps = [snapshot(c) for c in (a, b)]
            forms = [c.index_info(wait=True)["last_form"] for c in (a, b)]
            assert forms == ([1, 1] if launch == 2 else [0, 0]), (name, launch, forms)
            for k, s in enumerate(snaps):
                ifc.assert_same(planes, s, (name, "group launch", launch, k))
                ifc.assert_oracle(exp, s, (name, "group launch", launch, k))
        took = [x - y for x, y in zip(ifc.by_count(lib), before)]
        assert took == ([0, 2, 0, 1] if unfolded else [2, 0, 1, 0]), (name, took)     # every launch was alone
        assert b.index_info(wait=True)["entries"] == sum(lists) and 2 * b.index_info()["bytes"] == parent_bytes(stride, l, len(lists)), name
        grp.close()
    finally:
        a.close()
        b.close()
    return len(exp[3])


def main():
    import ctypes as C

    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_group_forms.restype = None
    lib.jl_tuning_group_forms_by_count.restype = None
    lib.jl_tuning_group_forms_by_count.argtypes = [C.POINTER(C.c_uint64)]
    orc = oracle_lib.load()
    unfolded = "JL_NO_FOLD_CALL" in os.environ
    for name, n, bound, make in WINDOWS:
        rows, ref, lists = make()
        called = one_window(lib, orc, name, n, bound, rows, ref, lists, unfolded)
        print("%s: %d reads x %d columns, lists %s, %d variants" % (name, n, rows.shape[1], lists, called))
    print("NARROW-OK", "unfolded" if unfolded else "folded")


if __name__ == "__main__":
    main()
