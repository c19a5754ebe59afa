"""Child process of tests/test_gpu_index_forms.py (not a test module: the form of a launch depends on the process's environment
and on the library build, and a process loads one library).

    python index_forms_child.py SCENARIO       SCENARIO: edges | forms
    JL_LIB: the library to load (the -DJL_TUNING build: jl_tuning_group_forms_by_count)
    JL_NO_FOLD_CALL=1 (edges): the unfolded kernels, whose list walk holds one round in registers

Prints EDGES-OK / FORMS-OK as its last line.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib  # noqa: E402
from minorseq_amd import capi  # noqa: E402

INT_FIELDS = ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")
FOLDED_PLANES, UNFOLDED_PLANES, FOLDED_INDEX, UNFOLDED_INDEX = range(4)


def by_count(lib):
    """Group launches of this process by (form, counting form): folded/planes, unfolded/planes, folded/index, unfolded/index."""
    out = (C.c_uint64 * 4)()
    lib.jl_tuning_group_forms_by_count(out)
    f, u = C.c_uint64(), C.c_uint64()
    lib.jl_tuning_group_forms(C.byref(f), C.byref(u))
    got = [int(x) for x in out]
    assert (got[0] + got[2], got[1] + got[3]) == (int(f.value), int(u.value)), (got, f.value, u.value)   # the two hooks agree
    return got


def one_frame(l):
    return np.array([(1, l + 1)], dtype=capi.GENE)


def snapshot(jl):
    """Column counts, histograms and variant table of the context's last run, as copies."""
    jl.run_wait()
    v = jl.run_fetch(False, False, cap_var=64)
    p = jl.pileup_fetch()
    return v["variants"].copy(), p


def assert_same(a, b, where):
    assert (a[1]["col_counts"] == b[1]["col_counts"]).all(), where
    assert (a[1]["hist"] == b[1]["hist"]).all() and (a[1]["coverage"] == b[1]["coverage"]).all(), where
    assert a[0].tobytes() == b[0].tobytes(), where


def assert_oracle(exp, snap, where):
    exp_cols, exp_hist, exp_cov, exp_v = exp
    got_v, pile = snap
    assert (pile["col_counts"] == exp_cols).all(), where
    assert (pile["hist"] == exp_hist).all() and (pile["coverage"] == exp_cov).all(), where
    assert len(got_v) == len(exp_v), where
    for k in INT_FIELDS:
        assert (got_v[k] == exp_v[k]).all(), (where, k)


# ---------------------------------------------------------------------------------------------------------------- edges
# The folded kernels' list walk holds DEPTH = 8 rounds of 256 lanes x 4 entries in registers: a round is 1024 entries, a batch 8192.
# Lists on both sides of a round, of one batch and of two batches, the empty list and a single entry; 16 385 is under the density
# bound of 9 x plane_stride / 8 = 16 416 entries at 116 000 reads (plane_stride 14 592).
EDGE_ENTRIES = (0, 1, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 16383, 16384, 16385)
EDGE_READS, EDGE_COLS = 116_000, 36


def edge_rows():
    """All reads equal the reference; chunk k has exactly EDGE_ENTRIES[k] reads with one substitution in one of its columns:
    three in four of them the same one (a codon frequent enough to be called in the long lists), the others any."""
    rng = np.random.default_rng(4242)
    ref = rng.integers(0, 4, EDGE_COLS).astype(np.uint8)
    rows = np.tile(ref, (EDGE_READS, 1))
    for k, e in enumerate(EDGE_ENTRIES):
        who = rng.choice(EDGE_READS, e, replace=False)
        same = rng.random(e) < 0.75
        col = np.where(same, 3 * k + 1, 3 * k + rng.integers(0, 3, e))
        rows[who, col] = (ref[col] + np.where(same, 1, 1 + rng.integers(0, 3, e))) % 4
    return rows.astype(np.uint8), ref


def scenario_edges(lib, orc):
    unfolded = "JL_NO_FOLD_CALL" in os.environ
    n, l = EDGE_READS, EDGE_COLS
    assert capi.load_library().jl_plane_stride(n) == 14592 and max(EDGE_ENTRIES) <= 9 * 14592 // 8
    rows, ref = edge_rows()
    genes = one_frame(l)
    prm = capi.default_params()
    a, b = capi.Juliet(0), capi.Juliet(0)
    try:
        a.upload_rows(rows)
        a.sync()
        # ---- alone: run 1 from the planes, run 2 with the build behind it, run 3 from the lists (the single kernel)
        a.run_async(genes, ref, prm, None, False, 10, False)
        planes = snapshot(a)
        assert a.index_info()["last_form"] == 0
        exp_hist, exp_cov = orc.codon_hist(rows, planes[1]["pos_col"])
        exp = (orc.pileup(rows), exp_hist, exp_cov, orc.call(rows, genes, refseq=ref))
        assert_oracle(exp, planes, "planes")
        assert len(exp[3]) >= 1     # (the long lists' common codon is called: the table is not empty)
        a.run_async(genes, ref, prm, None, False, 10, False)
        a.run_wait()
        info = a.index_info(wait=True, chunk_flags=True)
        assert info["state"] == capi.INDEX_BUILT and info["plain_chunks"] == 12 and info["indexed_chunks"] == 12, info
        assert list(info["chunk_flags"][:12]) == [1] * 12 and info["entries"] == sum(EDGE_ENTRIES), info
        a.run_async(genes, ref, prm, None, False, 10, False)
        single = snapshot(a)
        assert a.index_info()["last_form"] == 1
        assert_same(planes, single, "single run from the index")
        assert_oracle(exp, single, "single run from the index")
        # ---- the same rows in a group of two windows: launch 1 and 2 from the planes (window b is a run behind), launch 3 from the lists
        b.upload_rows(rows)
        b.sync()
        grp = capi.Group([a, b])
        before = by_count(lib)
        for launch in range(3):
            grp.run_async(genes, ref, prm, False, 10, False)
            snaps = [snapshot(c) for c in (a, b)]
            forms = [c.index_info(wait=True)["last_form"] for c in (a, b)]
            assert forms == ([1, 1] if launch == 2 else [0, 0]), (launch, forms)
            for k, s in enumerate(snaps):
                assert_same(planes, s, ("group launch", launch, k))
                assert_oracle(exp, s, ("group launch", launch, k))
        took = [x - y for x, y in zip(by_count(lib), before)]
        assert took == ([0, 2, 0, 1] if unfolded else [2, 0, 1, 0]), took     # every launch was alone
        grp.close()
    finally:
        a.close()
        b.close()
    print("EDGES-OK", "unfolded" if unfolded else "folded")


# ---------------------------------------------------------------------------------------------------------------- forms
GROUP_L = 34    # eleven plain chunks and a filler column: a rest table, so an index-form launch is two counting launches


def make_rows(n, l, seed, n_rate=0.01, minor=0.04, sub=0.004, ref_seed=None):
    """n reads x l columns: a reference, a minor haplotype that edits the first four codons' middle bases in `minor` of the reads,
    scattered N, deletions and substitutions: about 9 % of the reads deviate per codon, under the density bound of 14 %."""
    rng = np.random.default_rng(seed)
    ref = np.random.default_rng(seed if ref_seed is None else ref_seed).integers(0, 4, l).astype(np.uint8)
    rows = np.tile(ref, (n, 1))
    who = rng.random(n) < minor
    for c in range(1, min(l, 12), 3):   # (at most four variant positions: a group run phases with one key word)
        rows[who, c] = (ref[c] + 1) % 4
    r = rng.random((n, l))
    rows[r < n_rate] = 5
    rows[(r >= n_rate) & (r < n_rate + 0.003)] = 4
    sub = (r >= n_rate + 0.003) & (r < n_rate + 0.003 + sub)
    rows[sub] = (rows[sub] + 1 + rng.integers(0, 3, int(sub.sum()))) % 4
    return rows.astype(np.uint8), ref


def group_windows(seed0, n=1025, l=GROUP_L, k=3):
    ref = make_rows(n, l, seed=50)[1]
    ctxs, rows_of = [], []
    for i in range(k):
        rows = make_rows(n, l, seed=seed0 + i, ref_seed=50)[0]   # (different reads of one reference)
        jl = capi.Juliet(0)
        jl.upload_rows(rows)
        jl.sync()
        ctxs.append(jl)
        rows_of.append(rows)
    return ctxs, rows_of, ref


def scenario_forms(lib, orc):
    genes = one_frame(GROUP_L)
    prm = capi.default_params()
    sets = []
    for seed0 in (50, 60):
        ctxs, rows_of, ref = group_windows(seed0)
        exp, single = [], []
        for jl, rows in zip(ctxs, rows_of):
            ev = orc.call(rows, genes, refseq=ref)
            exp.append((ev, orc.phase(rows, ev), orc.pileup(rows)))
            single.append(jl.run(genes, ref, prm, None, True))     # run 1 of every window, alone
        sets.append((ctxs, ref, exp, single))
    groups = [capi.Group(s[0]) for s in sets]     # both live before the first launch: each has one neighbour on the device

    def collect(k, where, index_form=True):
        ctxs, ref, exp, single = sets[k]
        for jl, (ev, ep, cols), s in zip(ctxs, exp, single):
            jl.run_wait()
            v = jl.run_fetch(True, True, cap_var=64)
            assert v["variants"].tobytes() == s["variants"].tobytes(), where      # the single run's bits
            for f in INT_FIELDS:
                assert (v["variants"][f] == ev[f]).all(), (where, f)
            assert v["phase"]["summary"] == ep["summary"] == s["phase"]["summary"], where
            assert (v["phase"]["hap_count"] == ep["hap_count"]).all(), where
            assert (v["phase"]["read_hap"] == ep["read_hap"]).all() and (v["phase"]["read_hap"] == s["phase"]["read_hap"]).all(), where
            assert (jl.pileup_fetch()["col_counts"] == cols).all(), where
            assert jl.index_info()["last_form"] == (1 if index_form else 0), where

    def launch(k):
        groups[k].run_async(genes, sets[k][1], prm, True, 10, True)

    assert by_count(lib) == [0, 0, 0, 0]
    # ---- run 2 of every window: from the planes, alone (folded), the builds behind it
    for k in range(2):
        launch(k)
        collect(k, ("build launch", k), index_form=False)
        assert all(c.index_info(wait=True)["state"] == capi.INDEX_BUILT for c in sets[k][0])
    assert by_count(lib) == [2, 0, 0, 0]
    # ---- lone launches from the index: each collected before the next, so every one is folded
    made = 2
    for rep in range(3):
        for k in range(2):
            before = by_count(lib)
            launch(k)
            collect(k, ("lone", rep, k))
            made += 1
            after = by_count(lib)
            assert [x - y for x, y in zip(after, before)] == [0, 0, 1, 0], (rep, k, before, after)
    # ---- back to back: B is enqueued microseconds behind A, whose form it is free to find complete or not — every result is
    # checked whatever was taken, and launch by launch the four counts add up to the launches made
    start = by_count(lib)
    for rnd in range(10):
        launch(0)
        launch(1)
        made += 2
        now = by_count(lib)
        assert sum(now) == made and now[FOLDED_PLANES] == 2 and now[UNFOLDED_PLANES] == 0, (rnd, now)
        collect(0, ("back to back", rnd, 0))
        collect(1, ("back to back", rnd, 1))
    took = [x - y for x, y in zip(by_count(lib), start)]
    print("back to back, ten rounds: folded/planes %d, unfolded/planes %d, folded/index %d, unfolded/index %d" % tuple(took))
    assert sum(took) == 20 and took[FOLDED_PLANES] == took[UNFOLDED_PLANES] == 0     # (no form of such a launch is asserted)
    # The one thing here that leans on the device: B's enqueue finds A — a chain of counting, phasing and completion kernels behind
    # a graph launch made microseconds before — incomplete at least once in ten rounds, and so counts from the index UNFOLDED.
    assert took[UNFOLDED_INDEX] >= 1, took
    for g in groups:
        g.close()
    for ctxs, _, _, _ in sets:
        for c in ctxs:
            c.close()
    print("FORMS-OK", took[FOLDED_INDEX], took[UNFOLDED_INDEX])


def main():
    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_group_forms.restype = None
    lib.jl_tuning_group_forms_by_count.restype = None
    lib.jl_tuning_group_forms_by_count.argtypes = [C.POINTER(C.c_uint64)]
    orc = oracle_lib.load()
    {"edges": scenario_edges, "forms": scenario_forms}[sys.argv[1]](lib, orc)


if __name__ == "__main__":
    main()
