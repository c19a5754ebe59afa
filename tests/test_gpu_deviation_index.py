"""The deviation index (DESIGN.md "The deviation index"): a window that is run again counts from per-codon lists of the reads that
deviate from the column majority instead of from the planes, and nothing downstream may tell.  Every comparison is EXACT equality —
column counts, codon histograms, the variant table (its p-values bit for bit), the phasing result — between run 1 (planes), a run
>= 3 that jl_msa_index_info reports as index-form, and the oracle.  Runs only on a real MI355X: `pytest -m gpu`.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
from minorseq_amd import capi, msa, synth

pytestmark = pytest.mark.gpu

INT_FIELDS = ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")


@pytest.fixture(scope="module")
def orc():
    return oracle_lib.load()


def make_rows(n, l, seed, n_rate=0.01, minor=0.04, sub=0.004, ref_seed=None):
    """n reads x l columns: a reference, a minor haplotype that edits the first four codons' middle bases in `minor` of the reads, scattered
    N, deletions and substitutions: about 9 % of the reads deviate per codon, under the density bound of 14 % at every n used.  Returns (rows, ref)."""
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


def snapshot(jl, genes, ref, prm=None):
    out = jl.run(genes, ref, prm or capi.default_params(), phasing=True)
    pile = jl.pileup_fetch()
    return out, pile


def assert_same(a, b, where):
    (oa, pa), (ob, pb) = a, b
    assert (pa["col_counts"] == pb["col_counts"]).all(), where
    assert (pa["hist"] == pb["hist"]).all(), where
    assert oa["variants"].tobytes() == ob["variants"].tobytes(), where
    assert oa["phase"]["summary"] == ob["phase"]["summary"], where
    assert (oa["phase"]["hap_count"] == ob["phase"]["hap_count"]).all(), where
    assert (oa["phase"]["read_hap"] == ob["phase"]["read_hap"]).all(), where


def assert_oracle(orc, rows, genes, ref, snap, where):
    out, pile = snap
    assert (pile["col_counts"] == orc.pileup(rows)).all(), where
    hist, cov = orc.codon_hist(rows, pile["pos_col"])
    assert (pile["hist"] == hist).all() and (pile["coverage"] == cov).all(), where
    exp_v = orc.call(rows, genes, refseq=ref)
    assert len(out["variants"]) == len(exp_v), where
    for k in INT_FIELDS:
        assert (out["variants"][k] == exp_v[k]).all(), (where, k)
    exp_p = orc.phase(rows, exp_v)
    assert out["phase"]["summary"] == exp_p["summary"], where
    assert (out["phase"]["hap_count"] == exp_p["hap_count"]).all(), where
    assert (out["phase"]["read_hap"] == exp_p["read_hap"]).all(), where


def three_runs(jl, genes, ref, expect_state=capi.INDEX_BUILT):
    """run 1 (planes), run 2 (planes, build behind it), the build waited for, run 3: returns (snap1, snap3, info after run 3)."""
    builds = jl.index_info()["builds"]   # (counted over the context's life)
    s1 = snapshot(jl, genes, ref)
    i1 = jl.index_info()
    assert i1["runs"] == 1 and i1["state"] == capi.INDEX_NONE and i1["last_form"] == 0 and i1["builds"] == builds
    snapshot(jl, genes, ref)
    i2 = jl.index_info(wait=True)
    assert i2["runs"] == 2 and i2["last_form"] == 0 and i2["state"] == expect_state, i2
    s3 = snapshot(jl, genes, ref)
    i3 = jl.index_info()
    assert i3["runs"] == 3 and i3["last_form"] == (1 if expect_state == capi.INDEX_BUILT else 0), i3
    return s1, s3, i3


ONE_FRAME = lambda l: np.array([(1, l + 1)], dtype=capi.GENE)


@pytest.mark.parametrize("l", [3, 6, 7, 9, 33])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 1023, 1025, 4097])
def test_shapes_one_frame(orc, n, l):
    """7 columns: a short last chunk that stays on the planes in a run that also has indexed chunks (a second launch)."""
    rows, ref = make_rows(n, l, seed=1000 * n + l)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        for refseq in (ref, None):   # reference and majority-codon mode: the index seed must not care
            genes = ONE_FRAME(l)
            if refseq is None:
                jl.upload_rows(rows)   # a new generation: the counter restarts
            s1, s3, info = three_runs(jl, genes, refseq)
            assert info["plain_chunks"] == l // 3 and info["indexed_chunks"] == l // 3
            assert_same(s1, s3, (n, l, refseq is None))
            if refseq is not None:
                assert_oracle(orc, rows, genes, ref, s3, (n, l))
    finally:
        jl.close()


@pytest.mark.parametrize("n", [65, 1025])
def test_two_frames_halo_and_fillers(orc, n):
    """Two genes in different frames that overlap at one codon: a halo chunk and filler chunks beside the plain ones — counted
    correctly from both launches."""
    l = 33
    rows, ref = make_rows(n, l, seed=n)
    genes = np.array([(1, 16), (14, 32)], dtype=capi.GENE)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3, info = three_runs(jl, genes, ref)
        flags = jl.index_info(chunk_flags=True)["chunk_flags"]
        assert 0 < info["indexed_chunks"] == int((flags == 1).sum()) and (flags[:12] == 0).any()
        assert_same(s1, s3, n)
        assert_oracle(orc, rows, genes, ref, s3, n)
    finally:
        jl.close()


def test_dense_frames_stay_on_the_planes(orc):
    """Two frames over the whole window: the uniform six-column grid, which has no plain chunk — never indexed."""
    n, l = 257, 33
    rows, ref = make_rows(n, l, seed=5)
    genes = np.array([(1, 31), (2, 32)], dtype=capi.GENE)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3, info = three_runs(jl, genes, ref, expect_state=capi.INDEX_NONE)
        assert info["builds"] == 0
        assert_same(s1, s3, "w6")
        assert_oracle(orc, rows, genes, ref, s3, "w6")
    finally:
        jl.close()


def test_dense_chunk_stays_on_the_planes(orc):
    """Every read carries an N in codon 1: 1023 entries against the chunk's bound of 144 (9 x 128 / 8): that chunk has no list,
    its neighbours have."""
    n, l = 1023, 9
    rows, ref = make_rows(n, l, seed=11)
    rows[:, 4] = 5
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3, info = three_runs(jl, ONE_FRAME(l), ref)
        flags = jl.index_info(chunk_flags=True)["chunk_flags"]
        assert list(flags[:3]) == [1, 2, 1] and info["indexed_chunks"] == 2 and info["plain_chunks"] == 3
        assert_same(s1, s3, "dense")
        assert_oracle(orc, rows, ONE_FRAME(l), ref, s3, "dense")
    finally:
        jl.close()


def test_partial_reads_straddle_the_density_bound(orc):
    """partial_rate 0.9: runs of uncovered cells in most reads — chunks on both sides of the density bound in one window."""
    n, l = 4097, 33
    sp = synth.SynthParams(seed=3, partial_rate=0.9)
    ref = synth.reference(sp.seed, l)
    jl = capi.Juliet(0)
    try:
        jl.alloc(n, l)
        jl.synth_fill(sp, ref)
        s1, s3, info = three_runs(jl, ONE_FRAME(l), ref)
        flags = jl.index_info(chunk_flags=True)["chunk_flags"][:11]
        assert (flags == 2).any() and (flags == 1).any() and info["indexed_chunks"] == int((flags == 1).sum())
        assert_same(s1, s3, "partial")
        rows = msa.unpack_columns(jl.download_columns(), n)
        assert_oracle(orc, rows, ONE_FRAME(l), ref, s3, "partial")
    finally:
        jl.close()


def test_matrix_without_a_chunk_under_the_bound_is_refused(orc):
    """Every read carries an N in every codon: no chunk is under its bound (1023 entries against 144), the lists could only be
    longer than the planes: the index is refused and every later run takes the planes with identical results.  (A chunk over its
    bound never enters the total, so the total bound cannot be passed any other way.)"""
    n, l = 1023, 9
    rows, ref = make_rows(n, l, seed=13)
    rows[:, 1::3] = 5
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3, info = three_runs(jl, ONE_FRAME(l), ref, expect_state=capi.INDEX_REFUSED)
        assert info["builds"] == 1 and info["indexed_chunks"] == 0
        s4 = snapshot(jl, ONE_FRAME(l), ref)
        assert jl.index_info()["last_form"] == 0 and jl.index_info()["builds"] == 1
        assert_same(s1, s3, "refused")
        assert_same(s1, s4, "refused, run 4")
        assert_oracle(orc, rows, ONE_FRAME(l), ref, s4, "refused")
    finally:
        jl.close()


def test_accumulator_flush_edge(orc):
    """The counting kernel's fields are 9 bits; a lane takes 4 entries a round and flushes every 127 rounds (508 <= 511), i.e.
    a workgroup flushes after 127 x 4 x 256 = 130048 entries of a chunk.  A chunk stays indexed up to 9 plane_stride / 8 entries:
    924 673 reads are the fewest whose bound (plane_stride 115 712: 130 176) lies above the edge (tests/cpp/
    deviation_index_check.cpp).  All 130 176 entries carry the SAME non-seed code in column 0, so one field of every lane takes
    all four of a round's entries: 508 at the flush, 512 — an overflow into the next field, a wrong count of T and of G — with an
    interval one round longer; the other two columns put the same load on the seed's own fields."""
    n, l = 924673, 3
    stride = (n + 1023) // 1024 * 128
    e = 9 * stride // 8
    assert (n - 1 + 1023) // 1024 * 128 * 9 // 8 <= 127 * 4 * 256 < e == 130176
    rng = np.random.default_rng(17)
    ref = np.array([0, 1, 2], dtype=np.uint8)
    rows = np.tile(ref, (n, 1))
    who = rng.choice(n, e, replace=False)
    rows[who, 0] = 3                                       # T in column 0 of every listed read
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        s1, s3, info = three_runs(jl, ONE_FRAME(l), ref)
        assert info["entries"] == e and info["indexed_chunks"] == 1
        assert_same(s1, s3, "flush edge")
        assert (s3[1]["col_counts"] == orc.pileup(rows)).all()
        hist, cov = orc.codon_hist(rows, s3[1]["pos_col"])
        assert (s3[1]["hist"] == hist).all()
    finally:
        jl.close()


def test_staleness_every_producer_starts_a_new_generation(orc):
    """Build an index, rewrite the matrix through each producer in turn with different reads: the next run is run 1 of a new
    generation, plane form, and its results are those of the new reads (the image the producer left, which test_gpu_planes.py
    pins byte for byte per producer).  Then the new generation gets an index of its own (or is refused one: the record reads'
    uncovered ends put most chunks over the density bound), and the run after it still gives the same results."""
    from test_gpu_planes import records
    from test_gpu_qmask import MIN_QV, five, np_mask
    n, l = 1025, 36
    genes = ONE_FRAME(l)
    rec = records(n)
    jl, src = capi.Juliet(0), capi.Juliet(0)
    try:
        rows, ref = make_rows(n, l, seed=21)
        other = make_rows(n, l, seed=27, ref_seed=21)[0]
        src.upload_rows(other)
        src.sync()
        idx = np.random.default_rng(5).permutation(n).astype(np.uint32)

        def records_window(min_qv, wait):
            src.records_upload(*five(rec), qual=rec["qual"], qual_off=rec["qual_off"])
            try:
                jl.records_window(src, l, 0, min_qv, wait=wait)
                jl.sync()
            finally:
                src.records_drop()

        producers = [
            ("pack_rows", lambda: jl.upload_rows(make_rows(n, l, seed=22, ref_seed=21)[0])),
            ("upload", lambda: jl.upload_columns(msa.pack_columns(make_rows(n, l, seed=23, ref_seed=21)[0]), n)),
            ("synth_fill", lambda: jl.synth_fill(synth.SynthParams(seed=24), ref)),
            ("ingest_records", lambda: jl.ingest_records(l, 0, *five(rec))),
            ("ingest_records_masked", lambda: jl.ingest_records(l, 0, *five(rec), min_qv=MIN_QV, qmask=np_mask(rec, MIN_QV))),
            ("records_finish", lambda: jl.ingest_records_chunked(l, 0, *five(rec), rec["qual"], rec["qual_off"], min_qv=MIN_QV, chunk_reads=257)),
            ("records_window", lambda: records_window(0, True)),
            ("records_window_async", lambda: records_window(MIN_QV, False)),
            ("take", lambda: jl.take([(src, idx)])),
            ("take_async", lambda: jl.take([(src, idx[::-1].copy())], wait=False)),
        ]
        # (the record paths leave one of two images, with and without the QV filter: other producers in between, so that every
        # step rewrites the matrix with different reads)
        order = ["pack_rows", "ingest_records", "upload", "ingest_records_masked", "synth_fill", "records_finish", "take",
                 "records_window", "take_async", "records_window_async"]
        producers = sorted(producers, key=lambda p: order.index(p[0]))
        jl.upload_rows(rows)
        three_runs(jl, genes, ref)
        prev = rows
        for how, produce in producers:
            before = jl.index_info()
            assert before["runs"] >= 3 and before["state"] in (capi.INDEX_BUILT, capi.INDEX_REFUSED), (how, before)
            produce()
            s = snapshot(jl, genes, ref)
            info = jl.index_info()
            assert info["generation"] > before["generation"] and info["runs"] == 1 and info["last_form"] == 0, (how, info)
            assert info["state"] == capi.INDEX_NONE, (how, info)
            now = msa.unpack_columns(jl.download_columns(), n)
            assert now.shape == prev.shape and (now != prev).any(), how
            assert_oracle(orc, now, genes, ref, s, how)
            snapshot(jl, genes, ref)                       # ... and the new generation gets its own index, or is refused one
            state = jl.index_info(wait=True)["state"]
            assert state in (capi.INDEX_BUILT, capi.INDEX_REFUSED), how
            s3 = snapshot(jl, genes, ref)
            assert jl.index_info()["last_form"] == (1 if state == capi.INDEX_BUILT else 0), how
            assert_same(s, s3, how)
            prev = now
    finally:
        jl.close()
        src.close()


def test_adopted_matrix_is_never_indexed(orc):
    import torch
    n, l = 1025, 9
    rows, ref = make_rows(n, l, seed=31)
    planes = msa.pack_planes(rows)
    t = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    jl = capi.Juliet(0)
    try:
        jl.adopt(t.data_ptr(), n, l, planes.shape[2], keep_alive=t)
        snaps = [snapshot(jl, ONE_FRAME(l), ref) for _ in range(4)]
        info = jl.index_info(wait=True)
        assert info["runs"] == 4 and info["builds"] == 0 and info["state"] == capi.INDEX_NONE and info["last_form"] == 0
        for s in snaps[1:]:
            assert_same(snaps[0], s, "adopted")
        assert_oracle(orc, rows, ONE_FRAME(l), ref, snaps[-1], "adopted")
    finally:
        jl.close()


def test_changed_genes_restart_the_counter(orc):
    n, l = 1025, 33
    rows, ref = make_rows(n, l, seed=41)
    jl = capi.Juliet(0)
    try:
        jl.upload_rows(rows)
        three_runs(jl, ONE_FRAME(l), ref)
        genes2 = np.array([(4, 31)], dtype=capi.GENE)      # another chunk table
        s = snapshot(jl, genes2, ref)
        info = jl.index_info()
        assert info["runs"] == 1 and info["state"] == capi.INDEX_NONE and info["last_form"] == 0
        assert_oracle(orc, rows, genes2, ref, s, "genes2")
        snapshot(jl, genes2, ref)
        jl.index_info(wait=True)
        s3 = snapshot(jl, genes2, ref)
        assert jl.index_info()["last_form"] == 1
        assert_same(s, s3, "genes2 run 3")
    finally:
        jl.close()


GROUP_L = 34    # eleven plain chunks and a filler column: a rest table, so an index-form launch is two launches


def group_windows(n=1025, l=GROUP_L, k=3):
    ref = make_rows(n, l, seed=50)[1]
    ctxs, rows_of = [], []
    for i in range(k):
        rows = make_rows(n, l, seed=50 + i, ref_seed=50)[0]   # (different reads of one reference)
        jl = capi.Juliet(0)
        jl.upload_rows(rows)
        jl.sync()
        ctxs.append(jl)
        rows_of.append(rows)
    return ctxs, rows_of, ref


@pytest.mark.parametrize("case", ["plain-folded", "masked-folded", "plain-unfolded", "masked-unfolded"])
def test_group_takes_the_index_only_when_every_window_has_one(orc, case):
    """Three windows, one of them a run behind: the group counts from the planes for all until all three are built.  Both forms
    of a group run: a group without neighbours takes the folded form; JL_NO_FOLD_CALL (read once per process: a child process,
    as tests/test_gpu_call_edges.py does) forces the unfolded one — pileup_index_group_kernel and the plain plane kernel over the
    rest tables."""
    masked, unfolded = case.startswith("masked"), case.endswith("unfolded")
    if unfolded and "JL_NO_FOLD_CALL" not in os.environ:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", __file__, "-k",
                            "test_group_takes_the_index_only_when_every_window_has_one and " + case],
                           env=dict(os.environ, JL_NO_FOLD_CALL="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return
    n, l = 1025, GROUP_L
    genes = ONE_FRAME(l)
    prm = capi.default_params()
    ctxs, rows_of, ref = group_windows()
    try:
        for jl in ctxs[:2]:                                # windows 0 and 1: run 1 alone
            snapshot(jl, genes, ref)
        grp = capi.Group(ctxs)
        masks = [None, None, None]

        def launch():
            if masked:
                grp.run_masked_async(genes, ref, prm, masks, True, 10, True)
            else:
                grp.run_async(genes, ref, prm, True, 10, True)
            views = []
            for c in ctxs:
                c.run_wait()
                v = c.run_fetch(True, True, cap_var=64)
                views.append((v["variants"].copy(), dict(v["phase"]["summary"]), v["phase"]["read_hap"].copy(), c.pileup_fetch()))
            return views

        first = launch()                                   # run 2, 2, 1: planes; builds of windows 0 and 1 behind it
        assert [c.index_info(wait=True)["state"] for c in ctxs] == [capi.INDEX_BUILT, capi.INDEX_BUILT, capi.INDEX_NONE]
        assert [c.index_info()["last_form"] for c in ctxs] == [0, 0, 0]
        second = launch()                                  # run 3, 3, 2: window 2 has none yet -> planes for all; its build
        assert [c.index_info()["last_form"] for c in ctxs] == [0, 0, 0]
        assert all(c.index_info(wait=True)["state"] == capi.INDEX_BUILT for c in ctxs)
        third = launch()                                   # all built: the index form
        assert [c.index_info()["last_form"] for c in ctxs] == [1, 1, 1]
        for k in range(3):
            for other in (second, third):
                assert first[k][0].tobytes() == other[k][0].tobytes() and first[k][1] == other[k][1]
                assert (first[k][2] == other[k][2]).all()
                assert (first[k][3]["col_counts"] == other[k][3]["col_counts"]).all() and (first[k][3]["hist"] == other[k][3]["hist"]).all()
            assert (third[k][3]["col_counts"] == orc.pileup(rows_of[k])).all()
            exp_v = orc.call(rows_of[k], genes, refseq=ref)
            for f in INT_FIELDS:
                assert (third[k][0][f] == exp_v[f]).all(), (k, f)
            assert (third[k][2] == orc.phase(rows_of[k], exp_v)["read_hap"]).all()
        grp.close()
    finally:
        for c in ctxs:
            c.close()


def test_bound_exchange_in_index_form(orc):
    """A group with a bound exchange (the one-rank communicator): every run carries the all-gather of its windows' table heads,
    one graph per parity of the exchange.  Five runs, each collected: runs 1 and 2 from the planes, runs 3 to 5 — both parities —
    from the index; the gathered rows are the oracle's every time."""
    n, l = 1025, GROUP_L
    genes = ONE_FRAME(l)
    prm = capi.default_params()
    ctxs, rows_of, ref = group_windows(k=2)
    exp = [orc.call(r, genes, refseq=ref) for r in rows_of]
    grp = capi.Group(ctxs)
    idbuf = np.zeros(128, dtype=np.uint8)
    lib = ctxs[0].lib
    assert lib.jl_comm_unique_id(idbuf.ctypes.data_as(C.c_void_p)) == 0
    comm = C.c_void_p()
    ctxs[0]._chk(lib.jl_comm_create(ctxs[0].h, idbuf.ctypes.data_as(C.c_void_p), 0, 1, C.byref(comm)))
    try:
        grp.bind_exchange(comm)
        forms = []
        for run in range(1, 6):
            grp.run_async(genes, ref, prm, True, 10, True)
            rows_, counts = grp.exchange_collect(1)
            forms.append([c.index_info(wait=True)["last_form"] for c in ctxs])
            for k, e in enumerate(exp):
                assert counts[k, 0] == len(e), (run, k)
                got = rows_[k, 0, : counts[k, 0]]
                for f in INT_FIELDS:
                    assert (got[f] == e[f]).all(), (run, k, f)
                v = ctxs[k].run_fetch(True, True, cap_var=64)
                assert (v["phase"]["read_hap"] == orc.phase(rows_of[k], e)["read_hap"]).all(), (run, k)
                assert (ctxs[k].pileup_fetch()["col_counts"] == orc.pileup(rows_of[k])).all(), (run, k)
        assert forms == [[0, 0], [0, 0], [1, 1], [1, 1], [1, 1]]
        grp.bind_exchange(None)
    finally:
        grp.close()
        lib.jl_comm_destroy(comm)
        for c in ctxs:
            c.close()
