"""GPU parity for what round 2 added to the C ABI: the two-sided Fisher tail, packed per-read ids (4 / 8 / 16 bits),
group runs without phasing and with --drm-only masks per window, overlapping genes that share start columns
(several positions evaluated by the workgroup that counted the codon), and a soak test of the hand-offs between
workgroups (fresh reads in every buffer on every replay)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
from minorseq_amd import capi, msa, synth
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import P_ABS_TOL, assert_phase_equal, assert_variants_equal, oracle_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jl():
    j = capi.Juliet(0)
    yield j
    j.close()


def test_two_sided_tail_on_the_device(jl, oracle):
    """`tail` = 1.  Device numerics (symmetric closed form) against the oracle's brute-force sum
    over all tables, then whole calls: codons observed significantly LESS often than expected are called too."""
    rng = np.random.default_rng(7)
    n = rng.integers(1, 200000, size=4000).astype(np.uint32)
    a = np.minimum(rng.integers(0, 400, size=4000), n).astype(np.uint32)
    c = np.minimum(rng.integers(0, 60, size=4000), n).astype(np.uint32)
    p, lp = jl.fisher_eval(a, c, n, tail=1)
    for i in range(0, 4000, 7):
        op, olp = oracle.fisher(int(a[i]), int(n[i] - a[i]), int(c[i]), int(n[i] - c[i]), tail=1)
        assert abs(p[i] - op) <= P_ABS_TOL
        if np.isfinite(olp) and olp < -1e-9:
            assert abs(lp[i] - olp) <= 1e-8 * max(1.0, abs(olp))
    sp = synth.SynthParams(seed=21, minor_permille=(60, 50, 40, 30), sub_rate=0.004)
    l, nreads = 300, 6000
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, nreads, ref)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    jl.upload_rows(rows)
    for tail in (1, 0):
        prm = capi.default_params(tail=tail, alpha=0.05, n_tests=50)
        out = jl.run(genes, ref, prm, phasing=True)
        ev = oracle.call(rows, genes, refseq=ref, params=oracle_params(prm))
        assert len(ev) > 5
        assert_variants_equal(out["variants"], ev)
        assert_phase_equal(out["phase"], oracle.phase(rows, ev), len(ev))
    # stage API too
    prm = capi.default_params(tail=1, alpha=0.05, n_tests=50)
    jl.pileup_async(genes, ref)
    jl.call_async(prm)
    assert_variants_equal(jl.call_fetch(), oracle.call(rows, genes, refseq=ref, params=oracle_params(prm)))


def many_haplotypes(n_hap, reads_each, rng):
    """A 6-column matrix with n_hap distinct clean patterns of >= 10 reads each (plus damaged and sparse reads)."""
    pats = []
    for c0 in range(64):
        for c1 in range(64):
            pats.append((c0, c1))
    rng.shuffle(pats)
    pats = [(0, 0)] + [p for p in pats if p != (0, 0)][: n_hap - 1]
    rows = []
    for k, (c0, c1) in enumerate(pats):
        cnt = reads_each + (k % 7)
        r = np.zeros((cnt, 6), dtype=np.uint8)
        r[:, 0:3] = [c0 >> 4, (c0 >> 2) & 3, c0 & 3]
        r[:, 3:6] = [c1 >> 4, (c1 >> 2) & 3, c1 & 3]
        rows.append(r)
    extra = np.zeros((50, 6), dtype=np.uint8)
    extra[:20, 1] = msa.SYM_GAP
    extra[20:40, 4] = msa.SYM_MASK
    extra[40:45, :] = [3, 3, 3, 3, 3, 2]     # five reads of a pattern of its own: insufficient coverage
    extra[45:, 0] = msa.SYM_NONE
    m = np.concatenate(rows + [extra])
    return m[rng.permutation(len(m))]


@pytest.mark.parametrize("n_hap,bits", [(5, 4), (14, 4), (15, 8), (200, 8), (254, 8), (255, 16), (400, 16)])
def test_per_read_ids_travel_in_the_narrowest_code(jl, oracle, n_hap, bits):
    """4 bits up to 14 haplotypes, 8 up to 254, 16 beyond: the run view exposes the packed form and its width, every
    fetch gives the oracle's 16-bit ids; single run (ids written by the phasing launch) and group run."""
    rng = np.random.default_rng(n_hap)
    rows = many_haplotypes(n_hap, 12, rng)
    var = np.zeros(2, dtype=capi.VARIANT)
    var["col"] = [0, 3]
    exp = oracle.phase(rows, var.astype(oracle_lib.VARIANT))
    assert exp["summary"]["n_haplotypes"] == n_hap
    genes = np.array([(1, 7)], dtype=capi.GENE)
    # through the whole path: majority mode calls every non-major codon that is frequent enough; compare with the oracle
    jl.upload_rows(rows)
    prm = capi.default_params(alpha=0.5, n_tests=1)
    jl.run_async(genes, None, prm, None, True, 10, True)
    ev = oracle.call(rows, genes, params=oracle_params(prm))
    ep = oracle.phase(rows, ev)
    view = jl.run_view()
    rv = capi.RunView()
    assert jl.lib.jl_run_view_get(jl.h, C.byref(rv)) == 0
    if view is not None:
        H = view["phase"]["summary"]["n_haplotypes"]
        assert rv.read_hap_bits == (4 if H <= 14 else 8 if H <= 254 else 16)
        assert bool(rv.read_hap) == (rv.read_hap_bits == 16) and rv.read_hap_packed
        out = np.zeros(len(rows), dtype=np.uint16)
        assert jl.lib.jl_expand_read_hap(rv.read_hap_packed, rv.read_hap_bits, len(rows), out.ctypes.data_as(C.c_void_p)) == 0
        assert (out == ep["read_hap"]).all() and (np.asarray(view["phase"]["read_hap"]) == ep["read_hap"]).all()
    f = jl.run_fetch(True, True, cap_var=max(64, len(ev)))
    assert_variants_equal(f["variants"], ev)
    assert_phase_equal(f["phase"], ep, len(ev))
    # stage API with a host table: exactly n_hap haplotypes
    jl.phase_async(var, 10)
    got = jl.phase_fetch(cap_var=8)
    got["hit"] = got["hit"][:2]
    assert got["summary"] == exp["summary"] and (got["read_hap"] == exp["read_hap"]).all()
    assert (got["hap_count"] == exp["hap_count"]).all()


def test_group_run_without_phasing_and_with_drm_masks(oracle):
    """jl_group_run_async with phasing off (configs[1] through the group path) and jl_group_run_masked_async with a
    --drm-only mask on some windows only: per window the oracle's table, filtered by that window's mask."""
    l = 240
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ref = synth.reference(77, l)
    ctxs, rows_all = [], []
    for k in range(5):
        n = 4000 + 900 * k
        sp = synth.SynthParams(seed=77 + k, minor_permille=(60, 50, 40, 30), sub_rate=0.003)
        j = capi.Juliet(0)
        j.alloc(n, l)
        j.synth_fill(sp, ref)
        j.sync()
        rows_all.append(msa.unpack_columns(j.download_columns(), n))
        ctxs.append(j)
    grp = capi.Group(ctxs)
    prm = capi.default_params()
    try:
        for rep in range(3):
            grp.run_async(genes, ref, prm, False, 10, False)
            for j, rows in zip(ctxs, rows_all):
                v = j.run_view() or j.run_fetch(False, False)
                assert "phase" not in v
                assert_variants_equal(v["variants"], oracle.call(rows, genes, refseq=ref))
        # masks: window k keeps only codons whose index is divisible by (k + 2); windows 1 and 3 have none
        P = l // 3
        masks = []
        for k in range(5):
            if k in (1, 3):
                masks.append(None)
                continue
            bits = sum(1 << c for c in range(64) if c % (k + 2) == 0)
            masks.append(np.full(P, bits, dtype=np.uint64))
        for phasing in (True, False):
            grp.run_masked_async(genes, ref, prm, masks, phasing, 10, phasing)
            for k, (j, rows) in enumerate(zip(ctxs, rows_all)):
                ev = oracle.call(rows, genes, refseq=ref)
                if masks[k] is not None:
                    ev = ev[ev["codon"] % (k + 2) == 0]
                v = j.run_view() or j.run_fetch(phasing, phasing)
                assert_variants_equal(v["variants"], ev)
                if phasing:
                    assert_phase_equal(v["phase"], oracle.phase(rows, ev), len(ev))
    finally:
        grp.close()
        for j in ctxs:
            j.close()


def test_overlapping_genes_sharing_start_columns(jl, oracle):
    """Genes in ONE frame that overlap (and a duplicate gene): several positions start at the same column and are
    evaluated by the workgroup that counted the codon, rows appear once per (gene, codon); the plan sees each
    column once."""
    n, l = 9000, 360
    sp = synth.SynthParams(seed=33, minor_permille=(60, 50, 40, 30))
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    genes = np.array([(1, 181), (91, 361), (1, 361), (91, 361), (2, 359)], dtype=capi.GENE)
    jl.upload_rows(rows)
    for use_ref in (True, False):
        out = jl.run(genes, ref if use_ref else None, capi.default_params(), phasing=True)
        ev = oracle.call(rows, genes, refseq=ref if use_ref else None)
        assert len(ev) > 8 and len(np.unique(ev["col"])) < len(ev)
        assert_variants_equal(out["variants"], ev)
        assert_phase_equal(out["phase"], oracle.phase(rows, ev), len(ev))


def test_soak_fresh_reads_every_replay(oracle):
    """The hand-offs between workgroups (arrival counters, write-through stores, the completion word) under load: 2000
    replays of a group of six windows and of a single-window graph, NEW reads generated into the buffers before every
    replay (seed = replay number, different per window), every window's result compared with the oracle's — via a
    table of expectations for the 25 seeds the loop cycles through.  A stale header, a stale per-read id or a lost
    table row shows as a mismatch."""
    l, n_seeds, n_win = 90, 25, 6
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ref = synth.reference(3, l)
    shapes = [3000 + 1700 * k for k in range(n_win)]
    ctxs = []
    for n in shapes:
        j = capi.Juliet(0)
        j.alloc(n, l)
        ctxs.append(j)
    single = capi.Juliet(0)
    single.alloc(5000, l)
    prm = capi.default_params()
    expect = {}
    for s in range(n_seeds):
        for k, n in enumerate(shapes + [5000]):
            sp = synth.SynthParams(seed=1000 * k + s, minor_permille=(50 + s, 40, 30 + 2 * s, 25), partial_rate=0.01 * (s % 5))
            rows = synth.rows(sp, l, 0, n, ref)
            ev = oracle.call(rows, genes, refseq=ref)
            ep = oracle.phase(rows, ev)
            expect[(k, s)] = (sp, ev, ep, int(ep["read_hap"].astype(np.uint64).dot(np.arange(1, n + 1, dtype=np.uint64) % 1009)))
    grp = capi.Group(ctxs)
    try:
        for it in range(2000):
            s = (it * 7) % n_seeds
            for k, j in enumerate(ctxs):
                j.synth_fill(expect[(k, (s + k) % n_seeds)][0], ref)
            single.synth_fill(expect[(n_win, s)][0], ref)
            grp.run_async(genes, ref, prm, True, 10, True)
            single.run_async(genes, ref, prm, None, True, 10, True)
            for k, j in enumerate(ctxs + [single]):
                _, ev, ep, chk = expect[(k, (s + k) % n_seeds if k < n_win else s)]
                v = j.run_view()
                assert v is not None, (it, k)
                assert len(v["variants"]) == len(ev) and (v["variants"]["count"] == ev["count"]).all(), (it, k)
                assert v["phase"]["summary"] == ep["summary"], (it, k)
                assert (v["phase"]["hap_count"] == ep["hap_count"]).all(), (it, k)
                ids = np.asarray(v["phase"]["read_hap"])
                got = int(ids.astype(np.uint64).dot(np.arange(1, len(ids) + 1, dtype=np.uint64) % 1009))
                assert got == chk, (it, k)
    finally:
        grp.close()
        single.close()
        for j in ctxs:
            j.close()


def _comm(jl):
    idbuf = np.zeros(128, dtype=np.uint8)
    assert jl.lib.jl_comm_unique_id(idbuf.ctypes.data_as(C.c_void_p)) == 0
    comm = C.c_void_p()
    jl._chk(jl.lib.jl_comm_create(jl.h, idbuf.ctypes.data_as(C.c_void_p), 0, 1, C.byref(comm)))
    return comm


def _gather(c, comm):
    rows = np.zeros(capi.VARIANT_CAP, dtype=capi.VARIANT)
    cnt = np.zeros(1, dtype=np.uint32)
    rc = c.lib.jl_allgather_variants(c.h, comm, rows.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), capi.VARIANT_CAP)
    return rc, rows[: int(cnt[0])].copy()


def test_exchange_of_a_table_larger_than_the_head(oracle):
    """More than 128 called rows: the exchange falls back to the full fixed stride — issued by the communicator's
    worker like every other collective — and, because the full table is not double-buffered, is refused when the
    context has launched another run in between."""
    n, l = 5000, 600
    sp = synth.SynthParams(seed=12, sub_rate=0.02, minor_permille=(70, 60, 50, 40))
    ref = synth.reference(sp.seed, l)
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    prm = capi.default_params(alpha=0.5, n_tests=1)
    j = capi.Juliet(0)
    j.alloc(n, l)
    j.synth_fill(sp, ref)
    comm = _comm(j)
    try:
        j.run_async(genes, ref, prm, None, False, 10, False)
        table = j.run_fetch(False, False)["variants"].copy()
        assert len(table) > 128
        rc, got = _gather(j, comm)
        assert rc == 0 and (got == table).all()
        # requested, then another run before the collect: every rank refuses alike
        j.run_async(genes, ref, prm, None, False, 10, False)
        assert j.lib.jl_allgather_variants_async(j.h, comm) == 0
        j.run_async(genes, ref, prm, None, False, 10, False)
        rc, _ = _gather(j, comm)
        assert rc == -4 and b"not double-buffered" in j.lib.jl_last_error(j.h)
        # stage API: full stride as well
        j.pileup_async(genes, ref)
        j.call_async(prm)
        rc, got = _gather(j, comm)
        assert rc == 0 and (got == table).all()
    finally:
        j.lib.jl_comm_destroy(comm)
        j.close()


def test_batched_exchange_keeps_its_slots_until_all_members_are_collected(oracle):
    """A batch of three exchanges is ONE [rank][window][head] region with one event: collecting the first member must
    not free its slot for a new request whose all-gather would overwrite the heads of the other two."""
    l = 150
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    ref = synth.reference(5, l)
    prm = capi.default_params()
    ctxs, tables = [], []
    for k in range(3):
        j = capi.Juliet(0)
        j.alloc(3000 + 500 * k, l)
        j.synth_fill(synth.SynthParams(seed=50 + k, minor_permille=(60 + 10 * k, 50, 40, 30)), ref)
        ctxs.append(j)
    comm = _comm(ctxs[0])
    try:
        for rnd in range(20):
            for j in ctxs:
                j.run_async(genes, ref, prm, None, True, 10, False)
            tables = [j.run_fetch(True, False)["variants"].copy() for j in ctxs]
            arr = (C.c_void_p * 3)(*[j.h for j in ctxs])
            assert ctxs[0].lib.jl_allgather_variants_async_many(arr, 3, comm) == 0
            rc, got = _gather(ctxs[0], comm)
            assert rc == 0 and (got == tables[0]).all()
            # new work and a new exchange on the context that was just collected, while two members are outstanding
            ctxs[0].synth_fill(synth.SynthParams(seed=900 + rnd, minor_permille=(90, 80, 70, 60)), ref)
            ctxs[0].run_async(genes, ref, prm, None, True, 10, False)
            t0 = ctxs[0].run_fetch(True, False)["variants"].copy()
            assert ctxs[0].lib.jl_allgather_variants_async(ctxs[0].h, comm) == 0
            rc, got = _gather(ctxs[0], comm)
            assert rc == 0 and (got == t0).all()
            for k in (1, 2):
                rc, got = _gather(ctxs[k], comm)
                assert rc == 0 and (got == tables[k]).all(), (rnd, k)
            ctxs[0].synth_fill(synth.SynthParams(seed=50, minor_permille=(60, 50, 40, 30)), ref)
    finally:
        ctxs[0].lib.jl_comm_destroy(comm)
        for j in ctxs:
            j.close()


def test_insertion_counters_match_the_oracle(jl, oracle):
    """insertions per window column, counted on the device from the records (jl_msa_track_insertions),
    against the oracle's loops: lengths 1..30 and longer, inserted bases by offset, windows that cut the reads."""
    from test_gpu_parity import rows_to_records
    rng = np.random.default_rng(8)
    n, l = 3000, 240
    sp = synth.SynthParams(seed=8, partial_rate=0.3)
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    pos, cigar, cig_off, seq4, seq_off, qual, qual_off = rows_to_records(rows, ref, rng)
    # longer insertions than the noise ops have: splice a 33-base and a 9-base insertion into some reads' cigars
    cg, so, s4, co = [], [0], [], [0]
    for r in range(n):
        ops = [int(x) for x in cigar[int(cig_off[r]): int(cig_off[r + 1])]]
        bases = []
        raw = seq4[int(seq_off[r]): int(seq_off[r + 1])]
        for b in raw:
            bases += [b >> 4, b & 15]
        q_total = sum(x >> 4 for x in ops if (x & 15) in (1, 4, 7, 8))
        bases = bases[:q_total]
        if r % 5 == 0 and len(ops) > 3:
            # after the third op: an insertion of 9 (r % 10 == 0) or 33 bases
            k = 9 if r % 10 == 0 else 33
            q_before = sum(x >> 4 for x in ops[:3] if (x & 15) in (1, 4, 7, 8))
            ins = [[1, 2, 4, 8][(r + j) % 4] for j in range(k)]
            bases = bases[:q_before] + ins + bases[q_before:]
            ops = ops[:3] + [(k << 4) | 1] + ops[3:]
        cg += ops
        co.append(len(cg))
        if len(bases) % 2:
            bases.append(0)
        s4 += [(bases[i] << 4) | bases[i + 1] for i in range(0, len(bases), 2)]
        so.append(len(s4))
    cigar, cig_off, seq4, seq_off = (np.array(cg, dtype=np.uint32), np.array(co, dtype=np.uint64), np.array(s4, dtype=np.uint8),
                                     np.array(so, dtype=np.uint64))
    for wb, we in ((0, l), (37, 200)):
        jl.track_insertions(True)
        jl.ingest_records(we - wb, wb, pos, cigar, cig_off, seq4, seq_off)
        lh, bc = jl.insertions_fetch()
        elh, ebc = oracle.insertions(we - wb, wb, pos, cigar, cig_off, seq4, seq_off)
        assert (lh == elh).all() and (bc == ebc).all()
        assert lh[:, 9].sum() > 50 and lh[:, 31].sum() > 50 and lh[:, 1:3].sum() > 100
        # the consensus rule on the DEVICE's counters against the oracle's second formulation, which never sees a counter:
        # explicit insertion records + a sweep over the window's rows (orc_fuse_records)
        genes = np.array([(wb + 1, wb + 1 + 3 * ((we - wb) // 3))], dtype=capi.GENE)
        jl.pileup_async(genes, None)
        col = jl.pileup_fetch()["col_counts"]
        win_rows = msa.unpack_columns(jl.download_columns(), n)
        for frac, dist in ((0.5, 10), (0.05, 1), (0.0, 1), (0.001, 3)):
            assert oracle.fuse(col, lh, bc, frac, dist) == oracle.fuse_records(win_rows, wb, pos, cigar, cig_off, seq4, seq_off, frac, dist)
        assert len(oracle.fuse(col, lh, bc, 0.0, 1)) > len(oracle.fuse(col, None, None)) + 30    # insertions did enter
    jl.track_insertions(False)
    jl.ingest_records(l, 0, pos, cigar, cig_off, seq4, seq_off)
    with pytest.raises(capi.JulietError):
        jl.insertions_fetch()


def test_result_block_holds_a_sixteen_position_window(oracle):
    """More than ten variant positions (multi-word keys) with ~100 haplotypes: 49 variants x 125 haplotypes of `hit` used to
    overflow the pinned result block (4 KB), so every run fell back to the copying fetch.  The zero-copy view must now
    carry it, bit-exact, on the first run (single-word launch flags, fetch re-runs) and on the following ones."""
    n, l = 100_000, 900
    sp = synth.SynthParams(seed=23)
    ref = synth.reference(sp.seed, l)
    rows = synth.rows(sp, l, 0, n, ref)
    rng = np.random.default_rng(3)
    for k in range(12):
        who = rng.choice(n, n // 30, replace=False)
        c0 = 3 * (20 + 22 * k)
        rows[who, c0:c0 + 3] = (rows[who, c0:c0 + 3] + 1 + k % 3) % 4
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    exp_v = oracle.call(rows, genes, refseq=ref)
    exp = oracle.phase(rows, exp_v)
    assert exp["summary"]["n_positions"] > 10 and len(exp_v) * exp["summary"]["n_haplotypes"] > 4096
    assert len(exp_v) <= 128 and exp["summary"]["n_haplotypes"] <= 128       # the block's row limits
    c = capi.Juliet(0)
    c.upload_columns(msa.pack_columns(rows), n)
    prm = capi.default_params()
    for rep in range(3):
        c.run_async(genes, ref, prm, None, True, 10, True)
        v = c.run_view()
        if rep == 0 and v is None:      # the flagged first run may need the copying fetch (it re-runs the pipeline)
            v = c.run_fetch(True, True, cap_var=128)
        assert v is not None, "the result block must hold this window"
        ph = v["phase"]
        h = exp["summary"]["n_haplotypes"]
        assert ph["summary"] == exp["summary"]
        assert (np.asarray(ph["hap_count"])[:h] == exp["hap_count"]).all()
        assert (np.asarray(ph["hap_pattern"])[:h, :exp["summary"]["n_positions"]] == exp["hap_pattern"]).all()
        assert (np.asarray(ph["hit"])[:len(exp_v), :h] == exp["hit"]).all()
        assert (np.asarray(ph["read_hap"]) == exp["read_hap"]).all()
    c.close()


def test_fold_timeout_is_rerun_unfolded(tmp_path):
    """A phase launch with inline ids (it writes the per-read ids itself) whose waiting workgroups give up (they were not
    resident together) marks the run failed on the device; the host then runs the phasing stage again with a separate ids
    launch — transparently: the caller gets the right answer, the context keeps the separate ids launch from then on.  A
    group's later runs must then launch it too: the second group run below, on other reads, would keep the first run's
    ids otherwise.  The time-out is forced in a -DJL_TUNING build (tools_tuning/build_tuning_lib.sh;
    JL_FORCE_IDS_WAIT_TIMEOUT), in a child process (the test process holds the shipped library)."""
    import subprocess
    import sys
    lib = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")
    if not os.path.exists(lib):
        pytest.skip("no tuning build of the library (tools_tuning/build_tuning_lib.sh)")
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["JL_ROOT"]); sys.path.insert(0, os.path.join(os.environ["JL_ROOT"], "tests"))
import oracle_lib
from minorseq_amd import capi, msa, synth
capi.load_library(os.environ["JL_LIB"])
n, l = 5000, 300
sp = synth.SynthParams(seed=31, minor_permille=(70, 60, 50, 40), partial_rate=0.1)
ref = synth.reference(sp.seed, l)
rows = synth.rows(sp, l, 0, n, ref)
genes = np.array([(1, l + 1)], dtype=capi.GENE)
orc = oracle_lib.load()
ev = orc.call(rows, genes, refseq=ref)
ep = orc.phase(rows, ev)
jl = capi.Juliet(0)
jl.upload_rows(rows)
for rep in range(3):      # the first run times out and is run again; the next ones have a separate ids launch from the start
    out = jl.run(genes, ref)
    assert (out["variants"]["count"] == ev["count"]).all()
    assert out["phase"]["summary"] == ep["summary"] and (out["phase"]["read_hap"] == ep["read_hap"]).all(), rep
# a group of two windows: both time out, both are run again on the group's stream
a, b = capi.Juliet(0), capi.Juliet(0)
a.upload_rows(rows); b.upload_rows(rows[::-1].copy())
g = capi.Group([a, b])
g.run_async(genes, ref, capi.default_params(), True, 10, True)
va = a.run_view(); vb = b.run_view()
assert (va["phase"]["read_hap"] == ep["read_hap"]).all() and (vb["phase"]["read_hap"] == ep["read_hap"][::-1]).all()
# the group again with the windows' reads swapped: each window's ids are those of the reads it holds NOW (after a time-out
# both contexts take a separate ids launch, which the group has to make)
a.upload_rows(rows[::-1].copy()); b.upload_rows(rows)
g.run_async(genes, ref, capi.default_params(), True, 10, True)
va = a.run_view(); vb = b.run_view()
assert (va["phase"]["read_hap"] == ep["read_hap"][::-1]).all(), "window a: ids of the reads it holds now"
assert (vb["phase"]["read_hap"] == ep["read_hap"]).all(), "window b: ids of the reads it holds now"
# the stage API
c = capi.Juliet(0)
c.upload_rows(rows)
c.pileup_async(genes, ref); c.call_async(); c.phase_async()
ph = c.phase_fetch()
assert ph["summary"] == ep["summary"] and (ph["read_hap"] == ep["read_hap"]).all()
print("RERUN-OK")
'''
    env = dict(os.environ, JL_LIB=lib, JL_ROOT=ROOT, JL_FORCE_IDS_WAIT_TIMEOUT="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RERUN-OK" in out.stdout, out.stdout + out.stderr
    # ... and without the forced time-out the same build writes the ids inline and needs no second run
    env.pop("JL_FORCE_IDS_WAIT_TIMEOUT")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RERUN-OK" in out.stdout, out.stdout + out.stderr
