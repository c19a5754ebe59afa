"""Every reader of the resident matrix with its plane rows on both sides of 4 GiB (tests/high_rows.py): one adopted torch tensor
of 2049 reads x 1150 columns at a plane stride of 1 250 048 bytes — 3450 plane rows, 4.31 GB — that every test of this module
shares.  A plane row lies at base + (3 c + k) * plane_stride; from row 3436 on that offset needs more than 32 bits, and an offset
formed in 32 bits aliases a low row of the same allocation: wrong counts, no fault.  Every column holds its own seeded content, so
a wrapped offset changes the answer.

Every expectation is the stage's own mirror (tests/*_mirror.py) or the oracle over the by-row matrix, compared as the stage's own
test compares it (equality for every integer, that test's tolerance for p-values); never another device result.  Every stage is
asked about positions in three bands — columns 0 .. 20, the codons that hold column 1145 (plane 0 below the line, planes 1 and 2
above) and the codons above it, the last at n_cols - 3 — and once about the upper bands alone, and the mirror's answer is asserted
to hold what the stage distinguishes there before the device is looked at.

Padding.  The stages that bound their walk by n_reads (everything from the class pileup on) see seeded random bytes in bytes
257 .. 271 of every plane row, as the adopted-stride tests of their own files have it.  The pileup and the phasing kernels walk the
whole plane stride and rely on the contract of jl_msa_adopt (padding reads = code 6), so bytes 272 .. plane_stride - 1 of every
row hold code 6 once and for all, and the tests of those stages put code 6 into bytes 257 .. 271 too while they run (the caller
may rewrite an adopted matrix between runs).

Left out: the deviation index — an adopted matrix is never indexed (test_gpu_deviation_index.test_adopted_matrix_is_never_indexed),
so neither its build nor an index-form count can read this tensor; jl_group_run_async and the timing entry points run the kernels
of jl_run_async; the RCCL assemblies run the pack kernel of the local ones; jl_sites_assemble_alleles needs a record build as its
source.  tests/test_capi_exports.py holds the classification of every exported function.  Runs only on a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import class_codons_mirror
import control_mirror as cm
import deletion_alleles_mirror as am
import deletion_mirror as dm
import high_rows as hr
import hypermut_mirror as hm
import linkage_mirror
import nearest_mirror
import orf_mirror as om
import readstats_mirror as rm
import recombinant_mirror
import rescue_mirror
import sites_mirror as sm
import xwin_edges as xe
from minorseq_amd import capi, msa, sharding
from test_gpu_parity import assert_phase_equal, assert_variants_equal, oracle_params

pytestmark = pytest.mark.gpu

N, L, STRIDE = hr.N, hr.L, hr.STRIDE
U, NONE, AMB, WHOLE = capi.RESCUE_UNINFORMATIVE, capi.RESCUE_NONE, capi.RESCUE_AMBIGUOUS, capi.RECOMB_WHOLE
GENES = np.array(hr.GENES, dtype=capi.GENE)


class High:
    """The tensor, the rows it holds, and contexts that adopt it."""

    def __init__(self):
        import torch
        self.torch = torch
        self.rows, self.ref, self.haps = hr.build()
        garbage, clean = hr.pack_prefix(self.rows)
        self.t = torch.empty(3 * L * STRIDE, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0 and self.t.numel() > hr.LINE
        view = self.t.view(3 * L, STRIDE)
        planes = self.t.view(L, 3, STRIDE)
        planes[:, 0, hr.PREFIX:] = 0                     # code 6 behind the prefix: plane 0 clear, planes 1 and 2 set
        planes[:, 1:, hr.PREFIX:] = 0xFF
        self.prefix = view[:, :hr.PREFIX]
        self.d_garbage, self.d_clean = torch.from_numpy(garbage).cuda(), torch.from_numpy(clean).cuda()
        self.prefix.copy_(self.d_garbage)                # one strided copy of the packed planes
        torch.cuda.synchronize()
        self.open = []

    def padding(self, clean):
        self.prefix.copy_(self.d_clean if clean else self.d_garbage)
        self.torch.cuda.synchronize()

    def ctx(self):
        j = capi.Juliet(0)
        j.adopt(self.t.data_ptr(), N, L, STRIDE, keep_alive=self.t)
        self.open.append(j)
        return j

    def close(self):
        for j in self.open:
            j.close()
        self.open = []


@pytest.fixture(scope="module")
def high():
    h = High()
    yield h
    h.close()
    del h.t


@pytest.fixture
def jh(high):
    """A context on the tensor, random bytes behind the reads."""
    j = high.ctx()
    yield j
    j.sync()
    j.close()


@pytest.fixture
def jp(high):
    """A context on the tensor for the stages that walk the whole plane stride: code 6 behind the reads while the test runs."""
    high.padding(True)
    j = high.ctx()
    yield j
    j.sync()
    j.close()
    high.padding(False)


def test_the_matrix_is_the_edge_it_claims_to_be(high):
    """The numbers of tests/high_rows.py hold for the tensor as it lies in memory, and what a download shows is the rows."""
    assert high.t.numel() == 3 * L * STRIDE == 4_312_665_600
    row = lambda c, k: (3 * c + k) * STRIDE               # noqa: E731
    assert row(1145, 0) < hr.LINE <= row(1145, 1) and row(1144, 2) < hr.LINE and row(1149, 2) + STRIDE == high.t.numel()
    assert sum(1 for r in range(3 * L) if r * STRIDE >= hr.LINE) == 14
    # independent content on both sides of the line: no plane row above it equals the row a 32-bit offset would reach
    first = high.prefix[:, :hr.NB].cpu().numpy()
    for r in range(hr.FIRST_HIGH_ROW, 3 * L):
        wrapped = (r * STRIDE) % hr.LINE
        alias, off = divmod(wrapped, STRIDE)
        assert off + hr.NB <= STRIDE and alias < hr.FIRST_HIGH_ROW
        if off < hr.NB:
            assert not (first[r, :hr.NB - off] == first[alias, off:]).all()


# ------------------------------------------------------------------------------------------------ pileup, call, phase
def expected_run(oracle, rows, ref):
    prm = capi.default_params(n_tests=sharding.default_n_tests(GENES))
    exp_v = oracle.call(rows, GENES, refseq=ref, params=oracle_params(prm))
    cols = exp_v["col"].astype(np.int64)
    assert (cols <= 18).sum() >= 3 and np.isin(cols, hr.MID_STARTS).sum() >= 3 and np.isin(cols, hr.HIGH_STARTS).sum() >= 2
    assert {0, 1, 2} <= set(exp_v["gene"].tolist())                      # all three frames call
    exp_p = oracle.phase(rows, exp_v)
    s = exp_p["summary"]
    assert s["n_haplotypes"] >= 4 and s["damaged_reads"] >= 50 and s["insufficient_reads"] >= 1 and hr.in_high(exp_p["pos_cols"]).sum() >= 3
    return prm, exp_v, exp_p


def test_run_with_phasing(high, jp, oracle):
    prm, exp_v, exp_p = expected_run(oracle, high.rows, high.ref)
    out = jp.run(GENES, high.ref, prm, phasing=True)
    assert_variants_equal(out["variants"], exp_v)
    assert_phase_equal(out["phase"], exp_p, len(exp_v))
    print("pileup kernel:", jp.lib.jl_pileup_kernel_name(jp.h))
    pf = jp.pileup_fetch()
    assert (pf["col_counts"] == oracle.pileup(high.rows)).all()


def test_run_without_phasing(high, jp, oracle):
    prm, exp_v, _ = expected_run(oracle, high.rows, high.ref)
    jp.run_async(GENES, high.ref, prm, None, False, 10, False)
    assert_variants_equal(jp.run_fetch(False, False)["variants"].copy(), exp_v)
    pf = jp.pileup_fetch()
    hist, cov = oracle.codon_hist(high.rows, pf["pos_col"])
    assert (pf["hist"] == hist).all() and (pf["coverage"] == cov).all()


def test_stage_api_pileup_call_phase(high, jp, oracle):
    prm, exp_v, exp_p = expected_run(oracle, high.rows, high.ref)
    rows = high.rows
    jp.pileup_async(GENES, high.ref)
    got = jp.pileup_fetch()
    assert len(got["pos_col"]) == 383 + 383 + 382 and {1143, 1144, 1145, 1146, 1147} <= set(got["pos_col"].tolist())
    assert (got["col_counts"] == oracle.pileup(rows)).all()
    assert (got["col_counts"].sum(axis=1) == (rows != msa.SYM_NONE).sum(axis=0)).all()
    hist, cov = oracle.codon_hist(rows, got["pos_col"])
    assert (got["hist"] == hist).all() and (got["coverage"] == cov).all()
    col = oracle.pileup(rows)[:, :5]
    assert (jp.consensus() == np.where(col.max(axis=1) == 0, 5, col.argmax(axis=1)).astype(np.uint8)).all()
    jp.call_async(prm)
    table = jp.call_fetch()
    assert_variants_equal(table, exp_v)
    jp.phase_async(None)
    assert_phase_equal(jp.phase_fetch(cap_var=len(exp_v)), exp_p, len(exp_v))
    high_only = exp_v[hr.in_high(exp_v["col"])]
    assert len(high_only) >= 5
    jp.phase_async(high_only)
    exp_high = oracle.phase(rows, high_only)
    assert exp_high["summary"]["n_haplotypes"] >= 2 and exp_high["summary"]["damaged_reads"] >= 20
    assert_phase_equal(jp.phase_fetch(cap_var=len(high_only)), exp_high, len(high_only))


def test_control_call(high, jp):
    """Sample and control adopt the same tensor: nothing is called; then a context of its own holds the rows with a few columns
    perturbed, as the control of the tensor and as the sample against it."""
    rows = high.rows
    rng = np.random.default_rng(12)
    other = rows.copy()
    for c in (2, 1144, 1149):                                             # codons the tensor lacks
        who = rng.permutation(N)[:180]
        other[who, c] = (other[who, c] + 1 + rng.integers(0, 3, size=len(who))) % 7 % 4
    for c in (5, 1145, 1148):                                             # ... and the tensor's minor codons taken out
        base = other[:, c] < 4
        other[base, c] = high.ref[c]
    genes = np.array(hr.CONTROL_GENES, dtype=capi.GENE)
    pg, pk, pc, rc, n_tests = cm.positions(hr.CONTROL_GENES, L, high.ref)
    hs, ho = cm.hists(rows, pc), cm.hists(other, pc)
    twin, small = high.ctx(), capi.Juliet(0)
    try:
        small.upload_rows(other)
        for c in (jp, twin, small):
            c.pileup_async(genes, high.ref)
        prm = capi.default_params(alpha=0.01)
        jp.control_call_async(twin, prm)
        got, cov = jp.control_call_fetch()
        assert len(got) == 0 and len(cov) == 0                            # (c * cov_s > a * cov_c never holds: SPEC §21)
        from test_gpu_control import assert_table
        for s, c, h_s, h_c, where in ((jp, small, hs, ho, "tensor as sample"), (small, jp, ho, hs, "tensor as control")):
            want, want_cov = cm.call_rows(h_s, h_c, pg, pk, pc, rc, 0.01, n_tests)
            cols = np.array([w[2] for w in want])
            assert (cols <= 18).any() and np.isin(cols, hr.MID_STARTS).any() and np.isin(cols, hr.HIGH_STARTS).any(), where
            s.control_call_async(c, prm)
            got, cov = s.control_call_fetch()
            assert_table(got, cov, want, want_cov, where)
    finally:
        small.close()


# ------------------------------------------------------------------------------------------------ the hap walk
def pattern_of(high, pos_cols):
    return hr.codons_at(high.haps, pos_cols)


def test_rescue(high, jh):
    rows = high.rows
    for pos in (hr.POS_COLS, hr.HIGH_POS):
        pat = pattern_of(high, pos)
        exp = rescue_mirror.rescue(rows, pos, pat, 1)
        assert (exp[2] > 0).all(), exp[2]                                 # assigned, ambiguous, none, uninformative: all occur
        out = jh.phase_rescue(pos, pat, 1)
        assert (out["rescue"] == exp[0]).all() and (out["hap_reads"] == exp[1]).all() and (out["tally"] == exp[2]).all()
        assert int(out["tally"].sum()) == N


def test_nearest(high, jh):
    rows = high.rows
    for pos, d in ((hr.POS_COLS, 3), (hr.HIGH_POS, 2)):
        pat = pattern_of(high, pos)
        exp = nearest_mirror.nearest(rows, pos, pat, 1, d)
        assert (exp[3] > 0).all() and (exp[2].sum(axis=0) > 0).all(), (exp[3], exp[2].sum(axis=0))   # four categories, every distance
        out = jh.phase_nearest(pos, pat, 1, d)
        assert (out["nearest"] == exp[0]).all() and (out["dist"] == exp[1]).all()
        assert (out["hap_reads"] == exp[2]).all() and (out["tally"] == exp[3]).all()


def test_recombinant(high, jh):
    rows = high.rows
    for pos in (hr.POS_COLS, hr.HIGH_POS):
        pat = pattern_of(high, pos)
        exp = recombinant_mirror.recombinants(rows, pos, pat, 1)
        left, right = exp["left"], exp["right"]
        got = {"B": ((left < hr.N_HAP) & (right < hr.N_HAP)).any(), "W": (left == WHOLE).any(), "N": (left == NONE).any(), "U": (left == U).any()}
        assert all(got.values()), got                                     # both parents unique, whole, none, uninformative
        out = jh.phase_recombinants(pos, pat, 1)
        for key in ("left", "right", "prefix", "suffix", "parent_reads", "tally"):
            assert (out[key] == exp[key]).all(), key


# ------------------------------------------------------------------------------------------------ the tile walk and its kin
def class_labels():
    rng = np.random.default_rng(33)
    pool = np.array(list(range(17)) + [0xFFFE, 0xFFFF, 17], dtype=np.uint16)
    return pool[rng.integers(0, len(pool), size=N)], 17


def test_class_pileup_and_consensus(high, jh):
    from test_gpu_class import expected
    rows = high.rows
    lab, k = class_labels()
    exp_counts, exp_reads = expected(rows, lab, k)
    assert (exp_counts[:, 1143:, :5].sum(axis=(1, 2)) > 0).all() and exp_counts[:, 1145:, 4].sum() > 0 and exp_counts[:, 1145:, 5].sum() > 0
    counts, reads = jh.class_pileup(lab, k)
    assert (reads == exp_reads).all() and (counts == exp_counts).all(), np.argwhere(counts != exp_counts)[:8]
    assert (counts.sum(axis=(0, 2)) == (rows[lab < k] != 6).sum(axis=0)).all()
    cons = capi.consensus_of_counts(counts.reshape(k * L, 6)).reshape(k, L)
    c5 = exp_counts[:, :, :5]
    assert (cons == np.where(c5.max(axis=2) == 0, 5, c5.argmax(axis=2))).all()


def test_class_codons(high, jh):
    rows = high.rows
    lab, k = class_labels()
    cols = np.array(sorted(set(range(0, 19)) | set(range(1140, 1148))), dtype=np.uint32)
    exp_hist, exp_reads = class_codons_mirror.class_codons(rows, lab, k, cols)
    assert (exp_hist[:, hr.in_high(cols)].sum(axis=(1, 2)) > 0).all() and (exp_hist[:, -1].sum(axis=1) > 0).all()
    hist, reads = jh.class_codons(lab, k, cols)
    assert (reads == exp_reads).all() and (hist == exp_hist).all(), np.argwhere(hist != exp_hist)[:8]


def test_codon_deletions(high, jh):
    exp = dm.counts(high.rows)
    for band in (slice(0, 19), slice(1143, 1148)):
        assert exp[band, dm.CODON].all() and exp[band, dm.DEL3].any() and exp[band, dm.PARTIAL].any()
    assert exp[1147, dm.DEL3] > 0 and exp[1145, dm.DEL3] > 0
    got = jh.codon_deletions()
    assert got.shape == (L - 2, 4) and (got == exp).all(), np.argwhere(got != exp)[:8]


def test_deletion_alleles(high, jh):
    from test_gpu_deletion_alleles import assert_equal
    exp = am.alleles(high.rows)
    al = exp["alleles"]
    end = al["col"].astype(np.int64) + al["len"]
    assert exp["runs"][0] >= 100 and exp["runs"][1] >= 1 and exp["open"][1145:].any() and exp["open"][:3].any()
    assert ((al["col"] < 1145) & (end > 1145)).any() and (al["col"] >= 1146).any() and (al["col"] <= 18).any()     # across, above, below
    assert_equal(jh.deletion_alleles(), exp)


def test_variant_linkage(high, jh):
    from test_gpu_linkage import some_pair_has_all_four
    rows = high.rows
    for pos in (hr.POS_COLS, hr.HIGH_POS):
        codons = pattern_of(high, pos)
        var_pos, var_codon = [], []
        for p in range(len(pos)):
            present = list(dict.fromkeys(codons[:, p].tolist()))
            absent = [x for x in range(64) if x not in present]
            for cd in (present + absent)[:3]:
                var_pos.append(p), var_codon.append(cd)
        var_pos, var_codon = np.array(var_pos, dtype=np.uint32), np.array(var_codon, dtype=np.uint8)
        exp = linkage_mirror.linkage(rows, pos, var_pos, var_codon)
        assert some_pair_has_all_four(exp, var_pos)
        out = jh.variant_linkage(pos, var_pos, var_codon)
        for key in ("both", "carry", "joint"):
            assert (out[key] == exp[key]).all(), key


def test_read_stats(high, jh):
    rows = high.rows
    compare = rm.consensus(rows)
    compare[[5, 600, 1144, 1149]] = 0xFF
    exp = rm.stats(rows, compare)
    only_high = rm.stats(rows[:, 1145:], compare[1145:])
    assert only_high[4].any() and only_high[1].any() and only_high[2].any()          # mismatches, gaps and N above the line
    got = jh.read_stats(compare)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]


def test_read_hypermut(high, jh):
    from hypermut_tables import assert_p_close
    rows, ref = high.rows, high.ref
    exp = hm.counts(rows, ref)
    above = hm.counts(rows[:, 1143:], ref[1143:])
    assert above[hm.TARGET_MUT].any() and above[hm.CONTROL_SITES].any() and (exp[hm.TARGET_MUT] >= 5).any()
    got, p, lp = jh.read_hypermut(ref)
    assert (got == exp).all(), np.argwhere(got != exp)[:8]
    some = np.concatenate([np.flatnonzero(exp[hm.TARGET_MUT] >= 5)[:20], np.arange(0, N, 97)])
    assert_p_close(p[some], lp[some], exp[:, some])


def test_read_orf(high, jh):
    rows, ref = high.rows, high.ref
    spans = [(0, 7), (1, 6), (2, 5), (600, 100), (1131, 5), (1137, 4), (1140, 3), (1141, 3), (1142, 2), (1146, 1), (1147, 1)]
    assert spans[-1][0] + 3 == L and spans[4][0] + 15 <= 1146 and spans[5][0] < 1145 < spans[5][0] + 12      # below, across
    exp_c, exp_f = om.counters(rows, spans, ref)
    for s in (0, 5, 6, 7, 9, 10):
        assert exp_c[om.STOPS, s].any() and exp_c[om.GAP_CELLS, s].any() and (exp_f[s] != om.NO_STOP).any(), s
    got_c, got_f = jh.read_orf(spans, ref)
    assert (got_c == exp_c).all(), np.argwhere(got_c != exp_c)[:8]
    assert (got_f == exp_f).all(), np.argwhere(got_f != exp_f)[:8]


# ------------------------------------------------------------------------------------------------ the matrix as a source
def test_sites_assemble(high, jh, oracle):
    from test_gpu_sites import check
    NF = sm.NO_FILL
    sites = [(0, sm.CODON, NF), (3, sm.CODON, 27), (3, sm.DELETION, NF), (18, sm.DELETION, NF), (1143, sm.CODON, NF), (1144, sm.DELETION, NF),
             (1145, sm.CODON, 9), (1145, sm.DELETION, NF), (1146, sm.CODON, NF), (1147, sm.CODON, NF), (1147, sm.DELETION, NF)]
    for col, kind, _ in sites[4:]:
        codon, del3 = sm.classes(high.rows, col)
        assert codon.any() and del3.any() and (~(codon | del3)).any(), col
    pc = capi.Juliet(0)
    try:
        pc.sites_assemble(jh, sites)
        check(pc, jh, high.rows, sites, oracle)
    finally:
        pc.close()


def test_take(high, jh):
    from test_gpu_take import assert_is_selection
    rng = np.random.default_rng(5)
    dst = capi.Juliet(0)
    try:
        for idx in (rng.integers(0, N, size=1500).astype(np.uint32), np.arange(N, dtype=np.uint32)[::-1].copy()):
            dst.take([(jh, idx)])
            assert_is_selection(dst, high.rows[idx])
    finally:
        dst.close()


def test_download(high, jh):
    """jl_msa_download (planes_to_nibbles) over all 1150 columns: every cell of every read."""
    got = msa.unpack_columns(jh.download_columns(), N)
    assert (got == high.rows).all(), np.argwhere(got != high.rows)[:8]


def test_cross_window_pack_and_session(high, jp, oracle):
    """The pack launch cell by cell (both assemblies) over positions of all bands, and the smallest session — one window, one rank —
    that owns positions above the line, against the oracle's phasing of the same reads."""
    rows = high.rows
    table = np.zeros(len(hr.POS_COLS), dtype=capi.VARIANT)
    table["col"], table["codon"] = hr.POS_COLS, pattern_of(high, hr.POS_COLS)[4]
    for b, k in ((0, N), (256, N - 256)):
        pc = capi.Juliet(0)
        remapped, pos = pc.xwin_assemble_slice_local([jp], table, b, k)
        assert pos.tolist() == hr.POS_COLS.tolist()
        plane_reads = xe.stride_reads(k)
        shown = 2 * pc.col_stride
        got = msa.unpack_columns(pc.download_columns(), shown)
        exp = np.full((shown, 3 * len(pos)), 6, np.uint8)
        m = min(shown, plane_reads)
        exp[:m] = xe.pack_expected(rows, pos, b, k, plane_reads)[:m]
        assert (got == exp).all(), np.argwhere(got != exp)[:8]
        pc.close()
    prm, exp_v, exp_p = expected_run(oracle, rows, high.ref)
    ph, pos_global = capi.phase_across_windows([jp], exp_v)
    assert (pos_global == exp_p["pos_cols"]).all() and hr.in_high(pos_global).sum() >= 3
    assert_phase_equal(dict(ph, pos_cols=pos_global), exp_p, len(exp_v))


# ------------------------------------------------------------------------------------------------ strides of 4 GiB and more
def test_a_plane_stride_of_4_gib_is_refused(high):
    """Several launchers carry the stride, or a quotient of it, in 32 bits (kernels_phase.hip: col_stride / 4 dwords).  Nothing
    is launched: the shape is refused where it is set, and the context keeps no matrix."""
    j = capi.Juliet(0)
    lib = j.lib
    for stride in (1 << 32, (1 << 32) + 272, 1 << 36):
        rc = lib.jl_msa_adopt(j.h, C.c_void_p(high.t.data_ptr()), N, 1, stride, 0)
        assert rc == -1 and "4 GiB" in lib.jl_last_error(j.h).decode(), (stride, lib.jl_last_error(j.h))
    assert lib.jl_codon_deletions_async(j.h) == -4                        # no resident matrix
    rc = lib.jl_msa_adopt(j.h, C.c_void_p(high.t.data_ptr()), N, 1, (1 << 32) - 16, 0)      # the largest stride below: accepted
    assert rc == 0
    j.close()
