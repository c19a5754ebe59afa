"""jl_control_call_async / _fetch on the device against the exact mirror (control_mirror.py; docs/SPEC.md §21): a sample and a
control of different depth over windows of 9, 66 and 258 columns with 1, 4, 5, 43 and 67 positions (full and partial workgroups
of the four-positions-a-block launch), two overlapping genes in different frames, in majority mode and with a config sequence.
Positions are designed so that the control has no coverage, lacks the codon, carries more of it than the sample, the sample's
majority is tied, the config codon holds an N, and --min-perc removes a called codon; then sample == control, the decision edges
of the mirror, a table beyond `cap`, and every refusal.  Rows and control coverages must be equal, p and ln p within the bounds
of test_fisher_host.py.  Runs only on a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import control_mirror as cm
from minorseq_amd import capi

pytestmark = pytest.mark.gpu

P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12

# (columns, genes, sample reads, control reads, config sequence?)
CASES = {
    "P1": (9, [(4, 7)], 96, 33, False),
    "P4": (9, [(1, 10), (2, 5)], 1000, 2049, True),
    "P5": (66, [(1, 10), (3, 9)], 1025, 1024, False),
    "P43": (66, [(1, 67), (2, 65)], 96, 33, True),
    "P67": (258, [(1, 121), (2, 83)], 1000, 2049, False),
    "P67cfg": (258, [(1, 121), (2, 83)], 1025, 1024, True),
}
N_POS = {"P1": 1, "P4": 4, "P5": 5, "P43": 43, "P67": 67, "P67cfg": 67}


def make_pair(n_cols, n_s, n_c, seed):
    """(sample rows, control rows, base sequence): both follow one random sequence with a little substitution noise, and the
    codons of frame 0 take turns in six designs (see the module text)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, n_cols).astype(np.uint8)
    out = []
    for n in (n_s, n_c):
        m = np.tile(base, (n, 1))
        hit = rng.random(m.shape) < 0.002
        m[hit] = (m[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        out.append(m.astype(np.uint8))
    S, Ct = out
    S[: max(1, n_s // 20), : n_cols // 3] = 6            # reads that begin late
    for k in range(n_cols // 3):
        c0 = 3 * k
        alt = base[c0:c0 + 3].copy()
        alt[0] = (alt[0] + 1) % 4
        kind = k % 6
        if kind == 0:      # a minor codon of the sample that the control lacks
            S[rng.permutation(n_s)[: max(2, n_s * 6 // 100)], c0:c0 + 3] = alt
        elif kind == 1:    # no control coverage
            Ct[:, c0 + 1] = 6
        elif kind == 2:    # the control carries more of the codon than the sample
            S[rng.permutation(n_s)[: max(1, n_s * 2 // 100)], c0:c0 + 3] = alt
            Ct[rng.permutation(n_c)[: max(2, n_c * 10 // 100)], c0:c0 + 3] = alt
        elif kind == 3:    # the sample's majority is tied (an odd read out is masked)
            S[:, c0:c0 + 3] = base[c0:c0 + 3]
            S[: n_s // 2, c0:c0 + 3] = alt
            if n_s % 2:
                S[n_s - 1, c0 + 2] = 5
        elif kind == 4:    # a rare codon the control lacks: called, and below --min-perc 3
            alt2 = base[c0:c0 + 3].copy()
            alt2[2] = (alt2[2] + 2) % 4
            S[rng.permutation(n_s)[: max(1, n_s * 15 // 1000)], c0:c0 + 3] = alt2
        else:              # deletions and masked bases
            S[rng.permutation(n_s)[: n_s // 10], c0 + 1] = 4
            Ct[rng.permutation(n_c)[: n_c // 10], c0] = 5
    return S, Ct, base


@pytest.fixture(scope="module")
def ctxs():
    s, c = capi.Juliet(0), capi.Juliet(0)
    yield s, c
    s.close()
    c.close()


@pytest.fixture(scope="module")
def data():
    """Matrices, plans and histograms of every case, made once."""
    out = {}
    for name, (n_cols, genes, n_s, n_c, cfg) in CASES.items():
        S, Ct, base = make_pair(n_cols, n_s, n_c, seed=len(out) + 1)
        refseq = None
        if cfg:
            refseq = base.copy()
            refseq[9 if n_cols > 9 else 7] = 5     # a config codon with an N
        pg, pk, pc, rc, n_tests = cm.positions(genes, n_cols, refseq)
        assert len(pc) == N_POS[name]
        out[name] = dict(S=S, C=Ct, refseq=refseq, genes=np.array(genes, dtype=capi.GENE), pos=(pg, pk, pc, rc), n_tests=n_tests,
                         hs=cm.hists(S, pc), hc=cm.hists(Ct, pc))
    return out


def load(ctxs, d):
    s, c = ctxs
    s.upload_rows(d["S"])
    c.upload_rows(d["C"])
    s.pileup_async(d["genes"], d["refseq"])
    c.pileup_async(d["genes"], d["refseq"])


def assert_table(got, cov, want, want_cov, where):
    ints = [tuple(int(r[k]) for k in ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")) for r in got]
    assert ints == [w[:8] for w in want], where
    assert cov.tolist() == want_cov, where
    assert (got["flags"] == 0).all() and (got["pad_"] == 0).all(), where
    if not want:
        return
    gp = np.array([w[8] for w in want])
    glp = np.array([w[9] for w in want])
    assert np.abs(got["p_value"] - gp).max() <= P_ABS_TOL, where
    big = gp > 1e-300
    assert (np.abs(got["p_value"][big] - gp[big]) <= P_REL_TOL * gp[big]).all(), where
    assert (np.abs(got["log_p"] - glp) <= 1e-12 * np.maximum(1.0, np.abs(glp)) + 1e-13).all(), where


@pytest.mark.parametrize("name", list(CASES))
def test_device_against_the_mirror(ctxs, data, name):
    d = data[name]
    load(ctxs, d)
    s, c = ctxs
    assert s.lib.jl_n_positions(s.h) == N_POS[name]
    seen = {}
    for min_perc in (-1.0, 3.0):
        prm = capi.default_params(alpha=0.01, min_perc=min_perc)
        st = {}
        want, want_cov = cm.call_rows(d["hs"], d["hc"], *d["pos"], 0.01, d["n_tests"], min_perc=min_perc, stats=st)
        s.control_call_async(c, prm)
        got, cov = s.control_call_fetch()
        assert_table(got, cov, want, want_cov, (name, min_perc))
        seen[min_perc] = (st, len(want))
    st, n_rows = seen[-1.0]
    print(name, "rows", n_rows, "with --min-perc 3:", seen[3.0][1], st)
    if name.startswith("P67"):   # the deep windows meet every design
        assert n_rows >= 10 and st["control_lacks_codon"] > 20 and st["control_carries_more"] >= 5 and st["no_control_coverage"] >= 5
        assert seen[3.0][0].get("removed_by_perc", 0) >= 5 and seen[3.0][1] < n_rows
        assert (st.get("majority_tied", 0) >= 5) if d["refseq"] is None else (st["config_codon_not_acgt"] >= 1)


def test_drm_masks_keep_only_their_codons(ctxs, data):
    d = data["P67"]
    load(ctxs, d)
    s, c = ctxs
    drm = np.array([0xAAAAAAAAAAAAAAAA if p % 2 else 2 ** 64 - 1 for p in range(67)], dtype=np.uint64)
    st = {}
    want, want_cov = cm.call_rows(d["hs"], d["hc"], *d["pos"], 0.01, d["n_tests"], drm=drm, stats=st)
    s.control_call_async(c, capi.default_params(alpha=0.01), drm)
    got, cov = s.control_call_fetch()
    assert_table(got, cov, want, want_cov, "drm")
    assert st.get("removed_by_drm", 0) >= 1 and len(want) >= 5


def test_sample_as_its_own_control_calls_nothing(ctxs, data):
    d = data["P67"]
    load(ctxs, d)
    s, _ = ctxs
    s.control_call_async(s, capi.default_params(alpha=0.01, n_tests=1.0))
    got, cov = s.control_call_fetch()
    assert len(got) == 0 and len(cov) == 0


@pytest.mark.parametrize("alpha,n_tests", [(0.01, 1.0), (0.01, 99.0), (0.05, 3000.0), (1e-6, 1.0)])
def test_decision_edges_on_the_device(ctxs, alpha, n_tests):
    """a* - 1 and a* of every edge table as two codons of one position: exactly the a* codons are called."""
    tabs = cm.edge_tables(alpha, n_tests)
    assert len(tabs) >= 8
    hs, hc = cm.edge_window(tabs)
    P = len(tabs)
    genes = np.array([(1, 3 * P + 1)], dtype=capi.GENE)
    refseq = np.zeros(3 * P, dtype=np.uint8)       # config codon AAA = 0
    s, c = ctxs
    s.upload_rows(cm.rows_of_hists(hs, seed=1))
    c.upload_rows(cm.rows_of_hists(hc, seed=2))
    s.pileup_async(genes, refseq)
    c.pileup_async(genes, refseq)
    pg, pk, pc, rc, _ = cm.positions([(1, 3 * P + 1)], 3 * P, refseq)
    want, want_cov = cm.call_rows(hs, hc, pg, pk, pc, rc, alpha, n_tests)
    assert [w[4] for w in want] == [42] * P and [w[5] for w in want] == [t[3] for t in tabs]
    s.control_call_async(c, capi.default_params(alpha=alpha, n_tests=n_tests))
    got, cov = s.control_call_fetch()
    assert_table(got, cov, want, want_cov, (alpha, n_tests))


def test_a_table_beyond_cap_reports_the_full_count(ctxs, data):
    d = data["P67"]
    load(ctxs, d)
    s, c = ctxs
    want, want_cov = cm.call_rows(d["hs"], d["hc"], *d["pos"], 0.01, d["n_tests"])
    s.control_call_async(c, capi.default_params(alpha=0.01))
    for cap in (3, 0):
        rows, cov, n = np.zeros(max(cap, 1), dtype=capi.VARIANT), np.zeros(max(cap, 1), dtype=np.uint32), C.c_uint32()
        rc = s.lib.jl_control_call_fetch(s.h, rows.ctypes.data if cap else None, cov.ctypes.data if cap else None, cap, C.byref(n))
        assert rc == -5 and n.value == len(want) > 3
        assert b"capacity" in s.lib.jl_last_error(s.h)
        assert [int(r["codon"]) for r in rows[:cap]] == [w[4] for w in want[:cap]] and cov[:cap].tolist() == want_cov[:cap]
    got, cov = s.control_call_fetch()      # the full table is still there
    assert_table(got, cov, want, want_cov, "after the short fetches")


def test_the_call_stage_of_the_sample_is_untouched(ctxs, data):
    """jl_call_fetch returns the error-model table of jl_call_async, whatever the control call did in between."""
    d = data["P67"]
    load(ctxs, d)
    s, c = ctxs
    s.call_async(capi.default_params(alpha=0.01))
    before = s.call_fetch()
    s.control_call_async(c, capi.default_params(alpha=0.01))
    s.control_call_fetch()
    after = s.call_fetch()
    assert before.tobytes() == after.tobytes() and len(before) > 0


def refused(s, control_h, prm, status, word):
    rc = s.lib.jl_control_call_async(s.h, control_h, C.byref(prm) if prm is not None else None, None)
    msg = s.lib.jl_last_error(s.h).decode()
    assert rc == status and "jl_control_call_async" in msg and word in msg, (rc, msg)


def test_refusals(ctxs, data):
    s, c = ctxs
    d = data["P5"]
    prm = capi.default_params(alpha=0.01)
    fresh = capi.Juliet(0)
    try:
        fresh.upload_rows(d["C"])
        load(ctxs, d)
        refused(s, fresh.h, prm, -4, "control has no pileup")
        rc = fresh.lib.jl_control_call_async(fresh.h, s.h, C.byref(prm), None)
        assert rc == -4 and "sample has no pileup" in fresh.lib.jl_last_error(fresh.h).decode()
        rc = fresh.lib.jl_control_call_fetch(fresh.h, None, None, 0, C.byref(C.c_uint32()))
        assert rc == -4 and "before jl_control_call_async" in fresh.lib.jl_last_error(fresh.h).decode()
        refused(s, None, prm, -1, "no control")
        refused(s, c.h, None, -1, "no parameters")
        refused(s, c.h, capi.default_params(tail=1), -1, "tail")
        assert s.lib.jl_control_call_async(None, c.h, C.byref(prm), None) == -1
        assert b"no sample" in s.lib.jl_last_error(None)
        # another window: fewer columns
        fresh.upload_rows(d["C"][:, :63])
        fresh.pileup_async(d["genes"], d["refseq"])
        refused(s, fresh.h, prm, -4, "windows differ")
        # the same window, other genes
        fresh.upload_rows(d["C"])
        fresh.pileup_async(np.array([(1, 10)], dtype=capi.GENE), d["refseq"])
        refused(s, fresh.h, prm, -4, "position lists differ")
        # the same positions, another config codon (the sample is in majority mode)
        fresh.pileup_async(d["genes"], np.zeros(66, dtype=np.uint8))
        refused(s, fresh.h, prm, -4, "reference codons")
        assert s.lib.jl_control_call_fetch(s.h, None, None, 0, None) == -1
        if s.lib.jl_device_count() > 1:
            other = capi.Juliet(1)
            try:
                refused(s, other.h, prm, -1, "device")
            finally:
                other.close()
        # nothing of this left a result behind, and a good call still works
        s.control_call_async(c, prm)
        want, want_cov = cm.call_rows(d["hs"], d["hc"], *d["pos"], 0.01, d["n_tests"])
        got, cov = s.control_call_fetch()
        assert_table(got, cov, want, want_cov, "after the refusals")
    finally:
        fresh.close()
