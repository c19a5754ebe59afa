"""The call stage at its decision edges on the device: the cases of tests/golden/call_edges.json (exact arithmetic; see
tests/test_call_edges_host.py for the families) as designed matrices, one position per case, cases that share launch
parameters in one window, through every path that evaluates a position:

  * the stage API (upload_rows, pileup_async, call_async, call_fetch): call_kernel + compact_kernel;
  * jl_run_async without and with phasing (the compaction writes the result block / runs inside the phasing launch);
  * a group of two windows of different position counts, in both forms of a group run: the Fisher stage in the pileup
    launch's epilogue, and call_group_kernel + compact_group_kernel (JL_NO_FOLD_CALL, read once per process: a child process);

then one edge case repeated over position counts around the 4 positions of a call block and the 2048 positions of a compaction
pass, and the two-sided routine against the definition.  Rows must be the fixture's called set in table order; integers exactly,
p and log p within the tolerances of test_gpu_parity.py's golden test.  Runs only on a real MI355X: `pytest -m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import call_edges as ce
from minorseq_amd import capi

pytestmark = pytest.mark.gpu

P_ABS_TOL = 1e-10     # test_gpu_parity.py
P_REL_TOL = 1e-11


@pytest.fixture(scope="module")
def jl():
    j = capi.Juliet(0)
    yield j
    j.close()


@pytest.fixture(scope="module")
def fx():
    return ce.load_fixture()


@pytest.fixture(scope="module")
def windows(fx):
    """One window per set of launch parameters; the matrices are built once and shared by the tests."""
    return [ce.Window(cases, seed=key[0]) for key, cases in ce.batches(fx["cases"])]


def capi_params(prm):
    m, s, d = ce.error_row(prm)
    return capi.Params(prm["alpha"], prm["n_tests"], capi.ErrorModel(m, s, d), prm["expected_round"], prm["tail"],
                       prm["min_perc"], prm["max_perc"])


def assert_rows(got, want, where):
    ints = [tuple(int(r[k]) for k in ("codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")) for r in got]
    assert ints == [w[:7] for w in want], where
    assert (got["gene"] == 0).all(), where
    if not want:
        return
    gp = np.array([float(w[7]) for w in want])
    glp = np.array([float(w[8]) for w in want])
    assert np.abs(got["p_value"] - gp).max() <= P_ABS_TOL, where
    big = gp > 1e-300
    assert (np.abs(got["p_value"][big] - gp[big]) <= P_REL_TOL * gp[big]).all(), where
    assert (np.abs(got["log_p"] - glp) <= 1e-12 * np.maximum(1.0, np.abs(glp)) + 1e-13).all(), where


def test_fixture_is_laid_out_in_a_few_windows(windows, fx):
    assert sum(len(w.cases) for w in windows) == len(fx["cases"]) > 500
    assert {c["family"] for w in windows for c in w.cases} == set("abcdefgh")
    assert any(w.refseq is None for w in windows) and any(w.drm is not None for w in windows)
    assert max(w.rows.shape[0] for w in windows) == 100000 and max(w.rows.shape[1] for w in windows) < 400
    assert sum(len(w.expected_rows()) for w in windows) > 800


def test_stage_api_calls_the_fixtures_rows(jl, windows):
    for w in windows:
        jl.upload_rows(w.rows)
        jl.pileup_async(w.genes, w.refseq)
        assert jl.lib.jl_n_positions(jl.h) == w.P
        jl.call_async(capi_params(w.prm), w.drm)
        assert_rows(jl.call_fetch(), w.expected_rows(), w.prm)


@pytest.mark.parametrize("phasing", [False, True])
def test_run_calls_the_fixtures_rows(jl, windows, phasing):
    """jl_run_async: call_kernel behind the pileup in one enqueue; the table is compacted into the result block (no phasing)
    or inside the phasing launch.  Only the table is read back here."""
    for w in windows:
        jl.upload_rows(w.rows)
        jl.run_async(w.genes, w.refseq, capi_params(w.prm), w.drm, phasing, 10, phasing)
        assert_rows(jl.call_fetch(), w.expected_rows(), (w.prm, phasing))


@pytest.mark.parametrize("form", ["folded", "unfolded"])
def test_group_of_two_windows_calls_the_fixtures_rows(windows, form):
    """Every window's cases split over the two windows of a group: the first half, and the second half behind as many empty
    positions (so the windows differ in P and the grouped call launch has blocks past the shorter window's end)."""
    if form == "unfolded" and "JL_NO_FOLD_CALL" not in os.environ:   # the form is read once per process: a child process
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", __file__, "-k",
                            "test_group_of_two_windows_calls_the_fixtures_rows and unfolded"],
                           env=dict(os.environ, JL_NO_FOLD_CALL="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        return
    ctxs = [capi.Juliet(0), capi.Juliet(0)]
    grp = capi.Group(ctxs)
    try:
        for w in windows:
            half = (len(w.cases) + 1) // 2
            a = ce.Window(w.cases[:half], seed=1)
            b = ce.Window(w.cases[half:] or w.cases, lead=a.P, seed=2)
            assert b.P > a.P
            for j, x in zip(ctxs, (a, b)):
                j.upload_rows(x.rows)
                j.sync()
            refseq = b.refseq
            if refseq is not None:
                refseq = np.concatenate([a.refseq, b.refseq[3 * a.P:]])
            prm = capi_params(w.prm)
            if w.drm is not None:
                grp.run_masked_async(b.genes, refseq, prm, [a.drm, b.drm], False, 10, False)
            else:
                grp.run_async(b.genes, refseq, prm, False, 10, False)
            for j, x in zip(ctxs, (a, b)):
                assert j.lib.jl_n_positions(j.h) == x.P
                assert_rows(j.call_fetch(), x.expected_rows(), (w.prm, form))
    finally:
        grp.close()
        for j in ctxs:
            j.close()


@pytest.mark.parametrize("P", [1, 3, 4, 5, 2047, 2048, 2049, 4097])
def test_position_counts_around_the_block_and_the_pass(jl, fx, P):
    """h* - 1 and h* at coverage 64 over P positions: called positions first, last, at 2047 and at 2048 (the boundaries of the
    4-positions-a-block launch and of the 256 x 8 positions a compaction pass takes); everywhere else only h* - 1."""
    case = next(c for c in fx["cases"] if c["family"] == "a" and c["cov"] == 64 and len(c["codons"]) == 6)   # all three pairs
    quiet = dict(case, hist=dict(case["hist"]), codons={j: v for j, v in case["codons"].items() if v[1] == ce.NOT_SIGNIFICANT})
    for j, v in case["codons"].items():
        if v[1] == ce.CALLED:
            quiet["hist"][case["ref"]] += quiet["hist"].pop(j)
    assert len(quiet["codons"]) == 3 and sum(quiet["hist"].values()) == 64
    loud = sorted({0, P - 1} | {q for q in (2047, 2048) if q < P})
    w = ce.Window([case if p in loud else quiet for p in range(P)], seed=P)
    want = w.expected_rows()
    assert len(want) == 3 * len(loud) and w.rows.shape == (64, 3 * P)
    prm = capi_params(w.prm)
    jl.upload_rows(w.rows)
    jl.pileup_async(w.genes, w.refseq)
    assert jl.lib.jl_n_positions(jl.h) == P
    jl.call_async(prm)
    assert_rows(jl.call_fetch(), want, "stages")
    for phasing in (False, True):
        jl.run_async(w.genes, w.refseq, prm, None, phasing, 10, phasing)
        assert_rows(jl.call_fetch(), want, ("run", phasing))


def test_two_sided_on_the_device_against_the_definition(jl, fx):
    """jl_fisher_two_sided_equal_rows uses the symmetry of the equal-row table; the fixture sums, exactly, the tables no more
    likely than the observed one.  The one-sided routine over the rest of the fixture rides along."""
    for tail in (1, 0):
        tab = [(c["hist"][j], v, c["cov"], c["prm"]) for c in fx["cases"] if c["prm"]["tail"] == tail for j, v in c["codons"].items()]
        assert len(tab) > (30 if tail else 1500)
        p, lp = jl.fisher_eval([t[0] for t in tab], [t[1][0] for t in tab], [t[2] for t in tab], tail=tail)
        n_sig = 0
        for k, (h, v, cov, prm) in enumerate(tab):
            p_adj = min(1.0, p[k] * prm["n_tests"])
            assert (p_adj < prm["alpha"]) == (v[1] != ce.NOT_SIGNIFICANT), (h, v, cov, prm)
            if v[1] == ce.NOT_SIGNIFICANT:
                continue
            n_sig += 1
            gp, glp = float(v[2]), float(v[3])
            assert abs(p_adj - gp) <= P_ABS_TOL and (gp <= 1e-300 or abs(p_adj - gp) <= P_REL_TOL * gp), (h, v, cov, prm)
            assert abs(lp[k] - glp) <= 1e-12 * max(1.0, abs(glp)) + 1e-13, (h, v, cov, prm)
        assert n_sig > (15 if tail else 700)
