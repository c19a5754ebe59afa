"""The Fisher routines over their whole count domain on the device: tests/golden/fisher_domain.json (exact arithmetic; the
design and its census are in tests/fisher_domain.py and tests/test_fisher_domain_host.py) through

  * fisher_eval_kernel: one launch per tail over the whole fixture;
  * the call stage, on designed windows (call_edges.rows_from_hists, one codon position per table) under error rows that make
    `expected` the fixture's c: call_kernel behind the pileup (jl_run_async) and the Fisher stage folded into the pileup
    launch's epilogue (a group of two windows).

Tolerances: P_ABS_TOL and LOGP_REL_TOL of test_gpu_parity.py, and on p the host's relative bound (test_fisher_host.py).
Runs only on a real MI355X: `pytest -m gpu`."""
import collections

import numpy as np
import pytest

import call_edges as ce
import fisher_domain as fd
from minorseq_amd import capi
from test_call_edges_host import expected_count
from test_gpu_parity import LOGP_REL_TOL, P_ABS_TOL

pytestmark = pytest.mark.gpu

P_REL_TOL = 5e-12     # the host bound (test_fisher_host.py)
REF = 27              # CGT
ALPHA, N_TESTS = 2.0, 1.0   # every observed codon is called (p <= 1 < alpha) and nothing is skipped: its row carries p itself


@pytest.fixture(scope="module")
def fx():
    return fd.load_fixture()


def check_values(p, lp, tables, where):
    """Device values against the exact ones; returns the worst relative error of p and the worst error of log_p in units of
    max(1, |ln p|)."""
    gp = np.array([float(t["p"]) for t in tables])
    glp = np.array([float(t["log_p"]) for t in tables])
    one = np.array(["early_one" in t["labels"] for t in tables])
    assert (p[one] == 1.0).all() and (lp[one] == 0.0).all(), where
    assert np.isfinite(lp).all() and np.isfinite(p).all(), where
    err_lp = np.abs(lp - glp) / np.maximum(1.0, np.abs(glp))
    big = gp > 1e-300
    rel = np.abs(p[big] - gp[big]) / gp[big]
    print("%s: %d tables, worst relative error of p %.3g, worst error of log_p %.3g" % (where, len(tables), rel.max(initial=0.0), err_lp.max()))
    k = int(np.argmax(err_lp))
    assert err_lp[k] <= LOGP_REL_TOL, (where, tables[k], lp[k])
    k = int(np.argmax(np.abs(p - gp)))
    assert abs(p[k] - gp[k]) <= P_ABS_TOL, (where, tables[k], p[k])
    if big.any():
        k = int(np.argmax(rel))
        assert rel[k] <= P_REL_TOL, (where, np.array(tables)[big][k], p[big][k])
    zero = np.array(["p_zero" in t["labels"] for t in tables])
    assert (p[zero] == 0.0).all(), where
    return rel.max(initial=0.0), err_lp.max()


def test_fisher_eval_over_the_whole_fixture(fx):
    """Two launches of fisher_eval_kernel: every table of the fixture at its tail.  Measured on an MI355X: worst relative error
    of p 2.31e-13 at either tail (the host build: 2.31e-13), worst error of log_p 2.4e-15 of max(1, |ln p|): the device meets
    the host bound, which therefore stands as it is."""
    jl = capi.Juliet(0)
    try:
        for tail in (0, 1):
            tables = [t for t in fx["tables"] if t["tail"] == tail]
            assert len(tables) > (700 if tail == 0 else 300)
            p, lp = jl.fisher_eval([t["a"] for t in tables], [t["c"] for t in tables], [t["n"] for t in tables], tail=tail)
            check_values(p, lp, tables, "fisher_eval tail %d" % tail)
    finally:
        jl.close()


# ------------------------------------------------------------------------------------------------ the call stage
def chosen(fx):
    """About 40 (table, tail) pairs with n <= 2907 and a >= 1: a + c > n, expected fractions up to 100 %, K = 63 .. 66."""
    ts = [t for t in fx["tables"] if t["a"] >= 1]
    lo = [t for t in ts if t["fam"] == "lo_pos" and t["n"] in (7, 40, 65, 100, 1000)]
    fr = [t for t in ts if t["fam"] == "fraction" and t["n"] in (64, 65, 1000, 2907)]
    dr = [t for t in ts if t["fam"] == "direct" and 63 <= t["a"] + t["c"] <= 66 and t["n"] <= 2907]
    full = [t for t in fr if t["c"] == t["n"] == 2907 and t["tail"] == 0 and t["a"] in (1453, 2907)]   # an expected fraction of 100 %
    out = lo[::13] + fr[::17] + full + dr[::4]
    return list({(t["a"], t["c"], t["n"], t["tail"]): t for t in out}.values())


def error_row(c, n):
    """match = 1: a codon with one substituted base has P_err = substitution, and ceil(n * (c - 1/2) / n) = c (the way
    make_call_edges_golden.py's CUSTOM row gives 30 at coverage 1000)."""
    return (1.0, (c - 0.5) / n if c else 0.0, 0.0)


def windows_of(tables):
    """One window per (c, n, tail): its error row is the one that makes `expected` c; one codon position per table."""
    j = next(k for k in range(64) if ce.n_substituted(REF, k) == 1)
    groups = collections.OrderedDict()
    for t in tables:
        groups.setdefault((t["c"], t["n"], t["tail"]), []).append(t)
    out = []
    for (c, n, tail), ts in groups.items():
        prm = dict(alpha=ALPHA, n_tests=N_TESTS, err=list(error_row(c, n)), expected_round=0, tail=tail, min_perc=-1.0, max_perc=-1.0)
        assert expected_count(n, REF, j, prm) == c, (c, n)
        cases = []
        for t in ts:
            hist = {k: v for k, v in ((j, t["a"]), (REF, n - t["a"])) if v}
            cases.append(dict(family=t["fam"], cov=n, ref=REF, ref_codon=REF, drm=None, extra=0, hist=hist, prm=prm, table=t,
                              codons={j: [c, ce.CALLED, t["p"], t["log_p"]]}))
        out.append(ce.Window(cases, seed=len(out)))
    return out


def capi_params(prm):
    m, s, d = prm["err"]
    return capi.Params(prm["alpha"], prm["n_tests"], capi.ErrorModel(m, s, d), prm["expected_round"], prm["tail"],
                       prm["min_perc"], prm["max_perc"])


def assert_rows(got, w, where):
    want = w.expected_rows()
    ints = [tuple(int(r[k]) for k in ("codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")) for r in got]
    assert ints == [r[:7] for r in want], where
    assert (got["gene"] == 0).all(), where
    check_values(np.array(got["p_value"]), np.array(got["log_p"]), [c["table"] for c in w.cases], where)


def test_chosen_tables_reach_the_new_region(fx):
    ts = chosen(fx)
    assert 35 <= len(ts) <= 60
    assert {t["fam"] for t in ts} == {"lo_pos", "fraction", "direct"} and {t["tail"] for t in ts} == {0, 1}
    assert max(t["n"] for t in ts) == 2907
    labels = set().union(*(t["labels"] for t in ts))
    assert {"lo_pos", "early_one", "direct_upper", "direct_lower", "saddle_upper", "saddle_lower"} <= labels
    assert {t["a"] + t["c"] for t in ts if t["fam"] == "direct"} >= {63, 64, 65, 66}
    assert max(t["c"] / t["n"] for t in ts if t["fam"] == "fraction") == 1.0
    assert max(3 * len(w.cases) for w in windows_of(ts)) <= 120


def test_run_calls_the_chosen_tables(fx):
    """jl_run_async on one context: call_kernel behind the pileup."""
    ws = windows_of(chosen(fx))
    jl = capi.Juliet(0)
    try:
        for w in ws:
            jl.upload_rows(w.rows)
            jl.run_async(w.genes, w.refseq, capi_params(w.prm), None, False, 10, False)
            assert jl.lib.jl_n_positions(jl.h) == w.P
            assert_rows(jl.call_fetch(), w, ("run", w.prm))
    finally:
        jl.close()


def test_group_of_two_windows_calls_the_chosen_tables(fx):
    """A group of two windows (the Fisher stage in the pileup launch's epilogue): every window's positions split over the two,
    the second half behind as many empty positions."""
    ws = windows_of(chosen(fx))
    ctxs = [capi.Juliet(0), capi.Juliet(0)]
    grp = capi.Group(ctxs)
    try:
        for w in ws:
            half = (len(w.cases) + 1) // 2
            a = ce.Window(w.cases[:half], seed=1)
            b = ce.Window(w.cases[half:] or w.cases, lead=a.P, seed=2)
            assert b.P > a.P
            for j, x in zip(ctxs, (a, b)):
                j.upload_rows(x.rows)
                j.sync()
            refseq = np.concatenate([a.refseq, b.refseq[3 * a.P:]])
            grp.run_async(b.genes, refseq, capi_params(w.prm), False, 10, False)
            for j, x in zip(ctxs, (a, b)):
                assert j.lib.jl_n_positions(j.h) == x.P
                assert_rows(j.call_fetch(), x, ("group", w.prm))
    finally:
        grp.close()
        for j in ctxs:
            j.close()
