"""The general-margin Fisher routine over its whole count domain on the device: tests/golden/fisher_general_domain.json (exact
arithmetic; the design and its census are in tests/fisher_general_domain.py and tests/test_fisher_general_domain_host.py) through

  * control_eval_kernel (jl_control_eval): the whole fixture in one launch of the plain form and two of the skipping form;
  * control_call_kernel behind two pileups (jl_control_call_async): about 50 tables chosen by label, one codon position each, in
    windows built by control_mirror.rows_of_hists — one with coverages up to 70 000 and one of three positions whose 640 000
    reads on one side reach the direct product's fallback.

Bounds: test_control_host.py's (|dp| <= 1e-10, relative 5e-12 where p > 1e-300, |d ln p| <= 1e-12 max(1, |ln p|) + 1e-13).
Runs only on a real MI355X: `pytest -m gpu`."""
import collections

import numpy as np
import pytest

import control_mirror as cm
import fisher_general_domain as gd
from minorseq_amd import capi

pytestmark = pytest.mark.gpu

P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12
CODON, REF = 42, 0
ALPHA, N_TESTS = 2.0, 1.0   # every observed codon is called (p <= 1 < alpha) and nothing is skipped: its row carries p itself
MAX_COV, DEEP_COV, DEEP_MAX = 70000, 640000, 10 ** 6


@pytest.fixture(scope="module")
def fx():
    return gd.load_fixture()


def key(t):
    return t["a"], t["n"], t["c"], t["m"]


def check_values(p, lp, tables, where):
    """Device values against the exact ones; returns the worst relative error of p and the worst error of log_p in units of
    max(1, |ln p|), and prints where they occurred."""
    gp = np.array([float(t["p"]) for t in tables])
    glp = np.array([float(t["log_p"]) for t in tables])
    one = np.array(["early_one" in t["labels"] for t in tables])
    assert (p[one] == 1.0).all() and (lp[one] == 0.0).all(), where
    assert np.isfinite(lp).all() and np.isfinite(p).all(), where
    err_lp = np.abs(lp - glp)
    unit = err_lp / np.maximum(1.0, np.abs(glp))
    big = np.flatnonzero(gp > 1e-300)
    rel = np.abs(p[big] - gp[big]) / gp[big]
    kr, kl = big[int(np.argmax(rel))], int(np.argmax(unit))
    print("%s: %d tables, worst relative error of p %.3g at %s, worst error of log_p %.3g of max(1, |ln p|) at %s"
          % (where, len(tables), rel.max(), key(tables[kr]), unit[kl], key(tables[kl])))
    k = int(np.argmax(err_lp - (1e-12 * np.maximum(1.0, np.abs(glp)) + 1e-13)))
    assert err_lp[k] <= 1e-12 * max(1.0, abs(glp[k])) + 1e-13, (where, tables[k], lp[k])
    k = int(np.argmax(np.abs(p - gp)))
    assert abs(p[k] - gp[k]) <= P_ABS_TOL, (where, tables[k], p[k])
    assert rel.max() <= P_REL_TOL, (where, tables[kr], p[kr])
    zero = np.array(["p_zero" in t["labels"] for t in tables])
    assert (p[zero] == 0.0).all(), where
    return rel.max(), unit[kl]


def test_control_eval_over_the_whole_fixture(fx):
    """Three launches of control_eval_kernel: every table of the fixture, plain and gated.  Measured on an MI355X: worst relative
    error of p 6.56e-13 at (a, n, c, m) = (1546, 2000, 2454, 6000), worst error of ln p 3.96e-14 of max(1, |ln p|) at
    (2^26 + 1, 2^31 - 1, 2^26 + 1, 2^31 - 1) — the host build's figures: the device meets the host bounds, which stand."""
    tables = fx["tables"]
    cols = [[t[k] for t in tables] for k in ("a", "n", "c", "m")]
    jl = capi.Juliet(0)
    try:
        p, lp = jl.control_eval(*cols)
        check_values(p, lp, tables, "control_eval")
        for n_tests, alpha in ((1000.0, 0.01), (1e6, 0.01)):
            q, lq, sk = jl.control_eval(*cols, n_tests=n_tests, alpha=alpha)
            # where it does not skip: the plain launch's bits; where it skips: (1, 0), on the upper path, and never a call
            assert (q[~sk] == p[~sk]).all() and (lq[~sk] == lp[~sk]).all()
            assert (q[sk] == 1.0).all() and (lq[sk] == 0.0).all() and sk.sum() >= 50
            for t in np.array(tables)[sk]:
                assert "upper" in t["labels"] and min(1.0, float(t["p"]) * n_tests) >= alpha, t
            if n_tests == 1e6:   # the mean itself is the upper path (skipped here), one count below it is the lower one
                for k, t in enumerate(tables):
                    if t["fam"] == "mean" and "early_one" not in t["labels"]:
                        assert bool(sk[k]) == ("upper" in t["labels"]), t
    finally:
        jl.close()


# ------------------------------------------------------------------------------------------------ the control call's kernel
def chosen(fx):
    """(about 50 tables with both coverages up to MAX_COV: for every label the first two tables of the fixture that take it,
    three tables on each path of the direct product's fallback at DEEP_COV to DEEP_MAX reads)."""
    ts = [t for t in fx["tables"] if t["a"] >= 1]
    small = [t for t in ts if max(t["n"], t["m"]) <= MAX_COV]
    picked, have = {}, collections.Counter()
    for label in sorted(gd.all_labels()):
        for t in small:
            if have[label] >= 2:
                break
            if label in t["labels"] and key(t) not in picked:
                picked[key(t)] = t
                have.update(t["labels"])
    deep = [t for t in ts if DEEP_COV <= max(t["n"], t["m"]) <= DEEP_MAX and t["labels"] & {"direct_fallback:upper", "direct_fallback:lower"}]
    up = [t for t in deep if "direct_fallback:upper" in t["labels"]][:3]
    down = [t for t in deep if "direct_fallback:lower" in t["labels"]][:3]
    return list(picked.values()), up, down


def hists_of(tables):
    hs = np.zeros((len(tables), 64), dtype=np.int64)
    hc = np.zeros((len(tables), 64), dtype=np.int64)
    for p, t in enumerate(tables):
        hs[p][CODON], hs[p][REF] = t["a"], t["n"] - t["a"]
        hc[p][CODON], hc[p][REF] = t["c"], t["m"] - t["c"]
    return hs, hc


def test_chosen_tables_reach_what_the_kernel_must_see(fx):
    small, up, down = chosen(fx)
    assert 35 <= len(small) <= 70 and len(up) == 3 and len(down) == 3
    labels = set().union(*(t["labels"] for t in small))
    missing = gd.all_labels() - labels
    assert missing <= {"beyond_2^53", "direct_fallback:upper", "direct_fallback:lower", "stirlerr:s4@K"}, sorted(missing)
    assert any({"lo_pos", "lower"} <= t["labels"] for t in small) and any({"lo_pos", "upper"} <= t["labels"] for t in small)
    assert any(t["labels"] & {"zero_cell:%s" % v for v in gd.CELLS} for t in small)
    assert max(max(t["n"], t["m"]) for t in small) > 20000


@pytest.mark.parametrize("which", ["by_label", "fallback_upper", "fallback_lower"])
def test_control_call_kernel_on_the_chosen_tables(fx, which):
    """jl_control_call_async: every chosen table as one position of a sample and a control window; every row with == on its
    integers and the bounds on p and ln p.  Measured on an MI355X: worst relative error of p 1.6e-13 (at (64, 64, 0, 700000), the
    fallback on the upper path), worst error of ln p 1.0e-15 of max(1, |ln p|)."""
    tables = dict(zip(("by_label", "fallback_upper", "fallback_lower"), chosen(fx)))[which]
    hs, hc = hists_of(tables)
    P = len(tables)
    genes = np.array([(1, 3 * P + 1)], dtype=capi.GENE)
    refseq = np.zeros(3 * P, dtype=np.uint8)       # config codon AAA = 0
    s, c = capi.Juliet(0), capi.Juliet(0)
    try:
        s.upload_rows(cm.rows_of_hists(hs, seed=1))
        c.upload_rows(cm.rows_of_hists(hc, seed=2))
        s.pileup_async(genes, refseq)
        c.pileup_async(genes, refseq)
        s.control_call_async(c, capi.default_params(alpha=ALPHA, n_tests=N_TESTS))
        got, cov = s.control_call_fetch()
    finally:
        s.close()
        c.close()
    ints = [tuple(int(r[k]) for k in ("gene", "codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")) for r in got]
    assert ints == [(0, p + 1, 3 * p, REF, CODON, t["a"], t["n"], t["c"]) for p, t in enumerate(tables)]
    assert cov.tolist() == [t["m"] for t in tables]
    check_values(np.array(got["p_value"]), np.array(got["log_p"]), tables, "control_call_kernel " + which)
