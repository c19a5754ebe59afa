"""The general-margin Fisher test of the control call (docs/SPEC.md §21) without a GPU: csrc/jl_fisher_general.h compiled for the
host through tests/csrc/fisher_general_shim.cpp, and jl_control_test of the library (the same header inside libjuliet_hip.so),
against the 60-digit vectors of tests/golden/fisher_general_golden.json, against the equal-row routine of jl_fisher.h where
both rows sum to the same number, and against the exact rational mirror (control_mirror.py) at the decision edges.
The bounds are test_fisher_host.py's.  The device repeats the decisions in test_gpu_control.py."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import control_mirror as cm
from minorseq_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libfisher_general_shim.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(HERE, "csrc", "fisher_general_shim.cpp")])
    lib = C.CDLL(out)
    u32, dp = C.c_uint32, C.POINTER(C.c_double)
    lib.shim_fisher_general.restype = C.c_double
    lib.shim_fisher_general.argtypes = [u32, u32, u32, u32, dp]
    lib.shim_fisher_general_or_skip.restype = C.c_double
    lib.shim_fisher_general_or_skip.argtypes = [u32, u32, u32, u32, C.c_double, C.c_double, dp, C.POINTER(C.c_int)]
    lib.shim_fisher_equal_rows.restype = C.c_double
    lib.shim_fisher_equal_rows.argtypes = [u32, u32, u32, dp]
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "fisher_general_golden.json")) as f:
        return json.load(f)["tables"]


def check(p, lp, gp, glp, what):
    assert abs(p - gp) <= P_ABS_TOL, (what, p, gp)
    rel = abs(p - gp) / gp if gp > 1e-300 else 0.0
    assert rel <= P_REL_TOL, (what, p, gp, rel)
    assert abs(lp - glp) <= 1e-12 * max(1.0, abs(glp)) + 1e-13, (what, lp, glp)
    return rel


def test_golden_file_covers_the_margins(golden):
    assert 1000 < len(golden) <= 1500
    cov = {r["a"] + r["b"] for r in golden}
    assert {50, 2907, 6000, 100000, 10000000} <= cov
    ratios = {(r["c"] + r["d"]) / (r["a"] + r["b"]) for r in golden if r["a"] + r["b"] == 100000}
    assert {0.01, 0.1, 1.0, 10.0} <= ratios
    assert any(r["c"] == 0 for r in golden) and any(float(r["p"]) < 1e-300 for r in golden)
    assert sum(1 for r in golden if r["a"] + r["b"] <= 60 and r["c"] + r["d"] <= 60) > 100   # the tiny random ones


def test_header_vs_golden(shim, golden):
    worst, where = 0.0, None
    for r in golden:
        n, m = r["a"] + r["b"], r["c"] + r["d"]
        lp = C.c_double()
        p = shim.shim_fisher_general(r["a"], n, r["c"], m, C.byref(lp))
        rel = check(p, lp.value, float(r["p"]), float(r["log_p"]), r)
        if rel > worst:
            worst, where = rel, (r["a"], n, r["c"], m)
    print("checked", len(golden), "worst relative error", worst, "at (a, cov_s, c, cov_c) =", where)


def test_library_entry_vs_golden(golden):
    """jl_control_test: the header as the library compiles it (hipcc's host pass), n_tests = 1 so that p_value = p."""
    prm = capi.default_params(alpha=0.01)
    for r in golden:
        n, m = r["a"] + r["b"], r["c"] + r["d"]
        d = capi.control_test(r["a"], n, r["c"], m, prm, 1.0)
        assert (d["count"], d["coverage"], d["control_count"], d["control_coverage"]) == (r["a"], n, r["c"], m)
        if r["a"] == 0:
            assert (d["called"], d["p_value"], d["log_p"]) == (False, 1.0, 0.0)
            continue
        check(d["p_value"], d["log_p"], float(r["p"]), float(r["log_p"]), r)
        if abs(float(r["p"]) - 0.01) > 1e-8:
            assert d["called"] == (float(r["p"]) < 0.01), r


def test_skip_gate_never_changes_a_value_or_a_decision(shim, golden):
    """Where the gated form sums the tail it returns the ungated value bit for bit; where it skips, the codon is not called."""
    n_skipped = 0
    for n_tests, alpha in ((1.0, 0.01), (99.0, 0.01), (1000.0, 0.05)):
        for r in golden:
            if r["a"] == 0:
                continue
            n, m = r["a"] + r["b"], r["c"] + r["d"]
            lp, lq, sk = C.c_double(), C.c_double(), C.c_int()
            p = shim.shim_fisher_general(r["a"], n, r["c"], m, C.byref(lp))
            q = shim.shim_fisher_general_or_skip(r["a"], n, r["c"], m, n_tests, alpha, C.byref(lq), C.byref(sk))
            if sk.value:
                n_skipped += 1
                assert not min(1.0, p * n_tests) < alpha, r
                assert min(1.0, float(r["p"]) * n_tests) >= alpha, r
            else:
                assert (q, lq.value) == (p, lp.value), r
    assert n_skipped > 50


def test_equal_rows_agree_with_the_equal_row_routine(shim):
    rng = np.random.default_rng(7)
    tabs = [(int(a), int(c), int(n)) for n in (1, 2, 50, 65, 2907, 100000, 10000000)
            for a, c in zip(rng.integers(0, min(n, 400) + 1, 40), rng.integers(0, min(n, 90) + 1, 40))]
    tabs += [(n, n, n) for n in (1, 50, 6000)] + [(n // 2, n // 2, n) for n in (50, 6000, 100000)]
    for a, c, n in tabs:
        le, lg = C.c_double(), C.c_double()
        pe = shim.shim_fisher_equal_rows(a, c, n, C.byref(le))
        pg = shim.shim_fisher_general(a, n, c, n, C.byref(lg))
        check(pg, lg.value, pe, le.value, (a, c, n))


@pytest.mark.parametrize("alpha,n_tests", [(0.01, 1.0), (0.01, 99.0), (0.05, 3000.0), (1e-6, 1.0)])
def test_decision_edges_against_exact_arithmetic(alpha, n_tests):
    tabs = cm.edge_tables(alpha, n_tests)
    assert len(tabs) >= 8
    prm = capi.default_params(alpha=alpha)
    for n, m, c, a in tabs:
        below, at = capi.control_test(a - 1, n, c, m, prm, n_tests), capi.control_test(a, n, c, m, prm, n_tests)
        assert (below["called"], at["called"]) == (False, True), (n, m, c, a)
        want = float(min(Fraction(1), cm.exact_p(a, n, c, m) * Fraction(n_tests)))
        assert abs(at["p_value"] - want) <= P_REL_TOL * want


def test_tight_edges_alpha_either_side_of_p():
    """alpha a relative 4e-6 above and below the exact adjusted p of a small table: called, then not."""
    for n, m, c, a, n_tests in ((40, 40, 0, 6, 1.0), (64, 23, 1, 20, 7.0), (200, 64, 2, 30, 99.0), (1000, 100, 5, 120, 3.0)):
        adj = cm.exact_p(a, n, c, m) * Fraction(n_tests)
        assert adj < 1
        for f, want in ((1 + 4e-6, True), (1 - 4e-6, False)):
            alpha = float(adj) * f
            assert abs(Fraction(alpha) - adj) / adj >= Fraction(cm.MIN_GAP)
            assert capi.control_test(a, n, c, m, capi.default_params(alpha=alpha), n_tests)["called"] == want, (n, m, c, a)


def test_filters_skips_and_errors():
    prm = capi.default_params(alpha=0.01, min_perc=10.0)
    assert capi.control_test(30, 1000, 0, 1000, capi.default_params(), 1.0)["called"]
    assert not capi.control_test(30, 1000, 0, 1000, prm, 1.0)["called"]            # 3 % is not above --min-perc 10
    assert not capi.control_test(30, 1000, 0, 1000, capi.default_params(max_perc=3.0), 1.0)["called"]   # strict
    for a, n, c, m in ((0, 10, 5, 10), (0, 0, 0, 10), (5, 10, 0, 0)):
        d = capi.control_test(a, n, c, m, capi.default_params(), 1.0)
        assert (d["called"], d["p_value"], d["log_p"]) == (False, 1.0, 0.0)
    d = capi.control_test(1000, 1000, 0, 100000000, capi.default_params(), 1.0)   # p underflows to 0: called (log p carries it)
    assert d["called"] and d["p_value"] == 0.0 and d["log_p"] < -745.0
    for args, prm_, n_tests in (((5, 10, 0, 10), capi.default_params(tail=1), 1.0), ((5, 10, 0, 10), capi.default_params(), 0.0),
                                ((11, 10, 0, 10), capi.default_params(), 1.0), ((5, 10, 11, 10), capi.default_params(), 1.0)):
        with pytest.raises(capi.JulietError) as e:
            capi.control_test(*args, prm_, n_tests)
        assert e.value.status == -1 and "jl_control_test" in str(e.value)
