"""The general-margin Fisher routine the device compiles (csrc/jl_fisher_general.h through tests/csrc/fisher_general_shim.cpp, and
inside the library behind jl_control_test) over its whole count domain, without a GPU: tests/golden/fisher_general_domain.json
(exact arithmetic, made by tests/golden/make_fisher_general_domain_golden.py from the design in tests/fisher_general_domain.py)
against

  * the design: the fixture is `tables()`, and a census over `classify` shows that every selection rule of the header (early
    return, upper | lower tail, the mean itself, lo > 0, direct product | its fallback on either path | saddle-point form, every
    zero cell, every form of stirlerr and bd0 for every argument, the renormalisation, the early break, the underflow of p,
    products beyond 2^53) is taken by at least three tables, the switch points from both sides;
  * the plain and the skipping form at test_control_host.py's bounds, through the shim and through jl_control_test.

Measured on the host: worst relative error of p 6.6e-13 at (a, n, c, m) = (1546, 2000, 2454, 6000), worst error of ln p 4.0e-14
of max(1, |ln p|) at (2^26 + 1, 2^31 - 1, 2^26 + 1, 2^31 - 1) (test_values_vs_fixture prints both for every family).  tests/test_gpu_fisher_general_domain.py sends the same tables through the kernels."""
import collections
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import pytest

import fisher_general_domain as gd
from minorseq_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minorseq_amd", "csrc")

# the bounds of test_control_host.py
P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12
DENORMAL_QUANTUM = 2.0 ** -1074


def logp_tol(glp):
    return 1e-12 * max(1.0, abs(glp)) + 1e-13


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
    return lib


@pytest.fixture(scope="module")
def fx():
    return gd.load_fixture()


def key(t):
    return t["a"], t["n"], t["c"], t["m"]


def evaluate(shim, t):
    lp = C.c_double()
    return shim.shim_fisher_general(*key(t), C.byref(lp)), lp.value


def check_value(p, lp, t):
    """One table against its exact value at the bounds of test_control_host.py; returns (relative error of p, error of ln p in
    units of max(1, |ln p|)), 0 where not defined."""
    gp, glp = float(t["p"]), float(t["log_p"])
    if "early_one" in t["labels"]:
        assert (p, lp) == (1.0, 0.0) == (gp, glp), t
        return 0.0, 0.0
    assert abs(lp - glp) <= logp_tol(glp), (t, lp, glp)
    assert abs(p - gp) <= P_ABS_TOL, (t, p, gp)
    err_lp = abs(lp - glp) / max(1.0, abs(glp))
    if "p_zero" in t["labels"]:
        assert p == 0.0 and math.isfinite(lp), (t, p, lp)
    if gp > 1e-300:
        assert abs(p - gp) <= P_REL_TOL * gp, (t, p, gp, abs(p - gp) / gp)
        return abs(p - gp) / gp, err_lp
    return 0.0, err_lp


# ------------------------------------------------------------------------------------------------ the design and its census
def test_mirrored_constants_are_the_headers():
    with open(os.path.join(CSRC, "jl_fisher_general.h")) as f:
        text = f.read()
    direct = re.findall(r"const bool direct = K <= ([\d.]+) && \(pm = jl_pmf_general_small\(\w+, K, n, m\)\) > ([\de.-]+);", text)
    assert [(float(k), float(v)) for k, v in direct] == [(float(gd.K_DIRECT), gd.PMF_MIN)] * 2
    assert [float(v) for v in re.findall(r"if \(term < sum \* ([\de.-]+)\) break;", text)] == [gd.BREAK_EPS] * 2
    assert [float(v) for v in re.findall(r"return lp < (-[\d.]+) \? 0\.0", text)] == [gd.LOGP_ZERO]
    assert [float(v) for v in re.findall(r"l0 > (-[\d.]+)\)", text)] == [gd.LOGP_GATE]
    assert re.findall(r"if \(\+\+pending == (\d+)\)", text) == [str(gd.BATCH)]
    assert text.count("if (a <= lo) { *logp = 0.0; return 1.0; }") == 1
    assert text.count("const bool upper = (uint64_t)a_ * m_ >= (uint64_t)n_ * c_;") == 1
    assert gd.LN_DBL_MIN == math.log(2.0 ** -1022) and gd.K_DIRECT % gd.BATCH == 0
    with open(os.path.join(CSRC, "jl_fisher.h")) as f:       # stirlerr and bd0 are jl_fisher.h's
        text = f.read()
    assert re.search(r"if \(n < %d\.0\) return tab\[\(int\)n\];" % (gd.STIRLERR_LAST[0] + 1), text)
    series = re.findall(r"if \(n > ([\d.]+)\) return \(S0", text)
    assert [float(v) for v in series] == [float(v) for v in reversed(gd.STIRLERR_LAST[1:])]
    assert re.search(r"if \(fabs\(x - np\) < ([\d.]+) \* \(x \+ np\)\)", text).group(1) == repr(gd.BD0_SERIES)


def test_fixture_is_the_design(fx):
    got = [(t["fam"],) + key(t) for t in fx["tables"]]
    assert got == gd.tables() and len(set(r[1:] for r in got)) == len(got)
    assert 1000 < len(got) <= gd.MAX_TABLES
    for fam in gd.FAMILIES:
        assert sum(1 for r in got if r[0] == fam) >= 15, fam
    assert set(gd.UNREACHABLE) <= {"lower_is_one"} | {"stirlerr:%s@%s" % (f, v) for f in gd.STIRLERR_FORMS for v in gd.STIRLERR_ARGS}


def test_design_holds_what_it_promises(fx):
    rows = {key(t) for t in fx["tables"]}
    ratios = {Fraction(n, m) for a, n, c, m in rows}
    assert {Fraction(1), Fraction(1, 10 ** 4), Fraction(10 ** 4), Fraction(1, 10 ** 8), Fraction(10 ** 8), Fraction(1, 10), Fraction(10),
            Fraction(1, 100), Fraction(100)} <= ratios
    for rows_of in ({n for a, n, c, m in rows}, {m for a, n, c, m in rows}):
        assert {1, 10 ** 7} <= rows_of and any(10 < v < 100 for v in rows_of) and any(1000 < v < 10 ** 5 for v in rows_of)
    for n, m in gd.EXTREME:                                       # K = 1 .. 66 at each extreme ratio
        assert {a + c for a, n_, c, m_ in rows if (n_, m_) == (n, m)} >= set(range(1, 67)), (n, m)
    for n, m in gd.MARGINS:                                       # a at lo, lo + 1, either side of the mean, hi
        for K in gd.totals_of(n, m):
            lo, hi, mean = max(K - m, 0), min(K, n), K * n // (n + m)
            have = {a for a, n_, c, m_ in rows if (n_, m_, a + c) == (n, m, K)}
            assert {lo, min(lo + 1, hi), hi, min(max(mean - 1, lo), hi), min(max(mean + 1, lo), hi)} <= have, (n, m, K)
    beyond = [t for t in fx["tables"] if t["fam"] == "beyond"]
    assert len(beyond) >= 100 and all("beyond_2^53" in t["labels"] and min(t["n"], t["m"]) >= 10 ** 8 for t in beyond)
    assert any(t["a"] * (t["n"] + t["m"]) > gd.TWO_53 for t in beyond)
    # ln p in every range of the underflow family, for every (n, c, m) where the range can be reached; and far beyond
    under = [t for t in fx["tables"] if t["fam"] == "underflow"]
    for lo_, hi_ in gd.UNDERFLOW_RANGES:
        assert len({(t["n"], t["m"]) for t in under if lo_ < float(t["log_p"]) < hi_}) >= 3, (lo_, hi_)
    assert min(float(t["log_p"]) for t in fx["tables"]) < -1e6
    # the lower tail with lo > 0, and the exact mean with a count to either side
    assert sum(1 for t in fx["tables"] if {"lower", "lo_pos"} <= t["labels"]) >= 20
    for t in fx["tables"]:
        if t["fam"] == "mean" and "mean_exact" in t["labels"]:
            a, n, c, m = key(t)
            assert (a - 1, n, c, m) in rows and (a + 1, n, c, m) in rows
            assert "lower" in gd.classify(a - 1, n, c, m) and "upper" in gd.classify(a + 1, n, c, m)


def test_census_every_label_is_reached(fx):
    census = collections.Counter()
    by_family = collections.defaultdict(collections.Counter)
    for t in fx["tables"]:
        census.update(t["labels"])
        by_family[t["fam"]].update(t["labels"])
    universe = gd.all_labels()
    print("census of %d tables over %d labels" % (len(fx["tables"]), len(universe)))
    for label in sorted(universe):
        print("  %-24s %5d   %s" % (label, census[label], " ".join("%s %d" % (f, by_family[f][label]) for f in gd.FAMILIES if by_family[f][label])))
    for label, why in sorted(gd.UNREACHABLE.items()):
        print("  %-24s unreachable: %s" % (label, why))
    assert not set(census) - universe, sorted(set(census) - universe)      # nothing declared unreachable is reached
    assert not [l for l in universe if census[l] < 3], sorted((l, census[l]) for l in universe if census[l] < 3)
    # the fallback with every zero cell it can meet, lo > 0 on both paths, the mean itself on both forms of the point mass
    for pair in (("direct_fallback:upper", "zero_cell:c"), ("direct_fallback:lower", "zero_cell:x"), ("lo_pos", "upper"),
                 ("lo_pos", "lower"), ("mean_exact", "direct"), ("mean_exact", "saddle"), ("mean_exact", "beyond_2^53"),
                 ("beyond_2^53", "lower"), ("beyond_2^53", "break"), ("saddle", "p_zero"), ("direct_fallback:upper", "p_zero")):
        assert sum(1 for t in fx["tables"] if set(pair) <= t["labels"]) >= 3, pair


def test_census_switch_points_come_in_pairs(fx):
    """Every stirlerr argument sits ON each border it can reach (the last argument of one form) and on the first of the next,
    and every bd0 cell changes form between two neighbouring integers at the same mean, below the mean and above it."""
    args = [d for d in (gd.saddle_args(*key(t)) for t in fx["tables"]) if d is not None]
    seen = {name: {d[name] for d in args} for name in gd.STIRLERR_ARGS}
    for name in gd.STIRLERR_ARGS:
        for last in gd.STIRLERR_LAST:
            if "stirlerr:%s@%s" % (gd.stirlerr_form(last), name) in gd.UNREACHABLE:
                assert not [v for v in seen[name] if v <= last], (name, last)
                continue
            if (name, last) == ("K", 35):
                assert {34, 35, 36} <= seen[name] and min(seen[name]) == 33     # s4 | s3 through the fallback only
                continue
            assert {last, last + 1} <= seen[name], (name, last)
    calls = [gd.bd0_calls(*key(t)) for t in fx["tables"]]
    for name in gd.CELLS:
        forms = {(v, np_): gd.bd0_form(v, np_) for d in calls if d is not None and name in d for v, np_ in [d[name]]}
        flips = [(v, np_) for (v, np_), form in forms.items() if forms.get((v + 1, np_), form) != form]
        assert any(v < np_ for v, np_ in flips) and any(v > np_ for v, np_ in flips), (name, flips)
        for v, np_ in flips:   # ... and the flip is the one at 9/11 or 11/9
            assert (v / np_ < 9 / 11 < (v + 1) / np_) or (v / np_ < 11 / 9 < (v + 1) / np_), (name, v, np_)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("fam", gd.FAMILIES)
def test_values_vs_fixture(shim, fx, fam):
    worst, worst_lp, n = (0.0, ()), (0.0, ()), 0
    for t in fx["tables"]:
        if t["fam"] == fam:
            rel, err_lp = check_value(*evaluate(shim, t), t)
            worst, worst_lp = max(worst, (rel, key(t))), max(worst_lp, (err_lp, key(t)))
            n += 1
    print("%s: %d tables, worst relative error of p %.3g at %s, worst error of ln p %.3g of max(1, |ln p|) at %s"
          % (fam, n, worst[0], worst[1], worst_lp[0], worst_lp[1]))
    assert n >= 15


def test_library_entry_vs_fixture(fx):
    """jl_control_test: the header as the library compiles it (hipcc's host pass), n_tests = 1 so that p_value = p."""
    prm = capi.default_params(alpha=0.01)
    for t in fx["tables"]:
        a, n, c, m = key(t)
        d = capi.control_test(a, n, c, m, prm, 1.0)
        assert (d["count"], d["coverage"], d["control_count"], d["control_coverage"]) == (a, n, c, m)
        if a == 0:
            assert (d["called"], d["p_value"], d["log_p"]) == (False, 1.0, 0.0)
            continue
        check_value(d["p_value"], d["log_p"], t)
        if abs(float(t["p"]) - 0.01) > 1e-8:
            assert d["called"] == (float(t["p"]) < 0.01), t


N_TESTS_ALPHA = ((1.0, 0.01), (1000.0, 0.01), (1e6, 0.01), (0.5, 0.6))


def test_or_skip_returns_the_plain_forms_bits_and_skips_only_what_cannot_be_called(shim, fx):
    n_skipped = collections.Counter()
    for t in fx["tables"]:
        plain = evaluate(shim, t)
        for n_tests, alpha in N_TESTS_ALPHA:
            lp, sk = C.c_double(), C.c_int()
            p = shim.shim_fisher_general_or_skip(*key(t), n_tests, alpha, C.byref(lp), C.byref(sk))
            if sk.value:
                n_skipped[(n_tests, alpha)] += 1
                assert min(Fraction(1), Fraction(t["p"]) * Fraction(n_tests)) >= Fraction(alpha), (t, n_tests, alpha)   # never a call
                assert "upper" in t["labels"] and (p, lp.value) == (1.0, 0.0), t
            else:
                assert (p, lp.value) == plain, (t, n_tests, alpha)
            if (n_tests, alpha) == (1e6, 0.01) and t["fam"] == "mean" and "early_one" not in t["labels"]:
                # at the mean and above it the point mass (at least 1e-5 here) times 1e6 is 1: skipped; one count below the mean
                # the lower path is taken, which never skips
                assert bool(sk.value) == ("upper" in t["labels"]) and float(t["p"]) > 0.2, t
    # (a point mass is at most 1: at n_tests = 0.5 against alpha = 0.6 nothing may be skipped)
    assert min(n_skipped[k] for k in N_TESTS_ALPHA[:3]) >= 50 and n_skipped[(0.5, 0.6)] == 0, n_skipped


def test_direct_products_on_equal_rows_are_the_equal_row_routines_bits(shim):
    """With both rows of n reads and K <= 64 the header multiplies the factors jl_fisher.h's direct product multiplies, in its
    order and with its renormalisation every 16 factors, and a tail of one or no term has no early break to differ by: the two
    routines return the same bits for K up to 64 — and only there: from K = 65 both take their own saddle-point expression.  (The
    direct form and the saddle-point form agree far inside every tolerance, so only bits can tell which of them K = 64 takes.)"""
    shim.shim_fisher_equal_rows.restype = C.c_double
    shim.shim_fisher_equal_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    same = {}
    for K in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 80):
        same[K] = True
        for n in (100, 2907):
            for a, c in ((K, 0), (K - 1, 1)):
                le, lg = C.c_double(), C.c_double()
                pe = shim.shim_fisher_equal_rows(a, c, n, C.byref(le))
                pg = shim.shim_fisher_general(a, n, c, n, C.byref(lg))
                same[K] &= (pe, le.value) == (pg, lg.value)
    assert all(same[K] for K in same if K <= gd.K_DIRECT), same
    assert not any(same[K] for K in same if K > gd.K_DIRECT), same
