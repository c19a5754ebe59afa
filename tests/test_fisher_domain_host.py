"""The Fisher routines the device compiles (csrc/jl_fisher.h through tests/csrc/fisher_shim.cpp) over their whole count domain,
without a GPU: tests/golden/fisher_domain.json (exact arithmetic, made by tests/golden/make_fisher_domain_golden.py from the
design in tests/fisher_domain.py) against

  * the design: the fixture is `tables()`, and a census over `classify` shows that every selection rule of the header (direct
    products | saddle-point form, upper | lower tail, lo > 0, every form of stirlerr and bd0 for every argument, the fallback,
    the early break, the underflow of p, the renormalisation, the two-sided cases) is taken by at least three tables, the switch
    points from both sides;
  * the plain, the two-sided and the skipping form, at test_fisher_host.py's tolerances;
  * jl_deletion_test and jl_insertion_test at rates that reproduce the fixture's expected counts.

tests/test_gpu_fisher_domain.py sends the same tables through the kernels."""
import collections
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deletion_mirror as dm
import fisher_domain as fd
from minorseq_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))

# the host tolerances of this routine (test_fisher_host.py)
P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12
DENORMAL_QUANTUM = 2.0 ** -1074


def logp_tol(glp):
    return 1e-12 * max(1.0, abs(glp)) + 1e-13


def underflow_tol(gp, glp):
    """Where p leaves the normal range it is exp(log_p) rounded to the denormal grid: log_p's own tolerance carried through exp,
    and one quantum of that grid."""
    return gp * math.expm1(logp_tol(glp)) + DENORMAL_QUANTUM


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libfisher_shim.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out,
                           os.path.join(HERE, "csrc", "fisher_shim.cpp")])
    lib = C.CDLL(out)
    u, d = C.c_uint32, C.c_double
    for name in ("shim_fisher", "shim_fisher_two_sided"):
        getattr(lib, name).restype = d
        getattr(lib, name).argtypes = [u, u, u, C.POINTER(d)]
    lib.shim_fisher_or_skip.restype = d
    lib.shim_fisher_or_skip.argtypes = [u, u, u, d, d, C.POINTER(d), C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope="module")
def fx():
    return fd.load_fixture()


def evaluate(shim, t):
    lp = C.c_double()
    fn = shim.shim_fisher_two_sided if t["tail"] else shim.shim_fisher
    return fn(t["a"], t["c"], t["n"], C.byref(lp)), lp.value


def check_value(p, lp, t):
    """One table against its exact value; returns the relative error of p (0 where it is not defined)."""
    gp, glp = float(t["p"]), float(t["log_p"])
    if "early_one" in t["labels"]:
        assert (p, lp) == (1.0, 0.0) == (gp, glp), t
        return 0.0
    assert abs(lp - glp) <= logp_tol(glp), (t, lp, glp)
    assert abs(p - gp) <= P_ABS_TOL, (t, p, gp)
    if t["labels"] & {"p_zero", "p_denormal"}:
        assert gp < 2.0 ** -1022
        assert p == 0.0 or abs(p - gp) <= underflow_tol(gp, glp), (t, p, gp)
        if "p_zero" in t["labels"]:
            assert p == 0.0 and math.isfinite(lp), (t, p, lp)
        return 0.0
    if gp > 1e-300:
        assert abs(p - gp) <= P_REL_TOL * gp, (t, p, gp)
        return abs(p - gp) / gp
    return 0.0


# ------------------------------------------------------------------------------------------------ the design and its census
def test_mirrored_constants_are_the_headers():
    with open(os.path.join(HERE, "..", "minorseq_amd", "csrc", "jl_fisher.h")) as f:
        text = f.read()
    assert [float(v) for v in re.findall(r"if \(K <= ([\d.]+)\)", text)] == [float(fd.K_DIRECT)] * 2
    assert re.search(r"constexpr double tab\[%d\]" % (fd.STIRLERR_LAST[0] + 1), text)
    assert re.search(r"if \(n < %d\.0\) return tab\[\(int\)n\];" % (fd.STIRLERR_LAST[0] + 1), text)
    series = re.findall(r"if \(n > ([\d.]+)\) return \(S0", text)
    assert [float(v) for v in series] == [float(v) for v in reversed(fd.STIRLERR_LAST[1:])]
    assert re.search(r"if \(fabs\(x - np\) < ([\d.]+) \* \(x \+ np\)\)", text).group(1) == repr(fd.BD0_SERIES)
    assert [float(v) for v in re.findall(r"if \(term < sum \* ([\de.-]+)\) break;", text)] == [fd.BREAK_EPS] * 3
    assert [float(v) for v in re.findall(r"return lp < (-[\d.]+) \? 0\.0", text)] == [fd.LOGP_ZERO] * 2
    assert re.search(r"if \(\+\+pending == %d\)" % fd.BATCH, text)
    assert text.count("if (a <= lo) { *logp = 0.0; return 1.0; }") == 2
    assert fd.LN_DBL_MIN == math.log(2.0 ** -1022) and fd.K_DIRECT % fd.BATCH == 0
    # stirlerr's table is ln n! - ln(sqrt(2 pi n) (n / e)^n)
    tab = [float(v) for v in re.search(r"tab\[16\] = \{([^}]*)\}", text).group(1).split(",")]
    assert len(tab) == 16 and tab[0] == 0.0
    for k in range(1, 16):
        assert abs(tab[k] - (math.lgamma(k + 1) - (0.5 * math.log(2 * math.pi * k) + k * (math.log(k) - 1.0)))) < 2e-14, k


def test_fixture_is_the_design(fx):
    assert fx["k_max"] == fd.K_MAX
    got = [(t["fam"], t["a"], t["c"], t["n"], t["tail"]) for t in fx["tables"]]
    assert got == fd.tables() and len(set(r[1:] for r in got)) == len(got)
    assert 1000 < len(got) <= 2500
    for fam in fd.FAMILIES:
        assert sum(1 for r in got if r[0] == fam and r[4] == 0) >= 15, fam
    assert all(r[1] + r[2] <= fd.K_MAX or r[1:] == (10 ** 7, 1, 10 ** 7, 0) for r in got)
    two = [r for r in got if r[4] == 1]
    one = {r[1:4] for r in got if r[4] == 0 and r[0] in ("lo_pos", "fraction") and r[1] + r[2] <= fd.K_TWO_SIDED}
    assert {r[1:4] for r in two} == one and len(two) > 300


def test_design_holds_what_the_issue_lists(fx):
    rows = [(t["a"], t["c"], t["n"]) for t in fx["tables"] if t["tail"] == 0]
    lo_pos = [(a, c, n) for a, c, n in rows if a + c > n]
    for n in (1, 2, 7, 40, 63, 64, 65, 100, 1000):
        excess = {a + c - n for a, c, m in lo_pos if m == n}
        assert {v for v in (1, 2, n // 2, n - 1, n) if 1 <= v <= n} <= excess, n
        assert (n, n, n) in rows
        if n > 2:   # both sides of a == c, the early return (a == lo, c == n) and the count above it
            assert {np.sign(a - c) for a, c, m in lo_pos if m == n} == {-1, 0, 1}, n
            assert any(c == n and a < n for a, c, m in lo_pos if m == n) and any(c == n - 1 for a, c, m in lo_pos if m == n), n
    assert any(a + c <= 64 for a, c, n in lo_pos) and any(a + c > 64 for a, c, n in lo_pos)
    for n in (64, 65, 1000, 2907, 20000, 100000):
        for num, den in fd.FRACTIONS:
            c = fd.fraction_count(n, num, den)
            counts = {a for a, cc, m in rows if m == n and cc == c}
            assert ({1, c} <= counts) if 2 * c <= fd.K_MAX else (1 in counts or c + 1 > fd.K_MAX), (n, c)
            if 2 * c + 1 <= min(fd.K_MAX, 2 * n):
                assert {c - 1, c + 1, min(2 * c, n)} <= counts, (n, c)
    for K in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66):
        for n in (K, K + 1, 2907, 10 ** 7):
            assert {a for a, c, m in rows if m == n and a + c == K} >= {K // 2, K - 1, K}, (K, n)
    # ln p in every range of the underflow family, at both coverages and both expected counts where the range can be reached
    under = [t for t in fx["tables"] if t["fam"] == "underflow"]
    for lo_, hi_ in fd.UNDERFLOW_RANGES:
        hit = {(t["n"], t["c"]) for t in under if lo_ < float(t["log_p"]) < hi_}
        want = {(n, c) for n in (2907, 100000) for c in (1, 30) if hi_ > -1e4 or n == 100000}
        assert want <= hit, (lo_, hi_, hit)
    assert any(t["n"] == 10 ** 7 == t["a"] for t in under)


def test_census_every_label_is_reached(fx):
    census = collections.Counter()
    by_family = collections.defaultdict(collections.Counter)
    for t in fx["tables"]:
        census.update(t["labels"])
        by_family[t["fam"]].update(t["labels"])
    universe = fd.all_labels()
    print("census of %d tables over %d labels" % (len(fx["tables"]), len(universe)))
    for label in sorted(universe):
        print("  %-22s %5d   %s" % (label, census[label], " ".join("%s %d" % (f, by_family[f][label]) for f in fd.FAMILIES if by_family[f][label])))
    assert not set(census) - universe, sorted(set(census) - universe)      # nothing declared unreachable is reached
    assert not [l for l in universe if census[l] < 3], sorted((l, census[l]) for l in universe if census[l] < 3)


def test_census_switch_points_come_in_pairs(fx):
    """Every stirlerr argument sits ON each border it can reach (the last argument of one form, the first of the next), and every
    bd0 argument changes form between two neighbouring integers at the same mean, below the mean and above it."""
    args = [fd.saddle_args(t["a"], t["c"], t["n"]) for t in fx["tables"] if t["tail"] == 0]
    args = [d for d in args if d is not None]
    seen = {name: {d[name] for d in args} for name in fd.STIRLERR_ARGS}
    for name in fd.STIRLERR_ARGS:
        for last in fd.STIRLERR_LAST:
            first = last + 1 if name != "M" else last + 2 - last % 2     # M = 2n is even
            at = last if name != "M" else last - last % 2
            if "stirlerr:%s@%s" % (fd.stirlerr_form(at), name) in fd.UNREACHABLE:
                assert not [v for v in seen[name] if v <= last], (name, last)
                continue
            assert {at, first} <= seen[name], (name, last)
            assert fd.stirlerr_form(at) != fd.stirlerr_form(first)
    calls = [fd.bd0_calls(t["a"], t["c"], t["n"]) for t in fx["tables"] if t["tail"] == 0]
    for name in fd.BD0_ARGS:
        forms = {(v, np_): fd.bd0_form(v, np_) for d in calls if d is not None for v, np_ in [d[name]]}
        flips = [(v, np_) for (v, np_), form in forms.items() if forms.get((v + 1, np_), form) != form]
        assert any(v < np_ for v, np_ in flips) and any(v > np_ for v, np_ in flips), (name, flips)
        for v, np_ in flips:   # ... and the flip is the one at 9/11 or 11/9
            assert (v / np_ < 9 / 11 < (v + 1) / np_) or (v / np_ < 11 / 9 < (v + 1) / np_), (name, v, np_)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("fam", fd.FAMILIES)
def test_values_vs_fixture(shim, fx, fam):
    worst, n = 0.0, 0
    for t in fx["tables"]:
        if t["fam"] == fam:
            worst = max(worst, check_value(*evaluate(shim, t), t))
            n += 1
    print("%s: %d tables, worst relative error of p %.3g" % (fam, n, worst))
    assert n >= 15


N_TESTS_ALPHA = ((1.0, 0.01), (1000.0, 0.01), (0.5, 0.3))


def test_or_skip_returns_the_plain_forms_bits_and_skips_only_what_cannot_be_called(shim, fx):
    n_skipped = collections.Counter()
    for t in fx["tables"]:
        if t["tail"]:
            continue
        plain = evaluate(shim, t)
        for n_tests, alpha in N_TESTS_ALPHA:
            lp, sk = C.c_double(), C.c_int()
            p = shim.shim_fisher_or_skip(t["a"], t["c"], t["n"], n_tests, alpha, C.byref(lp), C.byref(sk))
            if sk.value:
                n_skipped[(n_tests, alpha)] += 1
                assert min(Fraction(1), Fraction(t["p"]) * Fraction(n_tests)) >= Fraction(alpha), (t, n_tests, alpha)
                assert t["a"] > t["c"] and (p, lp.value) == (1.0, 0.0)
            else:
                assert (p, lp.value) == plain, (t, n_tests, alpha)
    # (a point mass above the mean is at most 1/2: at n_tests = 0.5 against alpha = 0.3 nothing may be skipped)
    assert n_skipped[(1.0, 0.01)] >= 50 and n_skipped[(1000.0, 0.01)] >= 50 and n_skipped[(0.5, 0.3)] == 0, n_skipped


# ------------------------------------------------------------------------------------------------ the product's entry points
def rate_for(c, n, mode):
    """A rate whose expected count round_mode(n * rate) is c: the middle of the interval that each rounding rule of
    deletion_mirror.expected maps to c (0 ceil: (c - 1, c]; 1 floor: [c, c + 1); 2 floor(x + 0.5): [c - 1/2, c + 1/2))."""
    if mode == 0:
        return (c - 0.5) / n if c else 0.0
    if mode == 1:
        return (c + 0.5) / n if c < n else 1.0
    return c / n


@pytest.mark.parametrize("entry", ["deletion", "insertion"])
def test_product_entry_points_vs_fixture(fx, entry):
    n_checked = 0
    fractions = collections.Counter()
    for k, t in enumerate(fx["tables"]):
        if t["fam"] != "fraction":
            continue
        a, c, n, tail = t["a"], t["c"], t["n"], t["tail"]
        mode = k % 3
        rate = rate_for(c, n, mode)
        assert 0.0 <= rate <= 1.0 and dm.expected(n, rate, mode) == c, (t, mode, rate)   # (insertion_mirror takes the same rule)
        if entry == "deletion":
            prm = capi.Params(2.0, 1.0, capi.ErrorModel(0.99, 0.001, rate), mode, tail, -1.0, -1.0)
            got = capi.deletion_test((n - a, a, 0, n), prm, 1.0)
        else:
            prm = capi.Params(2.0, 1.0, capi.ErrorModel(0.99, 0.001, 0.0), mode, tail, -1.0, -1.0)
            got = capi.insertion_test(a, (n + 5, a, 2, 3), prm, rate, 1.0)
        assert (got["count"], got["coverage"], got["expected"]) == (a, n, c), (t, got)
        assert got["called"] == (a > 0)                     # alpha = 2: everything observed is called
        check_value(got["p_value"], got["log_p"], t)        # n_tests = 1: p_value is p
        fractions[(c, n)] += 1
        n_checked += 1
    assert n_checked > 400 and len(fractions) >= 30
