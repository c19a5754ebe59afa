"""The call stage at its decision edges, without a GPU: tests/golden/call_edges.json (exact arithmetic, made by
tests/golden/make_call_edges_golden.py) against

  * itself: every decision re-made from Python integers, the margin, the SPEC §5 anchor;
  * the Fisher routines the device compiles (csrc/jl_fisher.h through tests/csrc/fisher_shim.cpp), above all
    jl_fisher_greater_equal_rows_or_skip, the one call_eval.h calls;
  * a restatement of jl_call_position (call_eval.h) in Python on top of that shim: expected count, shortcut, gate, filters,
    DRM mask, majority codon with ties, in the order the device takes them;
  * the oracle on the matrices tests/call_edges.py builds from the designed histograms.

Families of the fixture: a the edge h* - 1 | h*; b the edge across K = 64 | 65; c counts at or below the expected one (the
shortcut); d tail = 1; e degenerate tables; f majority ties; g filters at equality; h DRM masks.
tests/test_gpu_call_edges.py runs the same cases through the kernels."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import call_edges as ce
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = "abcdefgh"
REF_MAJORITY, REF_SKIP = 64, 65

# the host tolerances of this routine (test_fisher_host.py)
P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12


def logp_tol(glp):
    return 1e-12 * max(1.0, abs(glp)) + 1e-13


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
    return ce.load_fixture()


def greater(shim, a, c, n):
    lp = C.c_double()
    return shim.shim_fisher(a, c, n, C.byref(lp)), lp.value


def two_sided(shim, a, c, n):
    lp = C.c_double()
    return shim.shim_fisher_two_sided(a, c, n, C.byref(lp)), lp.value


def or_skip(shim, a, c, n, n_tests, alpha):
    lp, sk = C.c_double(), C.c_int()
    p = shim.shim_fisher_or_skip(a, c, n, n_tests, alpha, C.byref(lp), C.byref(sk))
    return p, lp.value, bool(sk.value)


def of_family(fx, fam):
    cases = [c for c in fx["cases"] if c["family"] == fam]
    assert cases
    return cases


def expected_count(cov, ref, j, prm):
    """SPEC §5 in IEEE double: products left to right, the three rounding modes, the clamp."""
    match, sub = ce.error_row(prm)[:2]
    perr = 1.0
    for sh in (4, 2, 0):
        perr = perr * (match if ((ref >> sh) & 3) == ((j >> sh) & 3) else sub)
    x = float(cov) * perr
    r = math.floor(x) if prm["expected_round"] == 1 else (math.floor(x + 0.5) if prm["expected_round"] == 2 else math.ceil(x))
    return int(min(max(r, 0), cov))


# ------------------------------------------------------------------------------------------------ the helper
def test_rows_from_hists_gives_the_histograms_asked_for(oracle):
    rng = np.random.default_rng(5)
    hists = [{j: 1 + (7 * j) % 5 for j in range(64)},          # all 64 codons present
             {},                                               # `extra` only
             {63: 1}, {0: 300, 21: 1}, {}, {17: 8200, 18: 3}]
    extra = [3, 11, 0, 20, 0, 1]
    hists += [{int(j): int(v) for j, v in zip(rng.choice(64, 5, replace=False), rng.integers(1, 400, 5))} for _ in range(6)]
    extra += [int(x) for x in rng.integers(0, 30, 6)]
    rows = ce.rows_from_hists(hists, extra, seed=3)
    need = [sum(h.values()) + x for h, x in zip(hists, extra)]
    assert rows.shape == (max(need), 3 * len(hists)) and rows.dtype == np.uint8
    hist, cov = oracle.codon_hist(rows, np.arange(len(hists)) * 3)
    for p, h in enumerate(hists):
        want = np.zeros(64, dtype=np.uint32)
        for j, v in h.items():
            want[j] = v
        assert (hist[p] == want).all(), p
        assert cov[p] == sum(h.values())
        blk = rows[:, 3 * p: 3 * p + 3]
        assert ((blk != 6).any(axis=1)).sum() <= need[p]            # reads the position does not need carry code 6
        assert ((blk == 6).all(axis=1)).sum() >= rows.shape[0] - need[p]
    # the extra reads are there and are skipped: a deletion, an N or nothing in one column
    blk = rows[:, 3:6]
    assert ((blk != 6).any(axis=1)).sum() >= 11 - 2 and {4, 5} <= set(np.unique(blk))
    # the reads of a position are shuffled, and differently from position to position
    r0 = np.nonzero((rows[:, 9:12] != 6).any(axis=1))[0]
    assert len(r0) == 321 and not (np.diff(r0) == 1).all()
    assert (ce.rows_from_hists(hists, extra, seed=3) == rows).all()
    assert ce.rows_from_hists([], None).shape == (0, 0)


def test_every_fixture_window_has_its_histograms(fx, oracle):
    for key, cases in ce.batches(fx["cases"]):
        w = ce.Window(cases, seed=key[0])
        hist, cov = oracle.codon_hist(w.rows, np.arange(w.P) * 3)
        for p, c in enumerate(cases):
            assert cov[p] == c["cov"] == sum(c["hist"].values())
            assert {j: int(v) for j, v in enumerate(hist[p]) if v} == c["hist"]


# ------------------------------------------------------------------------------------------------ the fixture against itself
def pmf_weight(x, K, n):
    """P(X = x) * (2n)!/(2n-K)!, afresh for every x (no recurrence: the generator walks one)."""
    return math.comb(K, x) * math.perm(n, x) * math.perm(n, K - x)


def exact_p(a, c, n, tail):
    K = a + c
    lo, hi = max(0, K - n), min(K, n)
    D = math.perm(2 * n, K)
    if tail == 0:
        return Fraction(sum(pmf_weight(x, K, n) for x in range(max(a, lo), hi + 1)), D)
    wa = pmf_weight(a, K, n)
    return Fraction(sum(w for w in (pmf_weight(x, K, n) for x in range(lo, hi + 1)) if w <= wa), D)


def exact_decision(case, j):
    prm, h, cov = case["prm"], case["hist"][j], case["cov"]
    e = expected_count(cov, case["ref_codon"], j, prm)
    p_adj = min(Fraction(1), exact_p(h, e, cov, prm["tail"]) * Fraction(prm["n_tests"]))
    ratio = p_adj / Fraction(prm["alpha"])
    if not p_adj < Fraction(prm["alpha"]):
        return e, ce.NOT_SIGNIFICANT, ratio
    perc = Fraction(100 * h, cov)
    keep = not (prm["min_perc"] >= 0 and not perc > Fraction(prm["min_perc"]))
    keep = keep and not (prm["max_perc"] >= 0 and not perc < Fraction(prm["max_perc"]))
    keep = keep and not (case["drm"] is not None and not (case["drm"] >> j) & 1)
    return e, (ce.CALLED if keep else ce.FILTERED), ratio


@pytest.mark.parametrize("fam", FAMILIES)
def test_fixture_decisions_remade_from_integers(fx, fam):
    assert fx["dropped"] == 0
    for c in of_family(fx, fam):
        assert c["cov"] == sum(c["hist"].values())
        if c["ref"] is None:   # majority codon: lowest index on ties; none without a read
            top = max(c["hist"].values(), default=0)
            assert c["ref_codon"] == min((j for j, v in c["hist"].items() if v == top), default=None)
        tested = sorted(j for j in c["hist"] if j != c["ref_codon"]) if c["ref_codon"] is not None else []
        assert sorted(c["codons"]) == tested
        for j in tested:
            e, decision, ratio = exact_decision(c, j)
            assert c["codons"][j][:2] == [e, decision], (c, j)
            assert abs(ratio - 1) >= Fraction(1, 10 ** 6), (c, j)      # the margin a case needs to enter
            assert (len(c["codons"][j]) == 4) == (decision != ce.NOT_SIGNIFICANT)


def test_fixture_holds_the_spec_anchor(fx):
    """SPEC §5: coverage 2907, `sequel`, n_tests in [982, 1884], alpha 0.01: 21 reads are called, 20 are not."""
    seen = set()
    for c in of_family(fx, "a"):
        p = c["prm"]
        if c["cov"] == 2907 and p["err"] == "sequel" and p["alpha"] == 0.01 and p["n_tests"] in (1000.0, 1884.0) and p["expected_round"] == 0:
            one = {c["hist"][j]: v[1] for j, v in c["codons"].items() if ce.n_substituted(c["ref"], j) == 1}
            assert one == {20: ce.NOT_SIGNIFICANT, 21: ce.CALLED}
            seen.add(p["n_tests"])
    assert seen == {1000.0, 1884.0}


def test_fixture_covers_what_each_family_is_for(fx):
    a = of_family(fx, "a")
    combos = {(c["cov"], c["prm"]["n_tests"], c["prm"]["alpha"], c["prm"]["err"]) for c in a if c["prm"]["expected_round"] == 0}
    assert len({k for k in combos if k[0] in (1, 2, 7, 64, 65, 1000, 2907, 17241, 17242, 17300, 100000)}) == 11 * 4 * 3 * 2
    for c in a:   # every position: per number of substituted bases the pair (h* - 1, h*), or the one count there is
        for s in (1, 2, 3):
            d = sorted((c["hist"][j], v[1]) for j, v in c["codons"].items() if ce.n_substituted(c["ref"], j) == s)
            h0 = d[0][0] if d else 0
            assert d in ([], [(h0, 0)], [(h0, 1)], [(h0, 0), (h0 + 1, 1)]), (c, s)
    # `expected` steps from 1 to 2 between 17242 and 17300 (sequel, one substitution), and the three rounding modes are there
    e1 = {c["cov"]: v[0] for c in a for j, v in c["codons"].items()
          if c["prm"]["err"] == "sequel" and c["prm"]["expected_round"] == 0 and ce.n_substituted(c["ref"], j) == 1}
    assert e1[17241] == 1 and e1[17242] == 1 and e1[17300] == 2 and e1[100000] == 6
    assert {c["prm"]["expected_round"] for c in a} == {0, 1, 2}
    rounded = {(c["prm"]["expected_round"], c["cov"]): next(iter(c["codons"].values()))[0] for c in a if c["cov"] in (8640, 8641, 17281, 17282)}
    assert [rounded[(r, n)] for r in (0, 1, 2) for n in (8640, 8641, 17281, 17282)] == [1, 1, 1, 2, 0, 0, 0, 1, 0, 1, 1, 1]
    # b: K = count + expected on both sides of 64 | 65, the decision changing between them
    ks = sorted(sorted(c["hist"][j] + v[0] for j, v in c["codons"].items()) for c in of_family(fx, "b"))
    assert ks == [[63, 64], [64, 65], [64, 65], [65, 66], [65, 66], [66, 67]]
    assert all(sorted(v[1] for v in c["codons"].values()) == [0, 1] for c in of_family(fx, "b"))
    # c: counts at or below the expected one, behind the shortcut (never called) and in front of it (some called)
    behind = [c for c in of_family(fx, "c") if min(1.0, 0.5 * c["prm"]["n_tests"]) >= c["prm"]["alpha"]]
    front = [c for c in of_family(fx, "c") if not min(1.0, 0.5 * c["prm"]["n_tests"]) >= c["prm"]["alpha"]]
    assert len(behind) >= 3 and len(front) >= 4
    at = lambda cs, d: {(c["hist"][j] - v[0]) for c in cs for j, v in c["codons"].items() if v[1] == d and c["hist"][j] <= v[0]}
    assert not at(behind, ce.CALLED) and {0, -1} <= at(behind, ce.NOT_SIGNIFICANT)
    assert {0, -1} <= at(front, ce.CALLED) and at(front, ce.NOT_SIGNIFICANT)
    # d: called above and below the expected count, never at it
    d = of_family(fx, "d")
    assert all(c["prm"]["tail"] == 1 for c in d)
    side = {(np.sign(c["hist"][j] - v[0]), v[1]) for c in d for j, v in c["codons"].items()}
    assert side == {(1, 0), (1, 1), (-1, 0), (-1, 1), (0, 0)}
    # e: h == cov with the reference codon unobserved, coverage 1, e == cov, positions without a read (with a reference and without)
    e = of_family(fx, "e")
    assert {c["cov"] for c in e if len(c["hist"]) == 1 and c["ref"] not in c["hist"]} >= {1, 2, 7, 64, 1000}
    assert any(v[0] == c["cov"] for c in e for v in c["codons"].values())
    assert {c["ref"] is None for c in e if c["cov"] == 0} == {True, False} and any(c["extra"] for c in e if c["cov"] == 0)
    assert {c["prm"]["tail"] for c in e} == {0, 1}
    # f: ties at (0, 63), (5, 6), (62, 63), three ways, all 64; one read; a tied codon called against the lowest one
    f = of_family(fx, "f")
    tied = [tuple(sorted(j for j, v in c["hist"].items() if v == max(c["hist"].values()))) for c in f]
    assert {(0, 63), (5, 6), (62, 63), (9, 33, 58), tuple(range(64)), (37,)} <= set(tied)
    assert all(c["ref"] is None and c["ref_codon"] == t[0] for c, t in zip(f, tied))
    assert any(c["codons"][63][1] == ce.CALLED for c in f if c["ref_codon"] == 0)
    # g: a percentage equal to a bound is filtered, one count either side is kept / filtered as the bound says
    g = of_family(fx, "g")
    eq = [(c, j) for c in g for j in c["codons"]
          if Fraction(100 * c["hist"][j], c["cov"]) in (Fraction(c["prm"]["min_perc"]), Fraction(c["prm"]["max_perc"]))]
    assert len(eq) >= 12 and all(c["codons"][j][1] == ce.FILTERED for c, j in eq)
    assert all(100.0 * c["hist"][j] / c["cov"] in (c["prm"]["min_perc"], c["prm"]["max_perc"]) for c, j in eq)   # exact in binary
    assert any(c["prm"]["min_perc"] >= 0 and c["prm"]["max_perc"] >= 0 and ce.CALLED in [v[1] for v in c["codons"].values()] for c in g)
    # h: masks of codon 0 alone, codon 63 alone, nothing
    h = of_family(fx, "h")
    assert {1, 1 << 63, 0} <= {c["drm"] for c in h}
    for c in h:
        assert all((v[1] == ce.CALLED) == bool((c["drm"] >> j) & 1) for j, v in c["codons"].items()), c
        assert all(v[1] != ce.NOT_SIGNIFICANT for v in c["codons"].values())


# ------------------------------------------------------------------------------------------------ the routines the device compiles
def check_value(p_adj, lp, v, where):
    gp, glp = float(v[2]), float(v[3])
    assert abs(p_adj - gp) <= P_ABS_TOL, where
    if gp > 1e-300:
        assert abs(p_adj - gp) <= P_REL_TOL * gp, (where, p_adj, gp)
    assert abs(lp - glp) <= logp_tol(glp), (where, lp, glp)


@pytest.mark.parametrize("fam", FAMILIES)
def test_fisher_routines_vs_fixture(shim, fx, fam):
    """The skipping form the kernel calls (tail 0) and the two-sided form (tail 1), codon by codon: a skipped codon is one the
    fixture does not call; a value that is returned is bit for bit the one of the plain form (the header's promise); the
    decision min(1, p n_tests) < alpha is the exact one; values of significant codons are the 60-digit ones."""
    n_skipped = n_values = 0
    for c in of_family(fx, fam):
        prm = c["prm"]
        for j, v in c["codons"].items():
            a, e, n = c["hist"][j], v[0], c["cov"]
            if prm["tail"] == 0:
                p, lp, skipped = or_skip(shim, a, e, n, prm["n_tests"], prm["alpha"])
                if skipped:
                    n_skipped += 1
                    assert v[1] == ce.NOT_SIGNIFICANT, (c, j)
                    continue
                assert (p, lp) == greater(shim, a, e, n), (c, j)
            else:
                p, lp = two_sided(shim, a, e, n)
            p_adj = min(1.0, p * prm["n_tests"])
            assert (p_adj < prm["alpha"]) == (v[1] != ce.NOT_SIGNIFICANT), (c, j, p_adj)
            if v[1] != ce.NOT_SIGNIFICANT:
                check_value(p_adj, lp, v, (c, j))
                n_values += 1
    if fam == "a":
        assert n_skipped > 100 and n_values > 100   # the count below the edge is what the gate is for


def test_gate_skips_only_what_cannot_be_called(shim):
    """The gate compares the point mass with alpha (1 + 1e-6).  Where the tail IS the point mass (the count is the largest
    the table allows) p == pmf in the same floating-point expressions, so alpha a hair above p n_tests must still call it and
    alpha at p n_tests must not; over both pmf branches (K <= 64 direct products, above it the saddle-point form)."""
    for a, c, n in ((1, 0, 1), (7, 1, 7), (20, 0, 20), (40, 3, 40), (64, 0, 64), (65, 0, 65), (60, 7, 60), (300, 2, 300), (20, 30, 1000)):
        p0, lp0 = greater(shim, a, c, n)
        for n_tests in (1.0, 50.0, 0.5):
            x = p0 * n_tests
            if not 0.0 < x < 0.5:
                continue
            for alpha in (x * (1 + 1e-9), x * (1 + 1e-7), x * (1 + 1e-5), x * 2, math.nextafter(x, 1.0), x, x * (1 - 1e-9), x / 2):
                p, lp, skipped = or_skip(shim, a, c, n, n_tests, alpha)
                if x < alpha:
                    assert not skipped and (p, lp) == (p0, lp0), (a, c, n, n_tests, alpha)
                else:
                    assert skipped or (p, lp) == (p0, lp0)
    # and over tables with a real tail: skipped implies that the plain form's p_adj does not reach below alpha
    rng = np.random.default_rng(11)
    n_skipped = 0
    for _ in range(4000):
        n = int(rng.integers(1, 50000))
        c = int(rng.integers(0, min(n, 40) + 1))
        a = int(rng.integers(1, min(n, 120) + 1))
        p0, lp0 = greater(shim, a, c, n)
        n_tests = float(rng.choice([0.5, 1.0, 50.0, 1884.0]))
        for alpha in (0.01, 0.3, min(1.0, p0 * n_tests) * (1 + 1e-7), min(1.0, p0 * n_tests) * (1 - 1e-7)):
            if alpha <= 0.0:
                continue
            p, lp, skipped = or_skip(shim, a, c, n, n_tests, alpha)
            n_skipped += skipped
            if skipped:
                assert not min(1.0, p0 * n_tests) < alpha, (a, c, n, n_tests, alpha)
            else:
                assert (p, lp) == (p0, lp0)
    assert n_skipped > 1000


# ------------------------------------------------------------------------------------------------ jl_call_position, restated
def call_position(shim, hist, refcfg, prm, drm):
    """call_eval.h's jl_call_position for one position: -> (ref, [(codon, count, expected, p_adj, log_p)] of the called codons)."""
    alpha, n_tests = prm["alpha"], prm["n_tests"]
    cov = sum(hist)
    ref = refcfg
    if ref == REF_MAJORITY:
        best = max((h << 8) | (63 - lane) for lane, h in enumerate(hist))
        ref = 63 - (best & 0xFF) if cov else REF_SKIP
    rows = []
    for lane, h in enumerate(hist):
        if not (ref < 64 and h > 0 and lane != ref):
            continue
        e = expected_count(cov, ref, lane, prm)
        called, p_adj, lp = False, 1.0, 0.0
        if prm["tail"] == 0:
            floor_adj = 0.5 * n_tests if 0.5 * n_tests < 1.0 else 1.0
            if h > e or not floor_adj >= alpha:
                pv, lp, skipped = or_skip(shim, h, e, cov, n_tests, alpha)
                p_adj = min(1.0, pv * n_tests)
                called = not skipped and p_adj < alpha
        else:
            pv, lp = two_sided(shim, h, e, cov)
            p_adj = min(1.0, pv * n_tests)
            called = p_adj < alpha
        perc = 100.0 * float(h) / float(cov)
        if prm["min_perc"] >= 0.0 and not perc > prm["min_perc"]:
            called = False
        if prm["max_perc"] >= 0.0 and not perc < prm["max_perc"]:
            called = False
        if drm is not None and not (drm >> lane) & 1:
            called = False
        if called:
            rows.append((lane, h, e, p_adj, lp))
    return ref, rows


@pytest.mark.parametrize("fam", FAMILIES)
def test_call_position_restated_gives_the_fixture(shim, fx, fam):
    for c in of_family(fx, fam):
        hist = [c["hist"].get(j, 0) for j in range(64)]
        ref, rows = call_position(shim, hist, REF_MAJORITY if c["ref"] is None else c["ref"], c["prm"], c["drm"])
        assert ref == (REF_SKIP if c["ref_codon"] is None else c["ref_codon"]), c
        want = [(j, c["hist"][j], v[0]) for j, v in sorted(c["codons"].items()) if v[1] == ce.CALLED]
        assert [r[:3] for r in rows] == want, c
        for r in rows:
            check_value(r[3], r[4], c["codons"][r[0]], (c, r[0]))


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_params(prm):
    m, s, d = ce.error_row(prm)
    return oracle_lib.Params(prm["alpha"], prm["n_tests"], oracle_lib.ErrorModel(m, s, d), prm["expected_round"], prm["tail"])


@pytest.mark.parametrize("fam", FAMILIES)
def test_oracle_gives_the_fixture(fx, oracle, fam):
    """oracle.call on the designed matrices: its rows are the significant codons (the filters and the DRM mask are applied
    behind it), decided as the exact arithmetic decides; `expected` too."""
    for key, cases in ce.batches(of_family(fx, fam)):
        w = ce.Window(cases, seed=key[0])
        prm = oracle_params(w.prm)
        got = oracle.call(w.rows, w.genes, refseq=w.refseq, params=prm)
        want = w.expected_rows(keep=(ce.CALLED, ce.FILTERED))
        assert [tuple(int(r[k]) for k in ("codon_pos", "col", "ref_codon", "codon", "count", "coverage", "expected")) for r in got] == \
            [r[:7] for r in want], (key, w.prm)
        assert (got["gene"] == 0).all()
        for r, x in zip(got, want):
            gp, glp = float(x[7]), float(x[8])
            assert abs(r["p_value"] - gp) <= 1e-10 and abs(r["log_p"] - glp) <= 1e-9 * max(1.0, abs(glp)), (x, r)
        for c in cases:
            for j, v in c["codons"].items():
                assert oracle.expected(prm, c["cov"], c["ref_codon"], j) == v[0]
