"""The host-only half of the codon deletion calls (docs/SPEC.md §16): the mirror itself on rows small enough to count by hand, and
the test of one position (jl_deletion_test) against the mirror's exact arithmetic at the edge of a call.  No GPU: the library only
has to load."""
import ctypes as C
import math

import numpy as np
import pytest

import deletion_mirror as dm
from minorseq_amd import capi

A, C_, G, T, GAP, N, OUT = 0, 1, 2, 3, 4, 5, 6
NAMES = ("jl_codon_deletions_async", "jl_codon_deletions_fetch", "jl_deletion_test")


def one(*codes):
    """The counts of ONE read, as a list of (codon, del3, partial, span) per codon start."""
    return dm.counts(np.array([codes], dtype=np.uint8)).tolist()


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
def test_mirror_clean_deletion():
    assert one(GAP, GAP, GAP) == [[0, 1, 0, 1]]


def test_mirror_two_bases_deleted():
    assert one(GAP, GAP, A) == [[0, 0, 1, 1]]


def test_mirror_one_base_deleted_either_end():
    rows = np.array([[GAP, A, C_], [A, C_, GAP]], dtype=np.uint8)
    assert dm.counts(rows).tolist() == [[0, 0, 2, 2]]


def test_mirror_n_counts_in_span_only():
    assert one(N, GAP, GAP) == [[0, 0, 0, 1]]
    assert one(N, A, A) == [[0, 0, 0, 1]]
    assert one(A, GAP, N) == [[0, 0, 0, 1]]


def test_mirror_uncovered_cell_counts_nowhere():
    assert one(A, OUT, A) == [[0, 0, 0, 0]]
    assert one(GAP, GAP, OUT) == [[0, 0, 0, 0]]
    assert one(OUT, N, GAP) == [[0, 0, 0, 0]]


def test_mirror_six_base_deletion_reports_at_both_codons():
    """A C G | - - - | - - - | T T T: del3 at the two in-frame starts 3 and 6 and at the start between them in every frame; the
    starts that straddle an end of the deletion see a partly deleted codon."""
    got = one(A, C_, G, GAP, GAP, GAP, GAP, GAP, GAP, T, T, T)
    codon, del3, partial, span = (list(x) for x in zip(*got))
    assert codon == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert del3 == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert partial == [0, 1, 1, 0, 0, 0, 0, 1, 1, 0]
    assert span == [1] * 10


def test_mirror_three_base_deletion_out_of_frame():
    """A gene in frame 0 (starts 0, 3, 6), the deletion at columns 4..6: partial at two of the gene's positions, del3 at none of
    them — and del3 at start 4, which is another frame's."""
    got = one(A, C_, G, T, GAP, GAP, GAP, A, A)
    assert [got[c] for c in (0, 3, 6)] == [[1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1]]
    assert [c for c in range(7) if got[c][dm.DEL3]] == [4]


def test_mirror_a_read_counts_in_at_most_one_of_the_three():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 7, size=(400, 9), dtype=np.uint8)
    cnt = dm.counts(rows).astype(np.int64)
    assert (cnt[:, :3].sum(axis=1) <= cnt[:, 3]).all() and cnt[:, :3].min(axis=0).min() >= 0 and (cnt[:, 1] > 0).any()
    with_gap = np.array([(rows[:, c:c + 3] == GAP).any(axis=1).sum() for c in range(7)])
    assert (cnt[:, 1] + cnt[:, 2] <= with_gap).all()


# ---------------------------------------------------------------------------------------------- jl_deletion_test
def test_exports_and_struct():
    lib = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert C.sizeof(capi.DeletionCall) == 40


def check_against_exact(cnt, prm, n_tests):
    got = capi.deletion_test(cnt, prm, n_tests)
    exp = dm.test(cnt, prm.err.deletion, n_tests, prm.alpha, prm.expected_round, prm.tail == 1, prm.min_perc, prm.max_perc)
    for key in ("count", "coverage", "expected", "partial", "called"):
        assert got[key] == exp[key], (key, cnt, got, exp)
    p_adj, p = float(exp["p_adj"]), float(exp["p"])
    if p_adj > 1e-300:                       # tests/test_fisher_host.py's tolerances for the same routines
        assert abs(got["p_value"] - p_adj) <= 5e-12 * p_adj, (cnt, got["p_value"], p_adj)
    if p > 1e-300:
        lp = math.log(p)
        assert abs(got["log_p"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13, (cnt, got["log_p"], lp)
    return got


# (expected_round, tail): all three round modes and both tails at every coverage up to 3000; the exact sums are long integers of
# 15 000 and 60 000 digits at the two deep coverages, which get three combinations each — all modes and both tails again
MODES = {10: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)], 600: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)],
         3000: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)], 25000: [(0, 0), (1, 1), (2, 0)], 100000: [(0, 1), (1, 0), (2, 1)]}


@pytest.mark.parametrize("coverage", [10, 600, 3000, 25000, 100000])
@pytest.mark.parametrize("chemistry", ["sequel", "permissive"])
def test_edge_of_a_call_against_exact_arithmetic(coverage, chemistry):
    """The smallest called count — found by the exact mirror, not by the code under test — and the count below it."""
    n_tests = 4.0 if coverage == 10 else 1090.0               # (ten reads cannot reach 0.01 / 1090: 11 / C(20, 10) is 6e-5)
    for rnd, tail in MODES[coverage]:
        prm = capi.default_params(chemistry=chemistry, expected_round=rnd, tail=tail)
        edge = dm.smallest_called(coverage, prm.err.deletion, n_tests, prm.alpha, rnd, tail == 1)
        assert edge >= 2
        above = check_against_exact((coverage - edge, edge, 7, coverage + 9), prm, n_tests)
        below = check_against_exact((coverage - edge + 1, edge - 1, 7, coverage + 9), prm, n_tests)
        assert above["called"] and not below["called"] and above["partial"] == 7
        assert above["p_value"] < prm.alpha <= below["p_value"]


def test_other_counts_against_exact_arithmetic():
    """Away from the edge: nothing observed, the expected count itself, a count below it (two-sided: a deficit), everything deleted."""
    for tail in (0, 1):
        prm = capi.default_params(chemistry="permissive", tail=tail)
        for cov, d in ((600, 0), (600, 2), (5000, 10), (5000, 3), (600, 600), (40, 39), (3000, 3000)):
            got = check_against_exact((cov - d, d, 0, cov), prm, 500.0)
            if d == 0:
                assert not got["called"]                      # nothing observed is never called, whatever the tail says


def test_percent_filters_are_strict():
    n_tests = 10.0
    base = dict(chemistry="sequel")
    cnt = (570, 30, 0, 600)                                   # 100 * 30 / 600 = 5 exactly
    assert check_against_exact(cnt, capi.default_params(**base), n_tests)["called"]
    assert not check_against_exact(cnt, capi.default_params(min_perc=5.0, **base), n_tests)["called"]
    assert check_against_exact(cnt, capi.default_params(min_perc=4.999, **base), n_tests)["called"]
    assert not check_against_exact(cnt, capi.default_params(max_perc=5.0, **base), n_tests)["called"]
    assert check_against_exact(cnt, capi.default_params(max_perc=5.001, **base), n_tests)["called"]
    assert check_against_exact(cnt, capi.default_params(min_perc=0.0, max_perc=100.0, **base), n_tests)["called"]


def test_no_coverage():
    for cnt in ((0, 0, 0, 0), (0, 0, 12, 40)):
        got = capi.deletion_test(cnt, capi.default_params(), 1000.0)
        assert got == dict(count=0, coverage=0, expected=0, partial=cnt[2], called=False, p_value=1.0, log_p=0.0)


def test_bonferroni_factor_is_the_argument():
    """prm.n_tests is not read: the factor comes in resolved."""
    prm = capi.default_params(n_tests=1.0)
    a, b = capi.deletion_test((2960, 40, 0, 3000), prm, 1.0), capi.deletion_test((2960, 40, 0, 3000), prm, 1000.0)
    assert 0 < a["p_value"] < 1e-3 and b["p_value"] == pytest.approx(1000.0 * a["p_value"], rel=1e-15) and a["log_p"] == b["log_p"]


def test_argument_errors():
    lib = capi.load_library()
    cnt = np.array([100, 5, 0, 105], dtype=np.uint32)
    prm, out = capi.default_params(), capi.DeletionCall()

    def refused(word, c=cnt.ctypes.data, p=C.byref(prm), n_tests=100.0, o=C.byref(out)):
        assert lib.jl_deletion_test(c, p, n_tests, o) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)

    refused("NULL", c=None)
    refused("NULL", p=None)
    refused("NULL", o=None)
    refused("n_tests", n_tests=0.0)
    refused("n_tests", n_tests=-3.0)
    refused("n_tests", n_tests=float("nan"))
    for rate in (-1e-9, 1.0000001, float("nan")):
        bad = capi.default_params()
        bad.err.deletion = rate
        refused("outside [0, 1]", p=C.byref(bad))
    refused("32 bits", c=np.array([0xFFFFFFFF, 1, 0, 0], dtype=np.uint32).ctypes.data)
    for rate in (0.0, 1.0):                                    # the ends of the interval are rates
        ok = capi.default_params()
        ok.err.deletion = rate
        got = capi.deletion_test(cnt, ok, 100.0)
        assert got["expected"] == (0 if rate == 0.0 else 105)
    with pytest.raises(capi.JulietError) as e:
        capi.deletion_test(cnt, prm, 0.0)
    assert e.value.status == -1
