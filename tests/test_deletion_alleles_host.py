"""The host-only half of the deletion alleles (docs/SPEC.md §25): the mirror (a per-read scan) against two independent formulations
of the rule, the four identities of §25, the test of one allele (jl_deletion_allele_test) against exact arithmetic at the edge of a
call, the exports, and the refusals of `juliet --call-deletion-alleles`.  No GPU: the library only has to load."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import deletion_alleles_cases as cases
import deletion_alleles_mirror as am
import deletion_mirror as dm
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
A, C_, G, T, GAP, N, OUT = 0, 1, 2, 3, 4, 5, 6
NAMES = ("jl_deletion_alleles_async", "jl_deletion_alleles_fetch", "jl_deletion_allele_test")


# ---------------------------------------------------------------------------------------------- two other formulations of the rule
def by_run_lengths(rows):
    """Run-length encoding per row via np.diff: (runs, open, {(s, len): count})."""
    rows = np.asarray(rows)
    n_cols = rows.shape[1]
    runs, open_, table = [0, 0], np.zeros(n_cols, dtype=np.int64), {}
    for row in rows:
        edge = np.diff(np.concatenate(([0], (row == GAP).astype(np.int8), [0])))
        for s, e in zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()):
            if s >= 1 and e <= n_cols - 1 and row[s - 1] != OUT and row[e] != OUT:
                runs[0] += 1
                table[(s, e - s)] = table.get((s, e - s), 0) + 1
            else:
                runs[1] += 1
                open_[s:e] += 1
    return runs, open_, table


def by_cell_walk(rows):
    """Brute force: every cell of every read, one at a time."""
    n, n_cols = np.asarray(rows).shape
    runs, open_, table = [0, 0], [0] * n_cols, {}
    for i in range(n):
        c = 0
        while c < n_cols:
            if rows[i][c] != GAP:
                c += 1
                continue
            s = c
            while c < n_cols and rows[i][c] == GAP:
                c += 1
            left = s - 1 >= 0 and rows[i][s - 1] != OUT
            right = c <= n_cols - 1 and rows[i][c] != OUT
            if left and right:
                runs[0] += 1
                table[(s, c - s)] = table.get((s, c - s), 0) + 1
            else:
                runs[1] += 1
                for k in range(s, c):
                    open_[k] += 1
    return runs, np.array(open_, dtype=np.int64), table


def flank_by_hand(rows, s, length):
    return sum(1 for row in rows if row[s - 1] != OUT and row[s + length] != OUT)


def agree(rows):
    rows = np.asarray(rows, dtype=np.uint8)
    res = am.alleles(rows)
    for other in (by_run_lengths(rows), by_cell_walk(rows)):
        assert res["runs"].tolist() == list(other[0])
        assert (res["open"] == other[1]).all()
        assert [((int(a["col"]), int(a["len"])), int(a["count"])) for a in res["alleles"]] == sorted(other[2].items())
    for a in res["alleles"]:
        assert int(a["flank"]) == flank_by_hand(rows, int(a["col"]), int(a["len"]))
    return res


def listed(res):
    return [tuple(int(a[k]) for k in ("col", "len", "count", "flank")) for a in res["alleles"]]


def test_mirror_against_two_formulations_on_seeded_matrices():
    rng = np.random.default_rng(25)
    bounded = opened = 0
    for k in range(200):
        n, n_cols = int(rng.integers(1, 12)), int(rng.integers(1, 14))
        p = np.array([3, 3, 3, 3, 8, 1, 3], dtype=np.float64)         # '-' often, so that runs of every length occur
        res = agree(rng.choice(7, size=(n, n_cols), p=p / p.sum()).astype(np.uint8))
        bounded, opened = bounded + int(res["runs"][0]), opened + int(res["runs"][1])
    assert bounded > 200 and opened > 200


def test_mirror_designed_rows():
    assert listed(agree([[GAP, A, C_, G]])) == [] and am.alleles([[GAP, A, C_, G]])["open"].tolist() == [1, 0, 0, 0]      # a run at column 0
    res = agree([[A, C_, GAP, GAP]])                                   # a run ending at n_cols - 1
    assert listed(res) == [] and res["open"].tolist() == [0, 0, 1, 1] and res["runs"].tolist() == [0, 1]
    res = agree([[GAP] * 6])                                           # '-' throughout
    assert listed(res) == [] and res["open"].tolist() == [1] * 6
    assert listed(agree([[A, GAP, GAP, GAP, GAP, T]])) == [(1, 4, 1, 1)]                  # the longest bounded run
    for n_cols in (1, 2):
        res = agree([[GAP] * n_cols, [A] * n_cols])
        assert listed(res) == [] and res["runs"].tolist() == [0, 1]
    assert listed(agree([[A, GAP, T], [GAP, GAP, T], [A, C_, G]])) == [(1, 1, 1, 3)]      # three columns: one possible allele
    assert listed(agree([[N, GAP, GAP, N, A]])) == [(1, 2, 1, 1)]                         # N flanks: bounded
    for row in ([OUT, GAP, GAP, A, A], [A, GAP, GAP, OUT, A]):                            # a code-6 flank on either side: open
        res = agree([row])
        assert listed(res) == [] and res["open"].tolist() == [0, 1, 1, 0, 0]
    assert listed(agree([[A, GAP, GAP, C_, GAP, T]])) == [(1, 2, 1, 1), (4, 1, 1, 1)]    # two runs separated by one base
    assert listed(agree([[A, GAP, GAP, C_, T], [A, GAP, G, C_, T]])) == [(1, 1, 1, 2), (1, 2, 1, 2)]     # same s, different len
    assert listed(agree([[A, GAP, GAP, C_, T], [A, C_, GAP, GAP, T]])) == [(1, 2, 1, 2), (2, 2, 1, 2)]   # same len, different s
    # flank: the reads reaching across the extent, whatever they hold inside it
    assert listed(agree([[A, GAP, GAP, T], [A, C_, G, T], [OUT, C_, G, T], [A, OUT, OUT, T], [N, GAP, GAP, N]])) == [(1, 2, 2, 4)]


def test_the_gpu_cases_are_not_vacuous():
    for n, n_cols in cases.CASES:
        if n * n_cols > 200_000:
            continue                                                   # (the GPU test asserts the same on the large ones)
        rows = cases.make_case(n, n_cols, 1000 * n + n_cols)
        res = am.alleles(rows)
        cases.assert_not_vacuous(rows, res)
        if n * n_cols <= 3000:
            agree(rows)
    for rows, n_alleles in ((cases.distinct_alleles(4096, 130), 4096), (cases.every_allele(2048, 40), 741)):
        assert len(am.alleles(rows)["alleles"]) == n_alleles
    res = am.alleles(cases.one_allele_everywhere(4096, 130))
    assert listed(res)[0] == (5, 9, 4096, 4096) and res["runs"].tolist() == [8192, 0]


def test_identities():
    for n, n_cols, seed in ((1, 1, 1), (3, 2, 2), (40, 3, 3), (33, 9, 4), (300, 40, 5), (1025, 66, 6)):
        rows = cases.make_case(n, n_cols, seed)
        am.check_identities(am.alleles(rows), am.column_gaps(rows), am.column_covered(rows), dm.counts(rows)[:, dm.DEL3] if n_cols >= 3 else None)
    rng = np.random.default_rng(8)
    for k in range(40):
        rows = rng.choice(7, size=(30, 12), p=np.array([3, 3, 3, 3, 8, 1, 2]) / 23.0).astype(np.uint8)
        am.check_identities(am.alleles(rows), am.column_gaps(rows), am.column_covered(rows), dm.counts(rows)[:, dm.DEL3])
    # ... and they can fail: one count off breaks them
    rows = cases.make_case(300, 40, 5)
    res = am.alleles(rows)
    res["alleles"]["count"][0] += 1
    with pytest.raises(AssertionError):
        am.check_identities(res, am.column_gaps(rows), am.column_covered(rows), dm.counts(rows)[:, dm.DEL3])


def test_gene_overlaps():
    genes = [("G", 1, 91), ("H", 12, 72)]                              # H: another frame (12 = 1 + 11)
    assert am.gene_overlaps(31, 9, genes) == [dict(name="G", first_position=11, last_position=13, codon_aligned=True),
                                              dict(name="H", first_position=7, last_position=10, codon_aligned=False)]
    assert am.gene_overlaps(88, 9, genes) == [dict(name="G", first_position=30, last_position=30, codon_aligned=True)]      # clipped
    assert am.gene_overlaps(91, 3, genes) == [] and am.gene_overlaps(32, 1, genes)[0]["codon_aligned"] is False


# ---------------------------------------------------------------------------------------------- jl_deletion_allele_test
def test_exports_abi_and_structs():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header)
    assert lib.jl_abi_version() == 5 and "#define JL_ABI_VERSION 5" in header
    assert capi.DELETION_ALLELE.itemsize == 16 and "} jl_deletion_allele;" in header
    assert C.sizeof(capi.DeletionAlleleCall) == 32


def test_stage_refused_without_a_matrix():
    """With a device: a context without a matrix is a state error, and so is a fetch.  Without one no context exists (the loud
    refusal of test_capi_exports.py), and the entry points refuse the NULL context."""
    lib = capi.load_library()
    if lib.jl_device_count() > 0:
        j = capi.Juliet(0)
        assert lib.jl_deletion_alleles_async(j.h) == -4 and "no resident matrix" in lib.jl_last_error(j.h).decode()
        assert lib.jl_deletion_alleles_fetch(j.h, None, None, None, 0, None) == -4
        j.close()
    else:
        with pytest.raises(capi.JulietError) as e:
            capi.Juliet(0)
        assert e.value.status == -2
        assert lib.jl_deletion_alleles_async(None) == -1 and lib.jl_deletion_alleles_fetch(None, None, None, None, 0, None) == -1


def check_against_exact(count, flank, rate, prm, n_tests):
    got = capi.deletion_allele_test(count, flank, prm, rate, n_tests)
    exp = am.test(count, flank, rate, n_tests, prm.alpha, prm.expected_round, prm.tail == 1, prm.min_perc, prm.max_perc)
    for key in ("count", "coverage", "expected", "called"):
        assert got[key] == exp[key], (key, count, flank, rate, got, exp)
    p_adj, p = float(exp["p_adj"]), float(exp["p"])
    if p_adj > 1e-300:                       # §5's bounds: tests/test_fisher_host.py's tolerances for the same routines
        assert abs(got["p_value"] - p_adj) <= 5e-12 * p_adj, (count, flank, got["p_value"], p_adj)
    if p > 1e-300:
        lp = math.log(p)
        assert abs(got["log_p"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13, (count, flank, got["log_p"], lp)
    return got


ALL_MODES = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]           # (expected_round, tail)
# coverage: (rates, modes).  The exact sums are long integers of 15 000 and 60 000 digits at the two deep coverages, which get three
# combinations each — all modes and both tails again.  Two triples a combination: 12 + 12 + 12 + 12 + 6 = 54 either side of the edge.
EDGE = {64: ((1e-2,), ALL_MODES), 600: ((1e-3,), ALL_MODES), 3000: ((5e-3,), ALL_MODES),
        25000: ((1e-3, 1e-4), [(0, 0), (1, 1), (2, 0)]), 100000: ((1e-3,), [(0, 1), (1, 0), (2, 1)])}


@pytest.mark.parametrize("coverage", sorted(EDGE))
def test_edge_of_a_call_against_exact_arithmetic(coverage):
    """The smallest called count — found by the exact mirror, not by the code under test — and the count below it."""
    n_tests = 40.0 if coverage == 64 else 1090.0
    rates, modes = EDGE[coverage]
    for rate in rates:
        for rnd, tail in modes:
            prm = capi.default_params(expected_round=rnd, tail=tail)
            edge = am.smallest_called(coverage, rate, n_tests, prm.alpha, rnd, tail == 1)
            assert edge >= 2
            above = check_against_exact(edge, coverage, rate, prm, n_tests)
            below = check_against_exact(edge - 1, coverage, rate, prm, n_tests)
            assert above["called"] and not below["called"]
            assert above["p_value"] < prm.alpha <= below["p_value"]


def test_other_counts_against_exact_arithmetic():
    """Away from the edge: nothing observed, the expected count itself, a count below it (two-sided: a deficit), every read."""
    for tail in (0, 1):
        prm = capi.default_params(tail=tail)
        for cov, d in ((600, 0), (600, 2), (5000, 10), (5000, 3), (600, 600), (64, 63), (3000, 3000)):
            got = check_against_exact(d, cov, 2e-3, prm, 500.0)
            if d == 0:
                assert not got["called"]                      # nothing observed is never called, whatever the tail says


def test_percent_filters_are_strict():
    n_tests, rate = 10.0, 1e-3                                # 100 * 30 / 600 = 5 exactly
    assert check_against_exact(30, 600, rate, capi.default_params(), n_tests)["called"]
    assert not check_against_exact(30, 600, rate, capi.default_params(min_perc=5.0), n_tests)["called"]
    assert check_against_exact(30, 600, rate, capi.default_params(min_perc=4.999), n_tests)["called"]
    assert not check_against_exact(30, 600, rate, capi.default_params(max_perc=5.0), n_tests)["called"]
    assert check_against_exact(30, 600, rate, capi.default_params(max_perc=5.001), n_tests)["called"]
    assert check_against_exact(30, 600, rate, capi.default_params(min_perc=0.0, max_perc=100.0), n_tests)["called"]


def test_no_coverage_and_the_factor():
    got = capi.deletion_allele_test(0, 0, capi.default_params(), 1e-3, 1000.0)
    assert got == dict(count=0, coverage=0, expected=0, called=False, p_value=1.0, log_p=0.0)
    prm = capi.default_params(n_tests=1.0)                    # prm.n_tests is not read: the factor comes in resolved
    a, b = capi.deletion_allele_test(40, 3000, prm, 1e-3, 1.0), capi.deletion_allele_test(40, 3000, prm, 1e-3, 1000.0)
    assert 0 < a["p_value"] < 1e-3 and b["p_value"] == pytest.approx(1000.0 * a["p_value"], rel=1e-15) and a["log_p"] == b["log_p"]


def test_argument_errors():
    lib = capi.load_library()
    prm, out = capi.default_params(), capi.DeletionAlleleCall()

    def refused(word, count=5, flank=105, p=C.byref(prm), rate=1e-3, n_tests=100.0, o=C.byref(out)):
        assert lib.jl_deletion_allele_test(count, flank, p, rate, n_tests, o) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)

    refused("NULL", p=None)
    refused("NULL", o=None)
    for bad in (0.0, -3.0, float("nan")):
        refused("n_tests", n_tests=bad)
    for bad in (-1e-9, 1.0000001, float("nan")):
        refused("outside [0, 1]", rate=bad)
    refused("above the flank", count=106)
    for rate in (0.0, 1.0):                                    # the ends of the interval are rates
        assert capi.deletion_allele_test(5, 105, prm, rate, 100.0)["expected"] == (0 if rate == 0.0 else 105)
    assert capi.deletion_allele_test(105, 105, prm, 1e-3, 100.0)["called"]       # count == flank is a table
    with pytest.raises(capi.JulietError) as e:
        capi.deletion_allele_test(5, 105, prm, 1e-3, 0.0)
    assert e.value.status == -1


# ---------------------------------------------------------------------------------------------- the command line's refusals
FLAG = "--call-deletion-alleles"


def juliet(d, *args, prog=JULIET):
    return subprocess.run([prog, *args], cwd=d, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [
    [FLAG, "--windows", "2"], [FLAG, "--devices", "0,0"], [FLAG, "--mode-phasing", "--windows", "3"], [FLAG, "--control", "no_such_control.bam"],
    ["--deletion-allele-rate", "0.001"], ["--min-deletion-length", "3"], [FLAG, "--min-deletion-length", "0"],
    [FLAG, "--deletion-allele-rate", "1.5"], [FLAG, "--deletion-allele-rate", "-0.1"], [FLAG, "--deletion-allele-rate", "x"],
])
def test_cli_refusals_open_nothing(tmp_path, args):
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    r = juliet(tmp_path, *args, "no_such.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert re.search(r"--call-deletion-alleles|--deletion-allele-rate|--min-deletion-length", r.stderr) and "no_such" not in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_and_as_fuse(tmp_path):
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, FLAG, "--batch", "l.tsv")
    assert r.returncode == 1 and FLAG in r.stderr and "--batch" in r.stderr
    r = juliet(tmp_path, FLAG, "no_such.bam", "o.fasta", prog=os.path.join(ROOT, "minorseq_amd", "bin", "fuse"))
    assert r.returncode == 1 and FLAG in r.stderr and "fuse" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]


def test_cli_help_names_the_flag():
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert FLAG in text and "--deletion-allele-rate" in text and "--min-deletion-length" in text
