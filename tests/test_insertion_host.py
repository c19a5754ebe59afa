"""The host-only half of the insertion calls (docs/SPEC.md §17): the mirror itself on reads written out by hand, the test of one
allele (jl_insertion_test) against the mirror's exact arithmetic at the edge of a call, and what `juliet` refuses together with
--call-insertions.  No GPU: the library only has to load."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import insertion_mirror as im
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
NAMES = ("jl_msa_track_insertion_alleles", "jl_insertion_alleles_fetch", "jl_insertion_test")


def b(n):
    return "ACGT" * (n // 4) + "ACGT"[:n % 4]


# a window of eight columns from reference position 0
HAND_READS = [
    (0, [("I", 3), ("=", 8)], "TTT" + b(8)),                                     # before the first reference op
    (0, [("=", 8), ("I", 3)], b(8) + "TTT"),                                     # after the last
    (0, [("S", 2), ("I", 3), ("=", 8), ("I", 3), ("S", 1)], "GG" + "TTT" + b(8) + "TTT" + "G"),
    (0, [("=", 3), ("I", 3), ("N", 2), ("=", 3)], b(3) + "TTT" + b(3)),           # beside an N, on either side
    (0, [("=", 3), ("N", 2), ("I", 3), ("=", 3)], b(3) + "TTT" + b(3)),
    (0, [("=", 3), ("I", 3), ("D", 2), ("=", 3)], b(3) + "CCC" + b(3)),           # beside a D: spans, junction 3
    (0, [("=", 3), ("D", 2), ("I", 3), ("=", 3)], b(3) + "CCC" + b(3)),           # ... junction 5
    (0, [("D", 2), ("I", 3), ("D", 2)], "GGG"),                                  # between two deletions: junction 2
    (0, [("=", 2), ("I", 1), ("P", 1), ("I", 2), ("=", 6)], b(2) + "A" + "CG" + b(6)),       # I P I: ACG at junction 2
    (0, [("=", 2), ("I", 2), ("I", 2), ("=", 6)], b(2) + "AC" + "GT" + b(6)),                # I I: four bases, out of frame
    (0, [("=", 2), ("I", 3), ("H", 0), ("S", 0), ("I", 3), ("=", 6)], b(2) + "ACG" + "ACG" + b(6)),   # empty ops between: ACGACG
    (0, [("=", 2), ("I", 0), ("=", 6)], b(8)),                                   # an empty insertion is none
    (0, [("=", 7), ("I", 3), ("=", 1)], b(7) + "AAA" + b(1)),                     # junction n_cols - 1 = 7: counts
    (0, [("=", 8), ("I", 3), ("=", 1)], b(8) + "AAA" + b(1)),                     # junction n_cols = 8: nowhere
    (0, [("=", 9), ("I", 3), ("=", 1)], b(9) + "AAA" + b(1)),                     # beyond
    (0, [("=", 4), ("I", 3), ("=", 4)], b(4) + "AAA" + b(4)),                     # AAA and AAAAAA: one seq word, two rows
    (0, [("=", 4), ("I", 6), ("=", 4)], b(4) + "AAAAAA" + b(4)),
    (0, [("=", 4), ("I", 3), ("=", 4)], b(4) + "ANA" + b(4)),                     # unreadable: N, an ambiguity code, '='
    (0, [("=", 4), ("I", 3), ("=", 4)], b(4) + "RAA" + b(4)),
    (0, [("=", 4), ("I", 3), ("=", 4)], b(4) + "AA=" + b(4)),
    (0, [("=", 4), ("I", 33), ("=", 4)], b(4) + "A" * 33 + b(4)),                 # in frame, too long
    (0, [("=", 4), ("I", 30), ("=", 4)], b(4) + "ACGT" * 7 + "AC" + b(4)),        # two 30-base keys that differ in their last base
    (0, [("=", 4), ("I", 30), ("=", 4)], b(4) + "ACGT" * 7 + "AG" + b(4)),
    (0, [("=", 5), ("I", 30), ("=", 3)], b(5) + "ACGT" * 7 + "AG" + b(3)),        # ... and one that differs in its junction only
    (0, [("=", 4), ("I", 29), ("=", 4)], b(4) + "A" * 29 + b(4)),
    (0, [("=", 4), ("I", 31), ("=", 4)], b(4) + "A" * 31 + b(4)),
]
HAND_ALLELES = [(2, 3, "ACG", 1), (2, 3, "GGG", 1), (2, 6, "ACGACG", 1), (3, 3, "CCC", 1), (4, 3, "AAA", 1), (4, 6, "AAAAAA", 1),
                (4, 30, "ACGT" * 7 + "AC", 1), (4, 30, "ACGT" * 7 + "AG", 1), (5, 3, "CCC", 1), (5, 30, "ACGT" * 7 + "AG", 1), (7, 3, "AAA", 1)]
HAND_FRAMESHIFT = [0, 0, 1, 0, 2, 0, 0, 0]
HAND_UNREAD = [0, 0, 0, 0, 4, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
def named(alleles):
    return [(c, l, im.seq_of(s, l), n) for c, l, s, n in alleles]


def test_mirror_hand_written_reads():
    jcnt, alleles = im.walk(im.records(HAND_READS), 8)
    assert named(alleles) == HAND_ALLELES
    assert jcnt[:, im.FRAMESHIFT].tolist() == HAND_FRAMESHIFT and jcnt[:, im.UNREAD].tolist() == HAND_UNREAD
    assert jcnt[:, im.INFRAME].tolist() == [0, 0, 3, 1, 4, 2, 0, 1] and not jcnt[0].any()
    n = len(HAND_READS)
    # the read of two deletions covers columns 0..3 only; the reads with an N run do not span the junctions inside or beside it
    assert jcnt[:, im.SPAN].tolist() == [0, n, n, n - 2, n - 3, n - 3, n - 1, n - 1]


def test_mirror_seq_word():
    """Base j in bits 2 j, 2 j + 1; AAA and AAAAAA are the same word and two rows."""
    _, alleles = im.walk(im.records([(0, [("=", 2), ("I", 3), ("=", 2)], "AC" + "CGT" + "GT"), (0, [("=", 2), ("I", 3), ("=", 2)], "ACAAAGT"),
                                     (0, [("=", 2), ("I", 6), ("=", 2)], "ACAAAAAAGT")]), 4)
    assert alleles == [(2, 3, 0, 1), (2, 3, 1 | 2 << 2 | 3 << 4, 1), (2, 6, 0, 1)]


def test_mirror_filter_forms():
    """A quality below min_qv on one inserted base makes the read unread; 0xFF never does; the mask form reads its bit, whatever
    the qualities say; min_qv 0 switches either form off."""
    reads = [(0, [("=", 2), ("I", 3), ("=", 2)], "ACGGGGT", [40, 40, 40, 19, 40, 40, 40]),
             (0, [("=", 2), ("I", 3), ("=", 2)], "ACGGGGT", [40, 40, 20, 0xFF, 93, 40, 40]),
             (0, [("=", 2), ("I", 3), ("=", 2)], "ACGGGGT", [0, 0, 40, 40, 40, 0, 0])]
    rec = im.records(reads, with_qual=True)
    assert im.walk(rec, 4, 0, 0)[0][2].tolist() == [3, 3, 0, 0]
    assert im.walk(rec, 4, 0, 20)[0][2].tolist() == [3, 2, 0, 1]
    assert im.walk(rec, 4, 0, 200)[0][2].tolist() == [3, 0, 0, 3]            # taken as 127: 0xFF still passes, 93 does not
    mask = capi.qmask_from_quals(rec["seq_off"], rec["qual"], rec["qual_off"], 20)
    assert im.walk(rec, 4, 0, 20, mask)[0][2].tolist() == [3, 2, 0, 1] and im.walk(rec, 4, 0, 0, mask)[0][2].tolist() == [3, 3, 0, 0]
    none = im.records(reads)
    assert im.walk(none, 4, 0, 20)[0][2].tolist() == [3, 3, 0, 0]            # no qualities, no mask: no filter


def test_mirror_window_offset():
    jcnt, alleles = im.walk(im.records(HAND_READS), 4, 4)
    assert [(c, l) for c, l, _, _ in alleles] == [(1, 3), (1, 30), (3, 3)] and not jcnt[0].any()
    jcnt, alleles = im.walk(im.records(HAND_READS), 1, 4)
    assert jcnt.tolist() == [[0, 0, 0, 0]] and alleles == []


# ---------------------------------------------------------------------------------------------- jl_insertion_test
def test_exports_and_struct():
    lib = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert C.sizeof(capi.InsertionCall) == 40 and capi.INSERTION_ALLELE.itemsize == 24


def check_against_exact(count, jcnt, prm, rate, n_tests):
    got = capi.insertion_test(count, jcnt, prm, rate, n_tests)
    exp = im.test(count, jcnt, rate, n_tests, prm.alpha, prm.expected_round, prm.tail == 1, prm.min_perc, prm.max_perc)
    for key in ("count", "coverage", "expected", "frameshift", "unread", "called"):
        assert got[key] == exp[key], (key, count, jcnt, got, exp)
    p_adj, p = float(exp["p_adj"]), float(exp["p"])
    if p_adj > 1e-300:                       # tests/test_fisher_host.py's tolerances for the same routines
        assert abs(got["p_value"] - p_adj) <= 5e-12 * p_adj, (count, jcnt, got["p_value"], p_adj)
    if p > 1e-300:
        lp = math.log(p)
        assert abs(got["log_p"] - lp) <= 1e-12 * max(1.0, abs(lp)) + 1e-13, (count, jcnt, got["log_p"], lp)
    return got


MODES = {10: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)], 600: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)],
         3000: [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)], 25000: [(0, 0), (1, 1), (2, 0)]}


@pytest.mark.parametrize("coverage", [10, 600, 3000, 25000])
@pytest.mark.parametrize("rate", [1.0e-3, 4.0e-3])
def test_edge_of_a_call_against_exact_arithmetic(coverage, rate):
    """The smallest called count — found by the exact mirror, not by the code under test — and the count below it; seven
    frame-shifting and two unread reads stay out of the coverage."""
    n_tests = 4.0 if coverage == 10 else 1090.0               # (ten reads cannot reach 0.01 / 1090)
    for rnd, tail in MODES[coverage]:
        prm = capi.default_params(expected_round=rnd, tail=tail)
        edge = im.smallest_called(coverage, rate, n_tests, prm.alpha, rnd, tail == 1)
        assert edge >= 2
        above = check_against_exact(edge, (coverage + 9, edge + 3, 7, 2), prm, rate, n_tests)
        below = check_against_exact(edge - 1, (coverage + 9, edge + 3, 7, 2), prm, rate, n_tests)
        assert above["called"] and not below["called"] and above["frameshift"] == 7 and above["unread"] == 2 and above["coverage"] == coverage
        assert above["p_value"] < prm.alpha <= below["p_value"]


def test_other_counts_against_exact_arithmetic():
    """Away from the edge: nothing observed, the expected count itself, a count below it (two-sided: a deficit), every read."""
    for tail in (0, 1):
        prm = capi.default_params(tail=tail)
        for cov, d in ((600, 0), (600, 3), (5000, 20), (5000, 3), (600, 600), (40, 39), (3000, 3000)):
            got = check_against_exact(d, (cov, d, 0, 0), prm, 4.0e-3, 500.0)
            if d == 0:
                assert not got["called"]                      # nothing observed is never called, whatever the tail says


def test_percent_filters_are_strict():
    n_tests, rate = 10.0, 1.0e-3
    jcnt = (600, 30, 0, 0)                                    # 100 * 30 / 600 = 5 exactly
    assert check_against_exact(30, jcnt, capi.default_params(), rate, n_tests)["called"]
    assert not check_against_exact(30, jcnt, capi.default_params(min_perc=5.0), rate, n_tests)["called"]
    assert check_against_exact(30, jcnt, capi.default_params(min_perc=4.999), rate, n_tests)["called"]
    assert not check_against_exact(30, jcnt, capi.default_params(max_perc=5.0), rate, n_tests)["called"]
    assert check_against_exact(30, jcnt, capi.default_params(max_perc=5.001), rate, n_tests)["called"]
    assert check_against_exact(30, jcnt, capi.default_params(min_perc=0.0, max_perc=100.0), rate, n_tests)["called"]


def test_no_coverage_and_no_count():
    for jcnt in ((0, 0, 0, 0), (40, 0, 28, 12)):
        got = capi.insertion_test(0, jcnt, capi.default_params(), 1.0e-3, 1000.0)
        assert got == dict(count=0, coverage=0, expected=0, frameshift=jcnt[2], unread=jcnt[3], called=False, p_value=1.0, log_p=0.0)
    got = check_against_exact(0, (3000, 0, 0, 0), capi.default_params(), 0.0, 1.0)
    assert not got["called"] and got["expected"] == 0 and got["p_value"] == 1.0


def test_rate_and_factor_are_the_arguments():
    """prm.err.deletion and prm.n_tests are not read: both come in as arguments."""
    prm = capi.default_params(n_tests=1.0)
    jcnt = (3000, 40, 0, 0)
    a, b_ = capi.insertion_test(40, jcnt, prm, 1.0e-3, 1.0), capi.insertion_test(40, jcnt, prm, 1.0e-3, 1000.0)
    assert 0 < a["p_value"] < 1e-3 and b_["p_value"] == pytest.approx(1000.0 * a["p_value"], rel=1e-15) and a["log_p"] == b_["log_p"]
    prm.err.deletion = 0.5
    assert capi.insertion_test(40, jcnt, prm, 1.0e-3, 1.0) == a
    assert capi.insertion_test(40, jcnt, prm, 1.0e-2, 1.0)["expected"] == 30


def test_argument_errors():
    lib = capi.load_library()
    jcnt = np.array([105, 5, 0, 0], dtype=np.uint32)
    prm, out = capi.default_params(), capi.InsertionCall()

    def refused(word, count=5, c=jcnt.ctypes.data, p=C.byref(prm), rate=1.0e-3, n_tests=100.0, o=C.byref(out)):
        assert lib.jl_insertion_test(count, c, p, rate, n_tests, o) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)

    refused("NULL", c=None)
    refused("NULL", p=None)
    refused("NULL", o=None)
    refused("n_tests", n_tests=0.0)
    refused("n_tests", n_tests=-3.0)
    refused("n_tests", n_tests=float("nan"))
    for rate in (-1e-9, 1.0000001, float("nan")):
        refused("outside [0, 1]", rate=rate)
    refused("spanning", c=np.array([10, 1, 6, 5], dtype=np.uint32).ctypes.data)
    refused("above the coverage", count=106)
    for rate in (0.0, 1.0):                                    # the ends of the interval are rates
        assert capi.insertion_test(5, jcnt, prm, rate, 100.0)["expected"] == (0 if rate == 0.0 else 105)
    with pytest.raises(capi.JulietError) as e:
        capi.insertion_test(5, jcnt, prm, 1.0e-3, 0.0)
    assert e.value.status == -1


# ---------------------------------------------------------------------------------------------- what the front end refuses
def juliet(d, *args, exe=JULIET):
    return subprocess.run([exe, *args], cwd=d, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [["--windows", "2"], ["--devices", "0,0"], ["--mode-phasing", "--windows", "3"], ["--downsample", "100"],
                                  ["--mix", "a.bam:1"]])
def test_cli_refused_combinations_open_nothing(tmp_path, args):
    r = juliet(tmp_path, "--call-insertions", *args, "no_such.bam", "o.json")
    assert r.returncode == 1 and "--call-insertions" in r.stderr, (r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_refused_with_batch_as_fuse_and_the_rate_alone(tmp_path):
    (tmp_path / "l.tsv").write_text("no_such.bam\ta.json\n")
    r = juliet(tmp_path, "--call-insertions", "--batch", "l.tsv")
    assert r.returncode == 1 and "--call-insertions" in r.stderr and "--batch" in r.stderr
    r = juliet(tmp_path, "--call-insertions", "no_such.bam", "o.fasta", exe=os.path.join(ROOT, "minorseq_amd", "bin", "fuse"))
    assert r.returncode == 1 and "--call-insertions" in r.stderr and "fuse" in r.stderr
    r = juliet(tmp_path, "--insertion-rate", "0.001", "no_such.bam", "o.json")
    assert r.returncode == 1 and "--insertion-rate" in r.stderr and "--call-insertions" in r.stderr
    for bad in ("-0.1", "1.5", "x"):
        r = juliet(tmp_path, "--call-insertions", "--insertion-rate", bad, "no_such.bam", "o.json")
        assert r.returncode == 1 and "--insertion-rate" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]


def test_covered_pairs_from_the_cigars_are_the_matrix_own():
    """records_expand.covered_pairs — what the deep span case of tests/test_gpu_insertions.py expects — against SPAN as the mirror
    states it on the expanded matrix: generated reads with every kind of op (N beside an insertion, D, clips, reads that begin
    before the window and end behind it), windows that begin inside the reads."""
    import records_expand
    from test_gpu_insertions import WB, make_reads
    for n, n_cols, wb in ((300, 40, WB), (257, 130, WB), (64, 2, WB), (500, 25, WB + 9), (33, 64, WB - 2)):
        rec = im.records(make_reads(n, max(n_cols, 5), 7 * n + n_cols), with_qual=True)
        m = records_expand.expand_reference(rec, n_cols, wb, 0)
        exp = np.zeros(n_cols, dtype=np.int64)
        exp[1:] = ((m[:, :-1] != 6) & (m[:, 1:] != 6)).sum(axis=0)
        assert (records_expand.covered_pairs(rec, n_cols, wb) == exp).all(), (n, n_cols, wb)
        assert exp.any() == (n_cols > 1) and (n_cols < 5 or len(set(exp[1:].tolist())) > 1)
