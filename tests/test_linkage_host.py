"""The host-only half of the pairwise linkage (docs/SPEC.md §15): the mirror itself on matrices small enough to count by hand, the
statistics of a pair's 2 x 2 table (jl_linkage_stats) against the mirror's exact values, the three exports, and what the command
line refuses of --linkage before any file is read.  No GPU: the library only has to load."""
import ctypes as C
import fnmatch
import json
import os
import re
import subprocess

import numpy as np
import pytest

import linkage_mirror
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
FUSE = os.path.join(ROOT, "minorseq_amd", "bin", "fuse")
NAMES = ("jl_variant_linkage_async", "jl_variant_linkage_fetch", "jl_linkage_stats")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(FUSE)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


# ---------------------------------------------------------------------------------------------- the mirror, counted by hand
A, C_, G, T, GAP, N, OUT = 0, 1, 2, 3, 4, 5, 6


def codon(a, b, c):
    return 16 * a + 4 * b + c


def test_mirror_a_read_open_at_one_of_two_positions():
    """Codons at columns 0 and 3.  Read 2 has a gap in the second codon, read 3 an N in the first, read 4 covers neither."""
    rows = np.array([[A, A, A, C_, C_, C_],
                     [A, A, A, C_, C_, C_],
                     [A, A, A, C_, GAP, C_],
                     [N, A, A, C_, C_, C_],
                     [OUT, OUT, OUT, OUT, OUT, OUT],
                     [A, A, G, C_, C_, T]], dtype=np.uint8)
    t = linkage_mirror.linkage(rows, [0, 3], [0, 1], [codon(A, A, A), codon(C_, C_, C_)])
    assert t["both"].tolist() == [[4, 3], [3, 4]]         # informative at 0: reads 0 1 2 5; at 3: reads 0 1 3 5; at both: 0 1 5
    assert t["carry"].tolist() == [[3, 2], [2, 3]]        # AAA: reads 0 1 2, of them 0 1 readable at 3; CCC: reads 0 1 3, of them 0 1 at 0
    assert t["joint"].tolist() == [[3, 2], [2, 3]]
    assert linkage_mirror.pair_table(t, [0, 1], 0, 1) == (3, 2, 0, 0, 1)     # read 5 carries neither


def test_mirror_two_codons_at_one_position():
    """Variants 0 and 1 at position 0 (AAA, AAG), variant 2 at position 1 (CCC)."""
    rows = np.array([[A, A, A, C_, C_, C_],
                     [A, A, G, C_, C_, C_],
                     [A, A, G, C_, C_, T],
                     [A, A, A, GAP, C_, C_],
                     [T, T, T, C_, C_, C_]], dtype=np.uint8)
    var_pos, var_codon = [0, 0, 1], [codon(A, A, A), codon(A, A, G), codon(C_, C_, C_)]
    t = linkage_mirror.linkage(rows, [0, 3], var_pos, var_codon)
    assert t["both"].tolist() == [[5, 4], [4, 4]]
    assert t["carry"].tolist() == [[2, 1], [2, 2], [3, 3]]
    assert t["joint"].tolist() == [[2, 0, 1], [0, 2, 1], [1, 1, 3]]          # two different codons at one position: 0
    assert linkage_mirror.pair_table(t, var_pos, 0, 2) == (4, 1, 0, 2, 1)
    assert linkage_mirror.pair_table(t, var_pos, 1, 2) == (4, 1, 1, 2, 0)


def test_mirror_overlapping_codons_at_columns_0_and_1():
    """Two frames: the codons at columns 0 and 1 share two bases; a gap at column 0 opens the first only, one at column 3 the second only."""
    rows = np.array([[A, C_, G, T],
                     [A, C_, G, T],
                     [GAP, C_, G, T],
                     [A, C_, G, GAP],
                     [A, C_, G, A]], dtype=np.uint8)
    t = linkage_mirror.linkage(rows, [0, 1], [0, 1], [codon(A, C_, G), codon(C_, G, T)])
    assert t["both"].tolist() == [[4, 3], [3, 4]]
    assert t["carry"].tolist() == [[4, 3], [2, 3]]          # CGT: reads 0 1 2, of them 0 1 readable in the first frame
    assert t["joint"].tolist() == [[4, 2], [2, 3]]
    assert linkage_mirror.pair_table(t, [0, 1], 0, 1) == (3, 2, 1, 0, 0)


def test_mirror_statistics_by_hand():
    s = linkage_mirror.stats(2, 1, 1, 2)          # n = 6, margins 3 3 3 3: D_num = 12 - 9 = 3, r2 = 9 / 81, D_max = min(9, 9)
    assert (s["D_num"], s["r2"], s["d_prime"]) == (3, linkage_mirror.Fraction(1, 9), linkage_mirror.Fraction(1, 3))
    assert s["p_positive"] == linkage_mirror.Fraction(10, 20) and s["p_negative"] == linkage_mirror.Fraction(19, 20)   # C(3,x) C(3,3-x) = 1 9 9 1


# ---------------------------------------------------------------------------------------------- jl_linkage_stats
def tables_of(n11, n10, n01, n00):
    """Count tables of two positions with one variant each whose pair has this 2 x 2 table (what lies on the diagonals is not read)."""
    n = n11 + n10 + n01 + n00
    both = np.array([[n, n], [n, n]], dtype=np.uint32)
    carry = np.array([[n11 + n10, n11 + n10], [n11 + n01, n11 + n01]], dtype=np.uint32)
    joint = np.array([[n11 + n10, n11], [n11, n11 + n01]], dtype=np.uint32)
    return both, carry, joint


def close(got, exact, rel):
    exact = float(exact)
    return got == exact if exact == 0.0 else abs(got - exact) <= rel * abs(exact)


def check_table(n11, n10, n01, n00, p_values=True):
    exp = linkage_mirror.stats(n11, n10, n01, n00, p_values)
    for v, w in ((0, 1), (1, 0)):          # the pair in both orders: n10 and n01 change places, nothing else does
        got = capi.linkage_stats(*tables_of(n11, n10, n01, n00), [0, 1], v, w)
        t = (n11, n10, n01, n00) if v == 0 else (n11, n01, n10, n00)
        assert (got["n"], got["n11"], got["n10"], got["n01"], got["n00"]) == (sum(t), *t)
        # D_num is exact, the rest at most ten double roundings (< 2e-15): two orders over that
        assert close(got["r2"], exp["r2"], 1e-13), (t, got["r2"], float(exp["r2"]))
        assert close(got["d_prime"], exp["d_prime"], 1e-13), (t, got["d_prime"], float(exp["d_prime"]))
        if p_values:                        # the project's p-value tolerance (DESIGN.md "Numerics")
            assert abs(got["p_positive"] - float(exp["p_positive"])) <= 1e-10, (t, got["p_positive"], float(exp["p_positive"]))
            assert abs(got["p_negative"] - float(exp["p_negative"])) <= 1e-10, (t, got["p_negative"], float(exp["p_negative"]))
    return exp


@pytest.mark.parametrize("table", [
    (40, 0, 0, 60), (1, 0, 0, 1), (700, 0, 0, 2300),                    # perfect linkage
    (0, 40, 60, 0), (0, 1, 1, 0), (0, 30, 50, 20),                      # perfect exclusion; n11 = 0
    (0, 5, 7, 1000), (0, 1, 1, 1),                                      # n11 = 0
    (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),             # n = 1
    (0, 0, 12, 30), (12, 30, 0, 0), (0, 12, 0, 30), (12, 0, 30, 0),     # a zero margin in each of the four places
    (0, 0, 0, 0),                                                       # ... and nobody readable at both
    (3, 9, 7, 21), (10, 10, 10, 10), (1, 1, 1, 1), (20, 30, 200, 300),  # independence
    (2, 1, 1, 2), (25, 3, 4, 2968), (1500, 2, 3, 1495), (29, 0, 1, 2499), (5, 200, 150, 2000),
])
def test_linkage_stats_on_the_edges(table):
    exp = check_table(*table)
    n11, n10, n01, n00 = table
    if (n10, n01) == (0, 0) and n11 and n00:
        assert exp["r2"] == 1 and exp["d_prime"] == 1
    if (n11, n00) == (0, 0) and n10 and n01:
        assert exp["r2"] == 1 and exp["d_prime"] == -1
    if table in ((3, 9, 7, 21), (10, 10, 10, 10), (1, 1, 1, 1), (20, 30, 200, 300)):
        assert exp["D_num"] == 0                                        # exactly
        got = capi.linkage_stats(*tables_of(*table), [0, 1], 0, 1)
        assert got["r2"] == 0.0 and got["d_prime"] == 0.0
    if 0 in (n11 + n10, n01 + n00, n11 + n01, n10 + n00):
        got = capi.linkage_stats(*tables_of(*table), [0, 1], 0, 1)
        assert (got["r2"], got["d_prime"], got["p_positive"], got["p_negative"]) == (0.0, 0.0, 1.0, 1.0)


@pytest.mark.parametrize("table", [
    (2**32 - 1, 0, 0, 0), (2**31, 0, 0, 2**31 - 1), (0, 2**31, 2**31 - 1, 0), (2**30, 2**30, 2**30, 2**30 - 1),
    (2**30 + 12345, 2**30 - 54321, 2**30 + 7, 2**30 - 1 - 12345 + 54321 - 7), (3, 2**31, 2**31 - 10, 6), (2**32 - 4, 1, 1, 1),
    (1, 1, 1, 2**32 - 4), (123456789, 987654321, 1111111111, 2**32 - 1 - 123456789 - 987654321 - 1111111111),
])
def test_linkage_stats_keeps_d_num_exact_near_the_top_of_32_bits(table):
    """The products of D_num pass 2**64 / 4 here: r2 and d_prime only (the exact tails of such tables are out of reach)."""
    assert sum(table) == 2**32 - 1 and min(table) >= 0
    check_table(*table, p_values=False)


def test_linkage_stats_on_seeded_tables():
    """About 200 tables with n <= 3000: half of them drawn freely, half with the two variants strongly linked or exclusive."""
    rng = np.random.default_rng(15)
    for k in range(200):
        n = int(rng.integers(1, 3001))
        if k % 2:
            cuts = np.sort(rng.integers(0, n + 1, size=3))
            t = (int(cuts[0]), int(cuts[1] - cuts[0]), int(cuts[2] - cuts[1]), int(n - cuts[2]))
        else:
            minor, noise = int(rng.integers(0, n // 2 + 1)), rng.integers(0, 4, size=2)
            t = (minor, int(noise[0]), int(noise[1]), max(0, n - minor - int(noise.sum())))
            if k % 4 == 0:
                t = (t[1], t[0], t[3], t[2])
        check_table(*t)


# ---------------------------------------------------------------------------------------------- the tails over the whole domain
P_ABS_TOL, P_REL_TOL = 1e-10, 5e-12     # the project's p-value bounds (DESIGN.md "Numerics"; test_control_host.py)


@pytest.fixture(scope="module")
def tails():
    with open(os.path.join(ROOT, "tests", "golden", "linkage_tails.json")) as f:
        return json.load(f)["tables"]


def test_tail_fixture_is_the_design(tails):
    got = [(t["n11"], t["n10"], t["n01"], t["n00"]) for t in tails]
    assert got == linkage_mirror.tail_design() and len(set(got)) == len(got) and 300 < len(got) <= linkage_mirror.MAX_TAIL_TABLES
    assert {sum(t) for t in got} == set(linkage_mirror.TAIL_READS)
    for n in (10 ** 5, 10 ** 7, 2 * 10 ** 9):
        mine = [t for t in got if sum(t) == n]
        assert sum(1 for t in mine if t[1] == t[2] == 0) >= 3 and sum(1 for t in mine if t[0] == 0 and t[3] == 0) >= 3   # perfect
        assert sum(1 for t in mine if 0 < t[1] + t[2] <= 3 and t[0] >= 9) >= 3 and sum(1 for t in mine if t[0] == 1) >= 3      # nearly
        for row1, col1 in linkage_mirror.tail_margins(n):
            lo, hi, mean = max(0, row1 + col1 - n), min(row1, col1), row1 * col1 // n
            xs = {t[0] for t in mine if (t[0] + t[1], t[0] + t[2]) == (row1, col1)}
            assert {lo, lo + 1, hi, max(lo, mean - 1), min(hi, mean + 1)} <= xs, (n, row1, col1)
    for side in ("p_positive", "p_negative"):        # p from about 1/2 down to below the doubles, at every depth from 1e5
        for n in (10 ** 5, 10 ** 7, 2 * 10 ** 9, 2 ** 31 - 1):
            ps = [float(t[side]) for t in tails if t["n11"] + t["n10"] + t["n01"] + t["n00"] == n]
            for lo_, hi_ in ((0.3, 0.7), (1e-12, 1e-2), (1e-120, 1e-30), (1e-300, 1e-150), (0.0, 0.0)):
                assert any(lo_ <= v <= hi_ for v in ps), (side, n, lo_, hi_)


def test_linkage_tails_over_the_whole_domain(tails):
    """p_positive and p_negative against exact arithmetic for n = 1 .. 2^31 - 1: absolute 1e-10, relative 5e-12 where the exact
    value is above 1e-300, exactly 0 where it is below 2^-1075 (float() of the exact digits is then 0).  Measured: worst relative
    error 2.9e-13 (the saddle-point routine this entry had before missed the bound from 10^7 reads on: 1.2e-12 there, 1.9e-11 at
    2 10^9 within 12 sigma of the mean)."""
    worst = (0.0, (), "")
    for t in tails:
        cells = (t["n11"], t["n10"], t["n01"], t["n00"])
        got = capi.linkage_stats(*tables_of(*cells), [0, 1], 0, 1)
        assert (got["n11"], got["n10"], got["n01"], got["n00"]) == cells
        for side in ("p_positive", "p_negative"):
            exact, p = float(t[side]), got[side]
            assert abs(p - exact) <= P_ABS_TOL, (cells, side, p, exact)
            if exact == 0.0:
                assert p == 0.0, (cells, side, p)
            elif exact > 1e-300:
                assert abs(p - exact) <= P_REL_TOL * exact, (cells, side, p, exact, abs(p - exact) / exact)
                worst = max(worst, (abs(p - exact) / exact, cells, side))
    print("%d tables, worst relative error %.3g at %s (%s)" % (len(tails), *worst))


def test_linkage_stats_refusals():
    lib = capi.load_library()
    both, carry, joint = tables_of(2, 1, 1, 2)
    var_pos = np.array([0, 1], dtype=np.uint32)
    same = np.array([0, 0], dtype=np.uint32)
    out = capi.LinkPair()

    def refused(word, both=both, carry=carry, joint=joint, var_pos=var_pos, v=0, w=1, out=out):
        p = [None if a is None else a.ctypes.data for a in (both, carry, joint, var_pos)]
        assert lib.jl_linkage_stats(*p, 2, 2, v, w, None if out is None else C.byref(out)) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)

    refused("NULL", both=None)
    refused("NULL", carry=None)
    refused("NULL", joint=None)
    refused("NULL", var_pos=None)
    refused("NULL", out=None)
    refused("variants 2 and 1", v=2)
    refused("variants 0 and 2", w=2)
    refused("one position", var_pos=same)
    refused("one position", v=1, w=1)
    with pytest.raises(capi.JulietError) as e:
        capi.linkage_stats(both, carry, joint, same, 0, 1)
    assert e.value.status == -1 and "one position" in str(e.value)
    assert C.sizeof(capi.LinkPair) == 56


# ---------------------------------------------------------------------------------------------- exports
def test_the_three_symbols_are_declared_exported_and_mirrored():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "juliet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "minorseq_amd", "csrc", "exports.map")).read())
    symbols = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name            # declared in the header
        assert any(fnmatch.fnmatch(name, pat.strip()) for pat in patterns), name      # let through by the export script
        assert name in symbols and hasattr(lib, name)                      # in the library's dynamic symbol table
        assert name in capi.EXPORTS                                        # listed by the ctypes mirror
    assert "JL_LINK_MAX = 1024" in code and capi.LINK_MAX == 1024
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "variant_linkage") and hasattr(capi.Juliet, "variant_linkage_fetch") and callable(capi.linkage_stats)


# ---------------------------------------------------------------------------------------------- the command line
def run(exe, cwd, *args):
    return subprocess.run([exe, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, words", [
    (["--linkage", "--windows", "2"], ["--linkage", "--windows"]),
    (["--mode-phasing", "--linkage", "--windows", "2"], ["--linkage", "--windows"]),
    (["--linkage", "--devices", "0,0"], ["--linkage", "--devices"]),
    (["--mode-phasing", "--linkage", "--devices", "0,0", "--windows", "2"], ["--linkage", "--devices"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAM need not exist."""
    r = run(JULIET, tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_linkage_is_refused_with_batch(tmp_path):
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = run(JULIET, tmp_path, "--linkage", "--batch", "l.tsv")
    assert r.returncode == 1 and "--linkage" in r.stderr and "--batch" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]


def test_linkage_is_refused_as_fuse(tmp_path):
    r = run(FUSE, tmp_path, "--linkage", "a.bam", "o.fasta")
    assert r.returncode == 1 and "--linkage" in r.stderr and "fuse" in r.stderr
    assert not list(tmp_path.iterdir())


def test_help_names_the_flag_and_the_limit():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--linkage" in r.stderr and "1024" in r.stderr and "not Bonferroni-corrected" in r.stderr
