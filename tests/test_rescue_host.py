"""The host-only half of the rescue of damaged reads (docs/SPEC.md §14): the rule's mirror (tests/rescue_mirror.py) on hand-written
rows with the expected ids spelled out, the two exports, and what the command line refuses of --rescue-damaged before any file is
read.  No GPU: the library only has to load."""
import os
import subprocess

import numpy as np
import pytest

import rescue_mirror
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
FUSE = os.path.join(ROOT, "minorseq_amd", "bin", "fuse")

U, NONE, AMB = 0xFFFB, 0xFFFC, 0xFFFD
A, C_, G, T, GAP, N, OUT = range(7)


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(FUSE)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def codon(a, b, c):
    return 16 * a + 4 * b + c


def mirror(rows, pos_cols, pattern, min_positions=1):
    res, hap_reads, tally = rescue_mirror.rescue(np.array(rows, dtype=np.uint8), pos_cols, np.array(pattern, dtype=np.uint8), min_positions)
    assert int(tally.sum()) == len(rows)
    assert hap_reads.tolist() == [int((res == h).sum()) for h in range(len(pattern))]
    assert tally.tolist() == [int((res < len(pattern)).sum()), int((res == AMB).sum()), int((res == NONE).sum()), int((res == U).sum())]
    return res.tolist()


def test_the_constants():
    assert (rescue_mirror.UNINFORMATIVE, rescue_mirror.NONE, rescue_mirror.AMBIGUOUS) == (0xFFFB, 0xFFFC, 0xFFFD)
    assert (capi.RESCUE_UNINFORMATIVE, capi.RESCUE_NONE, capi.RESCUE_AMBIGUOUS) == (0xFFFB, 0xFFFC, 0xFFFD)
    assert len({capi.RESCUE_UNINFORMATIVE, capi.RESCUE_NONE, capi.RESCUE_AMBIGUOUS, capi.HAP_INSUFFICIENT, capi.HAP_DAMAGED}) == 5


def test_open_informative_and_the_four_answers():
    """Two positions (columns 0 and 3) and two haplotypes that differ only at the second."""
    pos = [0, 3]
    pat = [[codon(A, C_, G), codon(T, T, T)], [codon(A, C_, G), codon(T, T, A)]]
    rows = [
        [A, C_, G, T, T, T],          # clean, haplotype 0
        [A, C_, G, T, T, A],          # clean, haplotype 1
        [A, C_, G, T, GAP, T],        # the position where they differ is open (one deleted base opens the whole codon): both agree
        [A, C_, G, T, T, N],          # ... an N does the same
        [A, C_, G, OUT, OUT, OUT],    # ... and so does an uncovered cell
        [GAP, C_, G, T, T, A],        # the first position open: the second decides, haplotype 1
        [A, C_, T, N, T, A],          # a mismatch at the only informative position: none
        [A, C_, T, T, T, T],          # a mismatch at the first position, a match with haplotype 0 at the second: none
        [OUT, OUT, N, GAP, A, A],     # all open: uninformative
        [OUT] * 6,                    # code 6 throughout: uninformative
    ]
    assert mirror(rows, pos, pat) == [0, 1, AMB, AMB, AMB, 1, NONE, NONE, U, U]


def test_min_positions_at_and_above_k():
    pos = [0, 3, 6]
    pat = [[codon(A, A, A), codon(C_, C_, C_), codon(G, G, G)], [codon(A, A, A), codon(C_, C_, C_), codon(T, T, T)]]
    rows = [
        [A, A, A, C_, C_, C_, G, G, G],       # k = 3
        [A, A, A, C_, C_, C_, G, N, G],       # k = 2, both agree
        [A, A, A, GAP, C_, C_, T, T, T],      # k = 2, haplotype 1
        [N, A, A, GAP, C_, C_, T, T, T],      # k = 1, haplotype 1
        [N, A, A, GAP, C_, C_, T, T, C_],     # k = 1, none
        [N, A, A, GAP, C_, C_, T, T, OUT],    # k = 0
    ]
    assert mirror(rows, pos, pat, 1) == [0, AMB, 1, 1, NONE, U]
    assert mirror(rows, pos, pat, 2) == [0, AMB, 1, U, U, U]         # min_positions equal to k_i of rows 1, 2: still judged
    assert mirror(rows, pos, pat, 3) == [0, U, U, U, U, U]           # ... and one above it: uninformative, whatever agrees


def test_duplicate_pattern_rows_are_ambiguous():
    pos = [1]
    pat = [[codon(G, A, T)], [codon(G, A, C_)], [codon(G, A, T)]]
    rows = [[T, G, A, T], [T, G, A, C_], [T, G, A, A], [T, G, GAP, T]]
    assert mirror(rows, pos, pat) == [AMB, 1, NONE, U]
    assert mirror(rows, pos, pat[:2]) == [0, 1, NONE, U]


def test_overlapping_codons_and_the_window_edges():
    """Codons at columns 0 and 1 (two frames) and at n_cols - 3 = 2 of a 5-column window: position 0 at column 0, the last at
    n_cols - 3."""
    pos = [0, 1, 2]
    hap0, hap1 = [A, C_, G, T, A], [A, C_, G, T, C_]
    pat = [[codon(*h[c:c + 3]) for c in pos] for h in (hap0, hap1)]
    assert pat == [[6, 27, 44], [6, 27, 45]]
    rows = [
        hap0, hap1,
        [A, C_, G, T, GAP],           # only the codon at column 0 and the one at column 1 are informative: both agree
        [GAP, C_, G, T, C_],          # the codon at column 0 open; columns 1 and 2 decide: haplotype 1
        [A, N, G, T, C_],             # codons 0 and 1 open (they share column 1): haplotype 1 by the last
        [A, C_, N, T, C_],            # column 2 is part of all three: uninformative
        [A, C_, G, G, A],             # codon 1 and 2 mismatch both: none
    ]
    assert mirror(rows, pos, pat) == [0, 1, AMB, 1, 1, U, NONE]


def test_the_two_symbols_are_exported_and_listed():
    lib = capi.load_library()
    for name in ("jl_phase_rescue_async", "jl_phase_rescue_fetch"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "phase_rescue") and hasattr(capi.Juliet, "phase_rescue_fetch")


def run(exe, cwd, *args):
    return subprocess.run([exe, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


BOTH = ["--rescue-damaged", "--rescue-min-positions"]


@pytest.mark.parametrize("args, words", [
    (["--rescue-damaged"], ["--mode-phasing"]),                                                    # without phasing
    (["--mode-phasing", "--rescue-damaged", "--windows", "2"], ["--windows"]),
    (["--mode-phasing", "--rescue-damaged", "--devices", "0,0"], ["--devices"]),
    (["--mode-phasing", "--rescue-damaged", "--rescue-min-positions", "2", "--devices", "0,0", "--windows", "2"], ["--devices"]),
    (["--mode-phasing", "--rescue-min-positions", "2"], ["add it"]),                               # the threshold alone
    (["--mode-phasing", "--rescue-damaged", "--rescue-min-positions", "0"], ["at least one"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAM need not exist."""
    r = run(JULIET, tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in BOTH + words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_rescue_is_refused_with_batch(tmp_path):
    work = tmp_path / "work"
    work.mkdir()
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = run(JULIET, work, "--mode-phasing", "--rescue-damaged", "--batch", "../l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr and all(w in r.stderr for w in BOTH), r.stderr
    assert not list(work.iterdir())


def test_rescue_is_refused_as_fuse(tmp_path):
    r = run(FUSE, tmp_path, "--mode-phasing", "--rescue-damaged", "a.bam", "o.fasta")
    assert r.returncode == 1 and "fuse" in r.stderr and all(w in r.stderr for w in BOTH), r.stderr
    assert not list(tmp_path.iterdir())


def test_help_names_the_flags():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--rescue-damaged" in r.stderr and "--rescue-min-positions" in r.stderr
