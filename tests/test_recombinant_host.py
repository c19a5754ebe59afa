"""The host-only half of the recombinant stage (docs/SPEC.md §23): the rule's mirror (tests/recombinant_mirror.py) on hand-written
rows with the expected answers spelled out, jl_haplotype_recombinants against the mirror's restatement of the haplotype-level rule,
the exports, and what the command line refuses of --flag-recombinants before any file is read.  No GPU: the library only has to
load."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recombinant_mirror
import rescue_mirror
from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
FUSE = os.path.join(ROOT, "minorseq_amd", "bin", "fuse")

U, NONE, AMB, WHOLE = 0xFFFB, 0xFFFC, 0xFFFD, 0xFFFA
A, C_, G, T, GAP, N, OUT = range(7)


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(FUSE)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def test_the_symbols_are_exported_and_listed():
    lib = capi.load_library()
    for name in ("jl_phase_recombinants_async", "jl_phase_recombinants_fetch", "jl_haplotype_recombinants"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "phase_recombinants") and hasattr(capi.Juliet, "phase_recombinants_fetch")


def test_the_constants():
    m = recombinant_mirror
    assert (m.UNINFORMATIVE, m.NONE, m.AMBIGUOUS) == (capi.RESCUE_UNINFORMATIVE, capi.RESCUE_NONE, capi.RESCUE_AMBIGUOUS)
    assert m.WHOLE == capi.RECOMB_WHOLE == 0xFFFA
    assert len({m.WHOLE, m.UNINFORMATIVE, m.NONE, m.AMBIGUOUS, capi.HAP_INSUFFICIENT, capi.HAP_DAMAGED}) == 6
    assert m.WHOLE > capi.MAX_HAPLOTYPES


# ---------------------------------------------------------------------------------------------- the mirror, by hand
# five codon positions at columns 0, 3, .. 12; haplotype X has base x at every cell
POS5 = [0, 3, 6, 9, 12]


def hap_row(*bases):
    """A read (or haplotype) of 15 columns from one base per codon: codon p is (b, b, b)."""
    return [b for b in bases for _ in range(3)]


def pat_of(*rows):
    return [[16 * r[c] + 4 * r[c + 1] + r[c + 2] for c in POS5] for r in rows]


HA, HC, HG = hap_row(A, A, A, A, A), hap_row(C_, C_, C_, C_, C_), hap_row(G, G, G, G, G)


def mirror(rows, pattern, min_positions=1, pos=POS5):
    out = recombinant_mirror.recombinants(np.array(rows, dtype=np.uint8), pos, pattern, min_positions)
    n_hap = len(pattern)
    left, right = out["left"], out["right"]
    both = (left < n_hap) & (right < n_hap)
    assert int(out["tally"].sum()) == len(rows)
    assert out["tally"].tolist() == [int(both.sum()), int((~both & ((left < n_hap) | (left == AMB))).sum()), int((left == WHOLE).sum()),
                                     int((left == NONE).sum()), int((left == U).sum())]
    assert out["parent_reads"].tolist() == [[int((both & (left == h)).sum()), int((both & (right == h)).sum())] for h in range(n_hap)]
    assert ((out["prefix"] == len(pos)) == (out["suffix"] == len(pos))).all()                       # consequence (b)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(left, right, out["prefix"], out["suffix"])]


def test_a_clean_breakpoint():
    pat = pat_of(HA, HC, HG)
    assert mirror([hap_row(A, A, C_, C_, C_)], pat) == [(0, 1, 2, 3)]            # A up to position 2, C from there: b = 2 only
    assert mirror([hap_row(C_, C_, C_, C_, A)], pat) == [(1, 0, 4, 1)]
    assert mirror([hap_row(G, A, A, A, A)], pat) == [(2, 0, 1, 4)]
    assert mirror([hap_row(A, A, C_, C_, C_)], pat[::-1]) == [(2, 1, 2, 3)]      # ... wherever the parents stand


def test_whole_none_and_uninformative():
    pat = pat_of(HA, HC, HG)
    assert mirror([HA, HG], pat) == [(WHOLE, WHOLE, 5, 5)] * 2
    assert mirror([hap_row(A, C_, A, C_, A)], pat) == [(NONE, NONE, 1, 1)]                  # alternating: far from one breakpoint
    assert mirror([hap_row(A, A, T, C_, C_)], pat) == [(NONE, NONE, 2, 2)]                  # a codon of neither between them
    assert mirror([hap_row(A, A, G, C_, C_)], pat) == [(NONE, NONE, 2, 2)]                  # three parents are two breakpoints
    assert mirror([hap_row(T, T, T, T, T)], pat) == [(NONE, NONE, 0, 0)]
    open_all = [OUT] * 15
    assert mirror([open_all], pat) == [(U, U, 5, 5)]                                         # prefix and suffix are the true values
    one = [OUT] * 12 + [A, A, A]
    assert mirror([one], pat, 2) == [(U, U, 5, 5)] and mirror([one], pat, 1) == [(WHOLE, WHOLE, 5, 5)]
    # uninformative comes first: a read that is a recombinant at two positions is not judged when three are asked for
    two = [A, A, A] + [GAP] * 9 + [C_, C_, C_]
    assert mirror([two], pat, 2) == [(0, 1, 4, 4)] and mirror([two], pat, 3) == [(U, U, 4, 4)]


def test_open_positions_at_the_junction_widen_the_interval():
    pat = pat_of(HA, HC, HG)
    r = hap_row(A, A, C_, C_, C_)
    r[6:9] = [N, N, N]                          # position 2 open: A agrees up to position 3, C from position 2 on
    assert mirror([r], pat) == [(0, 1, 3, 3)]   # breakpoints [5 - 3, 3] = {2, 3}
    r[3:6] = [GAP, A, A]                        # position 1 open too: the suffix of C grows
    assert mirror([r], pat) == [(0, 1, 3, 4)]   # {1, 2, 3}
    r[0:3] = [OUT] * 3                          # position 0 open as well: C agrees with the whole read
    assert mirror([r], pat) == [(WHOLE, WHOLE, 5, 5)]


def test_ties():
    assert mirror([hap_row(A, A, C_, C_, C_)], pat_of(HA, HC, HA)) == [(AMB, 1, 2, 3)]          # equal rows tie on their side
    assert mirror([hap_row(A, A, C_, C_, C_)], pat_of(HA, HC, HC)) == [(0, AMB, 2, 3)]
    assert mirror([hap_row(A, A, C_, C_, C_)], pat_of(HA, HC, HA, HC)) == [(AMB, AMB, 2, 3)]
    # a tie of DIFFERENT rows: they share the prefix the read uses
    assert mirror([hap_row(A, A, C_, C_, C_)], pat_of(hap_row(A, A, G, G, G), hap_row(A, A, T, T, T), HC)) == [(AMB, 2, 2, 3)]
    # a tie BELOW the maximum does not matter
    assert mirror([hap_row(A, A, C_, C_, C_)], pat_of(HA, HC, hap_row(A, G, G, G, G), hap_row(A, T, T, T, T))) == [(0, 1, 2, 3)]


def test_one_position_never_yields_a_recombinant():
    """Consequence (e)."""
    pat = [[0], [21], [42]]
    rows = [[A, A, A], [C_, C_, C_], [T, T, T], [N, A, A], [OUT] * 3]
    got = mirror(rows, pat, 1, pos=[0])
    assert got == [(WHOLE, WHOLE, 1, 1), (WHOLE, WHOLE, 1, 1), (NONE, NONE, 0, 0), (U, U, 1, 1), (U, U, 1, 1)]


def test_whole_is_where_the_rescue_finds_somebody():
    """Consequence (a), mirror against mirror, on seeded reads with gaps, Ns and uncovered cells."""
    rng = np.random.default_rng(3)
    pos = np.array([0, 1, 4, 7, 10, 13], dtype=np.uint32)
    haps = rng.integers(0, 3, size=(5, 16), dtype=np.uint8)
    haps[4] = haps[1]
    rows = haps[rng.integers(0, 5, size=300)].copy()
    cut = rng.integers(0, 16, size=300)
    other = haps[rng.integers(0, 5, size=300)]
    for i in range(150):
        rows[i, cut[i]:] = other[i, cut[i]:]
    cell = rng.random(size=rows.shape)
    rows[cell < 0.03] = GAP
    rows[cell > 0.97] = OUT
    rows[(cell > 0.5) & (cell < 0.52)] = 3
    pattern = (16 * haps[:, pos] + 4 * haps[:, pos + 1] + haps[:, pos + 2]).astype(np.uint8)
    for k in (1, 3, 6):
        out = recombinant_mirror.recombinants(rows, pos, pattern, k)
        res, _, tally = rescue_mirror.rescue(rows, pos, pattern, k)
        assert ((out["left"] == WHOLE) == ((res < 5) | (res == AMB))).all()
        assert ((out["left"] == U) == (res == U)).all()
        assert (out["tally"][:4] > 0).all()


# ---------------------------------------------------------------------------------------------- the haplotype level
def check_haps(pattern, counts, ratio=2.0):
    got = capi.haplotype_recombinants(np.array(pattern, dtype=np.uint8), counts, ratio)
    assert got == recombinant_mirror.haplotype_recombinants(pattern, counts, ratio)
    return got


def test_haplotype_level_by_hand():
    pat = [[1, 1, 1, 1], [2, 2, 2, 2], [1, 1, 2, 2], [2, 1, 1, 1]]
    got = check_haps(pat, [450, 450, 60, 10])
    assert got[2] == dict(flagged=True, left=0, right=1, prefix=2, suffix=2)
    assert got[3] == dict(flagged=True, left=1, right=0, prefix=1, suffix=3)
    assert got[0] == got[1] == dict(flagged=False, left=0, right=0, prefix=0, suffix=0)      # nobody has twice their reads
    # the clones themselves become candidates of each other at a ratio of 1, and are still no recombinants
    got = check_haps(pat, [450, 450, 60, 10], 1.0)
    assert got[0] == dict(flagged=False, left=1, right=1, prefix=0, suffix=0) and not got[1]["flagged"]


def test_haplotype_level_ratio_edges():
    pat = [[1, 1, 1], [2, 2, 2], [1, 2, 2]]
    assert check_haps(pat, [20, 20, 10])[2]["flagged"]                      # exactly r * count: a candidate
    assert not check_haps(pat, [20, 19, 10])[2]["flagged"]                  # one below: haplotype 1 is none, and 0 alone does not cover
    assert check_haps(pat, [20, 19, 10])[2] == dict(flagged=False, left=0, right=0, prefix=1, suffix=0)
    assert check_haps(pat, [25, 25, 10], 2.5)[2]["flagged"] and not check_haps(pat, [25, 24, 10], 2.5)[2]["flagged"]
    # the product is taken in double, as written: 1.1 * 50 is 55.00000000000001 there, so 55 reads are not enough; 2.3 * 50 is
    # 114.99999999999999, so 115 are (and 114 are not)
    assert 1.1 * 50 > 55 and 114 < 2.3 * 50 < 115
    assert not check_haps(pat, [55, 55, 50], 1.1)[2]["flagged"] and check_haps(pat, [56, 56, 50], 1.1)[2]["flagged"]
    assert check_haps(pat, [115, 115, 50], 2.3)[2]["flagged"] and not check_haps(pat, [114, 115, 50], 2.3)[2]["flagged"]
    assert check_haps(pat, [0, 0, 0])[2]["flagged"]                         # 0 >= r * 0


def test_haplotype_level_ties_go_to_the_lowest_index():
    pat = [[1, 1, 9, 9], [1, 1, 8, 8], [7, 7, 2, 2], [6, 6, 2, 2], [1, 1, 2, 2]]
    assert check_haps(pat, [50, 50, 50, 50, 5])[4] == dict(flagged=True, left=0, right=2, prefix=2, suffix=2)
    pat = [pat[1], pat[0], pat[3], pat[2], pat[4]]
    assert check_haps(pat, [50, 50, 50, 50, 5])[4] == dict(flagged=True, left=0, right=2, prefix=2, suffix=2)
    # identical prefixes: two rows equal to h up to its end are both whole parents
    pat = [[3, 3, 3], [3, 3, 3], [3, 3, 3]]
    assert check_haps(pat, [9, 9, 1])[2] == dict(flagged=True, left=0, right=0, prefix=3, suffix=3)


def test_haplotype_level_one_position_and_one_haplotype():
    assert check_haps([[5], [6], [5]], [9, 9, 1])[2] == dict(flagged=True, left=0, right=0, prefix=1, suffix=1)
    assert check_haps([[5], [6], [7]], [9, 9, 1])[2] == dict(flagged=False, left=0, right=0, prefix=0, suffix=0)
    assert check_haps([[5, 6]], [9]) == [dict(flagged=False, left=0, right=0, prefix=0, suffix=0)]


def test_haplotype_level_seeded():
    rng = np.random.default_rng(11)
    for n_hap, vp in ((2, 2), (7, 5), (40, 9), (702, 3)):
        pat = rng.integers(0, 2, size=(n_hap, vp), dtype=np.uint8)
        counts = rng.integers(1, 50, size=n_hap).astype(np.uint32)
        got = check_haps(pat.tolist(), counts.tolist(), 1.5)
        assert n_hap < 40 or (any(g["flagged"] for g in got) and not all(g["flagged"] for g in got))


def test_haplotype_level_a_row_stride():
    lib = capi.load_library()
    wide = np.full((3, 8), 63, dtype=np.uint8)
    wide[:, :3] = [[1, 1, 1], [2, 2, 2], [1, 2, 2]]
    counts = np.array([20, 20, 10], dtype=np.uint32)
    out = (capi.HapRecombinant * 3)()
    assert lib.jl_haplotype_recombinants(wide.ctypes.data, 8, 3, 3, counts.ctypes.data, 2.0, C.byref(out)) == 0
    assert (out[2].flagged, out[2].left, out[2].right, out[2].prefix, out[2].suffix) == (1, 0, 1, 1, 2)


def test_haplotype_level_refusals():
    lib = capi.load_library()
    pat = np.zeros((703, 4097), dtype=np.uint8)
    counts = np.ones(703, dtype=np.uint32)
    out = (capi.HapRecombinant * 703)()

    def refused(word, pattern=pat.ctypes.data, stride=4, n_hap=3, n_pos=4, hap_count=counts.ctypes.data, ratio=2.0, dst=C.byref(out)):
        assert lib.jl_haplotype_recombinants(pattern, stride, n_hap, n_pos, hap_count, ratio, dst) == -1
        assert word in lib.jl_last_error(None).decode(), lib.jl_last_error(None)

    assert lib.jl_haplotype_recombinants(pat.ctypes.data, 4, 3, 4, counts.ctypes.data, 2.0, C.byref(out)) == 0
    assert lib.jl_haplotype_recombinants(pat.ctypes.data, 4096, 702, 4096, counts.ctypes.data, 2.0, C.byref(out)) == 0      # the limits themselves
    refused("NULL", pattern=None)
    refused("NULL", hap_count=None)
    refused("NULL", dst=None)
    refused("min_parent_ratio", ratio=0.999)
    refused("min_parent_ratio", ratio=-2.0)
    refused("min_parent_ratio", ratio=float("nan"))
    refused("0 positions", n_pos=0)
    refused("4097 positions", n_pos=4097, stride=4097)
    refused("0 haplotypes", n_hap=0)
    refused("703 haplotypes", n_hap=703)
    refused("pattern_stride", stride=3)


# ---------------------------------------------------------------------------------------------- the command line
def run(exe, cwd, *args):
    return subprocess.run([exe, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


PREFIX = "juliet: --flag-recombinants [--recombinant-min-positions K] [--recombinant-parent-ratio r] "


@pytest.mark.parametrize("args, words", [
    (["--flag-recombinants"], ["--mode-phasing"]),                                                   # without phasing
    (["--mode-phasing", "--recombinant-min-positions", "2"], ["add it"]),                            # either sub-option alone
    (["--mode-phasing", "--recombinant-parent-ratio", "2"], ["add it"]),
    (["--mode-phasing", "--flag-recombinants", "--recombinant-min-positions", "0"], ["at least one"]),
    (["--mode-phasing", "--flag-recombinants", "--recombinant-parent-ratio", "0.99"], ["below 1"]),
    (["--mode-phasing", "--flag-recombinants", "--recombinant-parent-ratio", "-3"], ["below 1"]),
    (["--mode-phasing", "--flag-recombinants", "--windows", "2"], ["--windows"]),
    (["--mode-phasing", "--flag-recombinants", "--devices", "0,0"], ["--devices"]),
    (["--mode-phasing", "--flag-recombinants", "--call-deletions", "--phase-deletions"], ["--phase-deletions"]),
    (["--mode-phasing", "--flag-recombinants", "--call-insertions", "--phase-insertions"], ["--phase-insertions"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAM need not exist."""
    r = run(JULIET, tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith(PREFIX), r.stderr      # its own refusal, not the usage text
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_refused_with_batch(tmp_path):
    work = tmp_path / "work"
    work.mkdir()
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = run(JULIET, work, "--mode-phasing", "--flag-recombinants", "--batch", "../l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr and r.stderr.startswith(PREFIX), r.stderr
    assert not list(work.iterdir())


def test_refused_as_fuse(tmp_path):
    r = run(FUSE, tmp_path, "--mode-phasing", "--flag-recombinants", "a.bam", "o.fasta")
    assert r.returncode == 1 and "fuse" in r.stderr and r.stderr.startswith(PREFIX), r.stderr
    assert not list(tmp_path.iterdir())


def test_help_names_the_flags():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert all(w in r.stderr for w in ("--flag-recombinants", "--recombinant-min-positions", "--recombinant-parent-ratio"))
