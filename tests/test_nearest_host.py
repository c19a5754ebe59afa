"""The host-only half of the nearest-haplotype assignment (docs/SPEC.md §22): the rule's mirror (tests/nearest_mirror.py) on
hand-written rows with the expected answers spelled out, its agreement with the rescue's mirror at a budget of 0, the budgets
nesting, the two exports, and what the command line refuses of --absorb-distance before any file is read.  No GPU: the library
only has to load."""
import os
import subprocess

import numpy as np
import pytest

import nearest_mirror
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


def mirror(rows, pos_cols, pattern, min_positions, max_distance):
    """(nearest, dist) as lists, after the mirror's own sums have been checked against each other."""
    near, dist, hap_reads, tally = nearest_mirror.nearest(np.array(rows, dtype=np.uint8), pos_cols, np.array(pattern, dtype=np.uint8),
                                                          min_positions, max_distance)
    n_hap = len(pattern)
    assert hap_reads.shape == (n_hap, max_distance + 1)
    assert int(tally.sum()) == len(rows)
    assert hap_reads.tolist() == [[int(((near == h) & (dist == d)).sum()) for d in range(max_distance + 1)] for h in range(n_hap)]
    assert tally.tolist() == [int((near < n_hap).sum()), int((near == AMB).sum()), int((near == NONE).sum()), int((near == U).sum())]
    return near.tolist(), dist.tolist()


def test_the_constants():
    assert (nearest_mirror.UNINFORMATIVE, nearest_mirror.NONE, nearest_mirror.AMBIGUOUS) == (0xFFFB, 0xFFFC, 0xFFFD)
    assert (nearest_mirror.UNINFORMATIVE, nearest_mirror.NONE, nearest_mirror.AMBIGUOUS) == \
           (capi.RESCUE_UNINFORMATIVE, capi.RESCUE_NONE, capi.RESCUE_AMBIGUOUS)          # §14's own codes, no second set
    assert nearest_mirror.MAX_DISTANCE == capi.NEAREST_MAX_DISTANCE == 7


POS4 = [0, 3, 6, 9]
READ4 = [A, A, A, C_, C_, C_, G, G, G, T, T, T]


def test_a_unique_minimum_below_two_others():
    """One haplotype one codon away, two haplotypes two codons away: the first, at distance 1, from a budget of 1 on."""
    pat = [[codon(A, A, A), codon(C_, C_, C_), codon(G, G, G), codon(T, T, A)],        # differs at position 3
           [codon(A, A, C_), codon(C_, C_, C_), codon(G, G, G), codon(T, T, A)],       # at 0 and 3
           [codon(A, A, A), codon(C_, C_, A), codon(G, G, G), codon(T, T, C_)]]        # at 1 and 3
    assert mirror([READ4], POS4, pat, 1, 1) == ([0], [1])
    assert mirror([READ4], POS4, pat, 1, 7) == ([0], [1])
    assert mirror([READ4], POS4, pat, 1, 0) == ([NONE], [1])
    assert mirror([READ4], POS4, pat[::-1], 1, 2) == ([2], [1])                         # ... wherever it stands among them
    # a codon position counts once, however many of its bases differ
    all_three = [[codon(C_, C_, C_), codon(C_, C_, C_), codon(G, G, G), codon(T, T, T)]]
    assert mirror([READ4], POS4, all_three, 1, 1) == ([0], [1])


def test_a_tie_at_the_minimum():
    pat = [[codon(A, A, A), codon(C_, C_, C_), codon(G, G, G), codon(T, T, A)],
           [codon(A, A, A), codon(C_, C_, C_), codon(G, G, A), codon(T, T, T)],
           [codon(T, A, A), codon(C_, T, C_), codon(G, G, G), codon(T, T, T)]]         # two away: it does not break the tie
    assert mirror([READ4], POS4, pat, 1, 1) == ([AMB], [1])
    assert mirror([READ4], POS4, pat, 1, 2) == ([AMB], [1])                             # the tie is at dmin, whatever the budget admits
    assert mirror([READ4], POS4, pat, 1, 0) == ([NONE], [1])
    assert mirror([READ4], POS4, pat[1:], 1, 1) == ([0], [1])                           # without the first, the second alone


def test_the_budget_itself_and_one_above():
    pat = [[codon(A, A, A), codon(C_, C_, A), codon(G, G, A), codon(T, T, T)],         # two away
           [codon(T, A, A), codon(C_, C_, A), codon(G, G, A), codon(T, T, T)]]         # three away
    assert mirror([READ4], POS4, pat, 1, 2) == ([0], [2])                               # dmin = D: assigned
    assert mirror([READ4], POS4, pat, 1, 1) == ([NONE], [2])                            # dmin = D + 1: none, dist = D + 1
    assert mirror([READ4], POS4, pat, 1, 0) == ([NONE], [1])                            # ... which is all dist says of a read beyond the budget
    assert mirror([READ4], POS4, pat[1:], 1, 2) == ([NONE], [3])
    assert mirror([READ4], POS4, pat[1:], 1, 3) == ([0], [3])


def test_equal_pattern_rows_tie_and_one_haplotype_never_does():
    pos = [1]
    pat = [[codon(G, A, T)], [codon(G, A, C_)], [codon(G, A, T)]]
    rows = [[T, G, A, T], [T, G, A, C_], [T, G, A, A], [T, G, GAP, T]]
    assert mirror(rows, pos, pat, 1, 0) == ([AMB, 1, NONE, U], [0, 0, 1, 0xFF])
    assert mirror(rows, pos, pat, 1, 1) == ([AMB, 1, AMB, U], [0, 0, 1, 0xFF])         # one away from all three
    assert mirror(rows, pos, pat[:1], 1, 0) == ([0, NONE, NONE, U], [0, 1, 1, 0xFF])   # H = 1
    assert mirror(rows, pos, pat[:1], 1, 1) == ([0, 0, 0, U], [0, 1, 1, 0xFF])


def test_open_positions_count_for_nobody():
    """A gap, an N and an uncovered cell open the whole codon: it is no difference, and it is not informative."""
    pos = [0, 3, 6]
    pat = [[codon(A, A, A), codon(C_, C_, C_), codon(G, G, G)], [codon(A, A, A), codon(C_, C_, C_), codon(T, T, T)]]
    rows = [
        [A, A, A, C_, C_, C_, G, N, G],       # k = 2, the position where they differ is open: both at 0
        [A, A, T, GAP, C_, C_, T, T, T],      # k = 2, one away from haplotype 1, two from haplotype 0
        [N, A, A, GAP, C_, C_, T, T, C_],     # k = 1, one away from both
        [N, A, A, GAP, C_, C_, T, T, OUT],    # open everywhere
        [OUT] * 9,                            # code 6 throughout
    ]
    assert mirror(rows, pos, pat, 1, 1) == ([AMB, 1, AMB, U, U], [0, 1, 1, 0xFF, 0xFF])
    assert mirror(rows, pos, pat, 2, 1) == ([AMB, 1, U, U, U], [0, 1, 0xFF, 0xFF, 0xFF])
    assert mirror(rows, pos, pat, 3, 7) == ([U] * 5, [0xFF] * 5)


def positions(vp):
    cols = [0, 1][:vp] + [3 * k - 2 for k in range(2, vp)]
    return np.array(cols, dtype=np.uint32), cols[-1] + 3


def codons_at(base_rows, pos_cols):
    c = pos_cols.astype(np.int64)
    return (16 * base_rows[:, c] + 4 * base_rows[:, c + 1] + base_rows[:, c + 2]).astype(np.uint8)


def make_case(n, vp, n_hap, seed):
    """The generator of the rescue's device tests: haplotype rows in twins that differ by one base, reads that are copies of them
    with '-' and N cells, ragged code-6 ends, code 6 throughout, single substitutions, and the twins' position opened."""
    rng = np.random.default_rng(seed)
    pos_cols, n_cols = positions(vp)
    haps = rng.integers(0, 4, size=(n_hap, n_cols), dtype=np.uint8)
    twin_col = np.zeros(n_hap, dtype=np.int64)
    for h in range(1, n_hap, 2):
        haps[h] = haps[h - 1]
        twin_col[h] = twin_col[h - 1] = int(pos_cols[rng.integers(0, vp)]) + 2
        haps[h, twin_col[h]] = (haps[h, twin_col[h]] + 1 + rng.integers(0, 3)) % 4
    of = rng.integers(0, n_hap, size=n)
    rows = haps[of].copy()
    kind = rng.integers(0, 10, size=n)
    cell = rng.random(size=rows.shape)
    some = (kind == 0) | (kind == 1) | (kind == 2)
    rows[some[:, None] & (cell < 1.5 / n_cols)] = 4
    rows[some[:, None] & (cell > 1.0 - 1.5 / n_cols)] = 5
    lo, hi = rng.integers(0, n_cols // 3 + 1, size=n), n_cols - rng.integers(0, n_cols // 3 + 1, size=n)
    ci = np.arange(n_cols)[None, :]
    rows[(kind == 3)[:, None] & ((ci < lo[:, None]) | (ci >= hi[:, None]))] = 6
    rows[kind == 4] = 6
    for i in np.flatnonzero(kind == 5):
        c = int(pos_cols[rng.integers(0, vp)]) + int(rng.integers(0, 3))
        rows[i, c] = (rows[i, c] + 1 + rng.integers(0, 3)) % 4
    for i in np.flatnonzero(kind == 6):
        rows[i, twin_col[of[i]]] = 4 + int(rng.integers(0, 3))
    return rows, pos_cols, codons_at(haps, pos_cols)


GENERATED = [(200, 5, 6, 1), (300, 17, 9, 2), (150, 2, 3, 1), (257, 33, 65, "vp")]


@pytest.fixture(scope="module")
def generated():
    """Per case (rows, pos_cols, pattern, min_positions, the mirror at D = 0 .. 7): computed once, shared, left unchanged."""
    out = []
    for n, vp, n_hap, k in GENERATED:
        rows, pos_cols, pattern = make_case(n, vp, n_hap, 1000 * n + 7 * vp + n_hap)
        k = vp if k == "vp" else k
        out.append((rows, pos_cols, pattern, k, [nearest_mirror.nearest(rows, pos_cols, pattern, k, d) for d in range(8)]))
    return out


def test_budget_zero_is_the_rescue(generated):
    """Consequence (a): with D = 0, nearest equals §14's rescue for every read; hap_reads and tally with it."""
    ambiguous = 0
    for rows, pos_cols, pattern, k, by_d in generated:
        res, hap_reads, tally = rescue_mirror.rescue(rows, pos_cols, pattern, k)
        near, dist, near_reads, near_tally = by_d[0]
        assert tally[0] > 0 and tally[2] > 0 and tally[3] > 0
        ambiguous += int(tally[1])                         # (none where min_positions = Vp: an opened codon leaves the read unjudged)
        assert (near == res).all()
        assert (near_reads[:, 0] == hap_reads).all() and (near_tally == tally).all()
        assert (dist[res < len(pattern)] == 0).all() and (dist[res == AMB] == 0).all()
        assert (dist[res == NONE] == 1).all() and (dist[res == U] == 0xFF).all()
    assert ambiguous > 0


def test_budgets_nest(generated):
    """Consequence (b): dmin and the haplotypes at it do not depend on D.  A read assigned or ambiguous at one budget is the same,
    at the same distance, at every larger one; a read beyond one budget says so with dist = D + 1 and nothing else."""
    for rows, pos_cols, pattern, k, by_d in generated:
        n_hap = len(pattern)
        dmin = nearest_mirror.true_distance(rows, pos_cols, pattern)
        grew = False
        for d in range(8):
            near, dist, hap_reads, tally = by_d[d]
            judged = near != U
            within = judged & (dmin <= d)
            assert ((near == NONE) == (judged & (dmin > d))).all()
            assert (dist[within] == dmin[within]).all() and (dist[judged & ~within] == d + 1).all()
            if d:
                p_near, p_dist, p_reads, p_tally = by_d[d - 1]
                kept = p_near < n_hap
                assert (near[kept] == p_near[kept]).all() and (dist[kept] == p_dist[kept]).all()
                amb = p_near == AMB
                assert (near[amb] == AMB).all() and (dist[amb] == p_dist[amb]).all()
                assert (hap_reads[:, :d] == p_reads).all()
                assert tally[3] == p_tally[3] and tally[2] <= p_tally[2]
                grew = grew or tally[2] < p_tally[2]
        assert grew                                        # some read is taken in by a larger budget: nothing passes vacuously


def test_the_two_symbols_are_exported_and_listed():
    lib = capi.load_library()
    for name in ("jl_phase_nearest_async", "jl_phase_nearest_fetch"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "phase_nearest") and hasattr(capi.Juliet, "phase_nearest_fetch")


def run(exe, cwd, *args):
    return subprocess.run([exe, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, words", [
    (["--absorb-distance", "1"], ["--mode-phasing"]),                                              # without phasing
    (["--mode-phasing", "--absorb-distance", "0"], ["1 to 7"]),
    (["--mode-phasing", "--absorb-distance", "8"], ["1 to 7"]),
    (["--mode-phasing", "--absorb-min-positions", "2"], ["add it"]),                               # the threshold alone
    (["--mode-phasing", "--absorb-distance", "2", "--absorb-min-positions", "0"], ["at least one"]),
    (["--mode-phasing", "--absorb-distance", "1", "--windows", "2"], ["--windows"]),
    (["--mode-phasing", "--absorb-distance", "1", "--devices", "0,0"], ["--devices"]),
    (["--mode-phasing", "--absorb-distance", "1", "--absorb-min-positions", "2", "--devices", "0,0", "--windows", "2"], ["--devices"]),
    (["--mode-phasing", "--absorb-distance", "1", "--call-deletions", "--phase-deletions"], ["--phase-deletions"]),
    (["--mode-phasing", "--absorb-distance", "1", "--call-insertions", "--phase-insertions"], ["--phase-insertions"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAM need not exist."""
    r = run(JULIET, tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("juliet: --absorb-distance D [--absorb-min-positions K] "), r.stderr      # its own refusal, not the usage text
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_absorb_is_refused_with_batch(tmp_path):
    work = tmp_path / "work"
    work.mkdir()
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = run(JULIET, work, "--mode-phasing", "--absorb-distance", "1", "--batch", "../l.tsv")
    assert r.returncode == 1 and "--batch" in r.stderr and r.stderr.startswith("juliet: --absorb-distance"), r.stderr
    assert not list(work.iterdir())


def test_absorb_is_refused_as_fuse(tmp_path):
    r = run(FUSE, tmp_path, "--mode-phasing", "--absorb-distance", "1", "a.bam", "o.fasta")
    assert r.returncode == 1 and "fuse" in r.stderr and r.stderr.startswith("juliet: --absorb-distance"), r.stderr
    assert not list(tmp_path.iterdir())


def test_help_names_the_flags():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--absorb-distance" in r.stderr and "--absorb-min-positions" in r.stderr
