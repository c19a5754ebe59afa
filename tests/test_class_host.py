"""The host-only half of the class pileup (docs/SPEC.md §13): the consensus rule over one count table
(jl_consensus_of_counts), the three exports, and what the command line refuses of --haplotype-fasta before any file is read.
No GPU: the library only has to load."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from minorseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")
FUSE = os.path.join(ROOT, "minorseq_amd", "bin", "fuse")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not (os.path.exists(JULIET) and os.path.exists(FUSE)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def mirror_consensus(counts):
    """The rule in numpy: the first (lowest) code among A C G T - with the most reads; 5 where none of the five has any.
    N (column 5 of the table) does not vote."""
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1, 6)
    out = np.argmax(counts[:, :5], axis=1).astype(np.uint8)      # argmax returns the first maximum
    out[counts[:, :5].max(axis=1) == 0] = 5
    return out


def edge_table():
    rows = []
    for a, b in itertools.combinations(range(5), 2):       # a tie between every pair of voting symbols: the lower code wins
        r = [1, 1, 1, 1, 1, 0]
        r[a] = r[b] = 7
        rows.append(r)
        r = [0] * 6                                        # ... and the same tie with nothing else in the column
        r[a] = r[b] = 3
        rows.append(r)
    rows.append([0, 0, 0, 0, 0, 0])                        # nobody covers the column: 5
    rows.append([0, 0, 0, 0, 0, 9])                        # only N: N does not vote, so nobody does: 5
    rows.append([1, 2, 0, 1, 5, 0])                        # a '-' majority: 4
    rows.append([3, 0, 4, 0, 0, 50])                       # N has the most reads and must not win: G
    rows.append([2, 2, 2, 2, 2, 2])                        # all equal: A
    rows.append([0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0])      # the counts are 32 bits wide
    return np.array(rows, dtype=np.uint32)


def test_consensus_of_counts_on_the_edges():
    t = edge_table()
    got = capi.consensus_of_counts(t)
    assert got.dtype == np.uint8 and got.shape == (len(t),)
    assert (got == mirror_consensus(t)).all()
    pairs = list(itertools.combinations(range(5), 2))
    assert got[:2 * len(pairs)].tolist() == [a for a, _ in pairs for _ in range(2)]       # spelled out: the lower code of each pair
    assert got[2 * len(pairs):].tolist() == [5, 5, 4, 2, 0, 3]


@pytest.mark.parametrize("seed,n_cols,high", [(1, 1, 3), (2, 1, 1000), (3, 257, 2), (4, 3000, 4), (5, 3000, 100000)])
def test_consensus_of_counts_equals_the_numpy_mirror(seed, n_cols, high):
    """Seeded tables; small `high` makes ties and all-zero columns frequent."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, high, size=(n_cols, 6), dtype=np.uint32)
    t[rng.random(n_cols) < 0.1] = 0
    assert (capi.consensus_of_counts(t) == mirror_consensus(t)).all()


def test_consensus_of_counts_refuses_null():
    lib = capi.load_library()
    out = np.zeros(4, dtype=np.uint8)
    t = np.zeros((4, 6), dtype=np.uint32)
    assert lib.jl_consensus_of_counts(None, 4, out.ctypes.data) == -1
    assert lib.jl_consensus_of_counts(t.ctypes.data, 4, None) == -1


def test_the_three_symbols_are_exported_and_listed():
    lib = capi.load_library()
    for name in ("jl_class_pileup_async", "jl_class_pileup_fetch", "jl_consensus_of_counts"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name)
    assert lib.jl_abi_version() == 5          # additive: the ABI version stays
    assert hasattr(capi.Juliet, "class_pileup") and callable(capi.consensus_of_counts)


def run(exe, cwd, *args):
    return subprocess.run([exe, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, words", [
    (["--haplotype-fasta", "h.fasta"], ["--haplotype-fasta", "--mode-phasing"]),                              # without phasing
    (["--mode-phasing", "--haplotype-fasta", "h.fasta", "--windows", "2"], ["--haplotype-fasta", "--windows"]),
    (["--mode-phasing", "--haplotype-fasta", "h.fasta", "--devices", "0,0"], ["--haplotype-fasta", "--devices"]),
    (["--mode-phasing", "--haplotype-fasta", "h.fasta", "--devices", "0,0", "--windows", "2"], ["--haplotype-fasta", "--devices"]),
])
def test_flag_combinations_the_command_line_refuses(tmp_path, args, words):
    """Exit 1 with a message, decided before any file is read or any device call is made: the BAM need not exist."""
    r = run(JULIET, tmp_path, *args, "a.bam", "o.json")
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not list(tmp_path.iterdir())


def test_haplotype_fasta_is_refused_with_batch(tmp_path):
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n")
    r = run(JULIET, tmp_path, "--mode-phasing", "--haplotype-fasta", "h.fasta", "--batch", "l.tsv")
    assert r.returncode == 1 and "--haplotype-fasta" in r.stderr and "--batch" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["l.tsv"]


def test_haplotype_fasta_is_refused_as_fuse(tmp_path):
    r = run(FUSE, tmp_path, "--mode-phasing", "--haplotype-fasta", "h.fasta", "a.bam", "o.fasta")
    assert r.returncode == 1 and "--haplotype-fasta" in r.stderr and "fuse" in r.stderr
    assert not list(tmp_path.iterdir())


def test_help_names_the_flag():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--haplotype-fasta" in r.stderr
    assert "Insertions are not included" in r.stderr
